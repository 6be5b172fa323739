/* vsc_hip.h -- C ABI of libvsc_hip.so, the MI355X (gfx950) hot path of the VSC22
 * descriptor track.  Plain pointers and sizes only; every pointer named *_dev is
 * device memory on the current HIP device, `stream` is a hipStream_t passed as
 * void* (NULL = default stream).  Every entry point returns 0 on success and a
 * negative vsc_status otherwise; vsc_last_error() gives the message of the last
 * failure on the calling thread.  Nothing here falls back to the CPU.
 *
 * Concurrency: one process per GPU is the deployment model.  An encoder handle, and the
 * search entry points as a group (vsc_knn_ip_f32, vsc_range_search_ip_f32, vsc_pair_similarity_f32,
 * vsc_video_pair_max_f32 share grow-only device scratch), must not be driven from two host threads at once, and
 * consecutive calls that share a handle or that scratch must be stream-ordered (same stream, or
 * ordered by events).  Different encoder handles are independent.
 *
 * Alignment: a device pointer is aligned to its element type unless its entry says "Alignment:" -- there the kernels read or write
 * the tensor 8 or 16 bytes at a time (dwordx4 accesses, LDS-DMA pieces), and a pointer less aligned than that is refused with
 * VSC_ERR_INVALID before anything is launched (the message names the argument).  Row-major operands have no leading dimension of
 * their own: with an aligned base their rows are aligned by the shape rules the entry already states (K % 64, N % 4, width % 4).
 * Offsets that an entry takes as ARGUMENTS are legal at any element: the element offsets of vsc_tn_align_f32,
 * vsc_match_segments_f32 and vsc_match_maps_f32, the row0 of vsc_pair_similarity_f32, the ld of vsc_pca_fit_update_f32.
 * Everything an allocator hands out (hipMalloc: 256 bytes, torch: 512) satisfies every requirement below.
 *
 * Each entry point names the reference interface it replaces
 * (paths relative to /root/reference/VSC22-Descriptor-Track-1st).
 */
#ifndef VSC_HIP_H
#define VSC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum vsc_status {
    VSC_OK = 0,
    VSC_ERR_INVALID = -1,     /* bad argument / unsupported shape */
    VSC_ERR_HIP = -2,         /* a HIP runtime call failed */
    VSC_ERR_NO_DEVICE = -3,   /* no gfx950 device visible */
    VSC_ERR_STATE = -4,       /* call order (e.g. forward before finalize) */
    VSC_ERR_NOMEM = -5
} vsc_status;

const char *vsc_last_error(void);
/* Number of visible HIP devices whose arch is gfx950; <0 on runtime failure. */
int vsc_device_count(void);
const char *vsc_version(void);
/* The 16-bit operand type of this build of the library: "bf16" (libvsc_hip.so, the configuration BASELINE.json names) or "fp16"
 * (libvsc_hip_f16.so: same kernels, same MFMA rate and bytes, 11 significand bits instead of 8; the infer/ entry points default to it
 * because the end-to-end uAP parity needs it).  Every `uint16_t *` tensor of the `*_bf16` kernel-level entry points
 * below holds THIS type's bit patterns; the entry points keep their names in both builds.  The similarity search and the fp32
 * convolutions are identical in both libraries (their bf16 stages are bf16 by construction). */
const char *vsc_operand_dtype(void);
/* Diagnostic / test switches (path forcing for the parity tests, A/B knobs of tools/micro).  Each switch VSC_<NAME> takes
 * its initial value from the environment variable of the same name, read ONCE per process; after that it changes only
 * through this call (name with or without the VSC_ prefix; value NULL or "" clears it).  No entry point reads the
 * environment on its launch path.  Unknown names return VSC_ERR_INVALID.  Not a reference interface: the reference has no
 * counterpart. */
int vsc_set_option(const char *name, const char *value);
/* Current value of a switch (NULL when unset or unknown); the string stays valid for the life of the process.  For callers
 * that change a switch temporarily and must restore what the environment or an enclosing scope had set. */
const char *vsc_get_option(const char *name);

/* ------------------------------------------------------------------------ *
 * Frame encoder: replaces `flat_features = model(flat_frames)` on the
 * TorchScript backbones -- infer/src/extractor.py:23, infer/extract_query_feats.py:150
 * (single_infer) and :171 (clip_model) -- for ViT-family backbones
 * (train/train_v115/vsc/baseline/model_factory/backbones/vit.py:10-54,
 *  train/train_vid_score/video/clip.py:82-161).
 * ------------------------------------------------------------------------ */
typedef struct vsc_encoder vsc_encoder;

typedef struct vsc_encoder_config {
    int32_t image_size;   /* square input, pixels */
    int32_t patch_size;
    int32_t channels;     /* 3 */
    int32_t width;        /* multiple of 64; head_dim must be 64 */
    int32_t layers;
    int32_t heads;
    int32_t mlp_dim;      /* multiple of 64 */
    int32_t out_dim;      /* Linear head outputs; 0 = emit the pooled feature */
    float ln_eps;
    int32_t act;          /* 0 = exact GELU (HF/timm), 1 = QuickGELU (clip.py:22) */
    int32_t pre_ln;       /* 1 = CLIP ln_pre after the position embedding */
    int32_t patch_bias;   /* 0 = bias-free patch conv (CLIP) */
    int32_t pool;         /* 0 = GeM over all tokens (vit.py:52), 1 = CLS token */
    float gem_p;
    int32_t max_batch;    /* frames per internal step; workspace is sized for it */
    int32_t l2_normalize; /* 1 = emit sklearn-style L2-normalised descriptors */
    int32_t head_conv_dim; /* >0: SSCD head (sscd.py:25-42): tokens -> Conv1d(width, head_conv_dim, 1)
                              -> GeM over tokens -> Linear(head_conv_dim, out_dim); needs pool = 0 */
    int32_t lanes;        /* 2: a forward call of more than max_batch frames alternates its chunks over
                             two internal streams (two workspaces) so memory-bound kernels of one
                             chunk overlap the GEMMs of the other; anything else = 1 */
    int32_t fuse_ln;      /* 1: LayerNorm folding -- LN2 / the next layer's LN1 applied inside the fc1 / qkv GEMM
                             epilogues from statistics the proj / fc2 write-out emits (no LN pass);
                             same results within the bf16 rounding noise, throughput-neutral on MI355X.  0: off */
} vsc_encoder_config;

int vsc_encoder_create(const vsc_encoder_config *cfg, vsc_encoder **out);
void vsc_encoder_destroy(vsc_encoder *enc);

/* Upload one weight tensor (float32, host memory, canonical names and layouts of
 * vsc_hip/weights.py: "patch.weight", "blocks.3.qkv.bias", "head.weight" ...).
 * `count` is the number of float32 elements and is checked against the config. */
int vsc_encoder_set_weight(vsc_encoder *enc, const char *name, const float *host, size_t count);
/* Check completeness, build the bf16 device copies.  Required before forward. */
int vsc_encoder_finalize(vsc_encoder *enc);

/* frames_dev: float32 [n, channels, image, image], already normalised as
 * infer/src/transform.py does.  desc_dev: float32 [n, desc_dim] where desc_dim =
 * out_dim ? out_dim : width.  Asynchronous on `stream`.
 * Alignment: frames_dev 16 bytes (the patch gather reads float4). */
int vsc_encoder_forward(vsc_encoder *enc, const float *frames_dev, int64_t n, float *desc_dev,
                        void *stream);
/* The same from DECODED frames: frames_u8_dev uint8 [n, image, image, channels] (PIL / numpy layout); torchvision's
 * ToTensor + Normalize(mean, std) (infer/src/transform.py:37-42, extract_query_feats.py:97-105) run inside the
 * patchify kernel in the reference's fp32 op order, so the result is bit-identical to vsc_encoder_forward on the fp32
 * tensor -- with a quarter of the bytes over PCIe and HBM.  mean / std: `channels` floats in HOST memory. */
int vsc_encoder_forward_u8(vsc_encoder *enc, const uint8_t *frames_u8_dev, int64_t n, const float *mean,
                           const float *std, float *desc_dev, void *stream);
/* Same, but also copies the last hidden state (after the final LayerNorm),
 * float32 [n, tokens, width], for parity tests.  tokens_dev may be NULL.  Alignment: frames_dev and tokens_dev 16 bytes. */
int vsc_encoder_forward_debug(vsc_encoder *enc, const float *frames_dev, int64_t n,
                              float *desc_dev, float *tokens_dev, void *stream);
int64_t vsc_encoder_workspace_bytes(const vsc_encoder *enc);

/* Per-kernel-class timing for bench.py's roofline: when on, every launch of
 * vsc_encoder_forward is bracketed by HIP events on the caller's stream.
 * vsc_encoder_get_profile synchronises the device, then returns the accumulated
 * milliseconds and launch counts per class since profiling was switched on. */
typedef enum vsc_prof_class {
    VSC_PROF_PATCHIFY = 0, VSC_PROF_GEMM_PATCH = 1, VSC_PROF_LAYERNORM = 2, VSC_PROF_GEMM_QKV = 3,
    VSC_PROF_ATTENTION = 4, VSC_PROF_GEMM_PROJ = 5, VSC_PROF_GEMM_FC1 = 6, VSC_PROF_GEMM_FC2 = 7,
    VSC_PROF_POOL_HEAD = 8, VSC_PROF_MISC = 9, VSC_PROF_CLASSES = 10
} vsc_prof_class;
int vsc_encoder_set_profiling(vsc_encoder *enc, int32_t on);
int vsc_encoder_get_profile(vsc_encoder *enc, double ms_out[VSC_PROF_CLASSES],
                            int64_t launches_out[VSC_PROF_CLASSES]);

/* ------------------------------------------------------------------------ *
 * Swin-Transformer-V2 frame encoder: replaces `model(flat_frames)` for the swinv2_v106/v107/v115
 * TorchScript backbones (infer/infer_ref.sh; model = train/train_v115/torch2scripts.py:480-657:
 * patch embed + norm, stages of res-post-norm blocks with windowed cosine attention and continuous
 * relative position bias, patch merging, final norm, GeM(p) over tokens, output_proj).
 * Weight names are the reference's state-dict names ("layers.2.blocks.5.attn.qkv.weight" ...).
 * Supported: head_dim 32, window 8, 12, 16 or 24 (after clipping to the feature map; 8 and 16 run the tuned kernel), mlp_ratio 4.
 * ------------------------------------------------------------------------ */
typedef struct vsc_swin vsc_swin;

typedef struct vsc_swin_config {
    int32_t image_size, patch_size, channels, embed_dim, stages;
    int32_t depths[4], heads[4];
    int32_t window_size;
    int32_t pretrained_window_sizes[4];
    int32_t mlp_ratio, out_dim;
    float ln_eps, gem_p;
    int32_t max_batch, l2_normalize;
} vsc_swin_config;

int vsc_swin_create(const vsc_swin_config *cfg, vsc_swin **out);
void vsc_swin_destroy(vsc_swin *enc);
int vsc_swin_set_weight(vsc_swin *enc, const char *name, const float *host, size_t count);
int vsc_swin_finalize(vsc_swin *enc);
/* frames_dev f32 [n, channels, image, image] -> desc_dev f32 [n, out_dim]; asynchronous on `stream`.  Alignment: frames_dev 16 bytes
 * (and tokens_dev of vsc_swin_forward_debug). */
int vsc_swin_forward(vsc_swin *enc, const float *frames_dev, int64_t n, float *desc_dev, void *stream);
/* uint8 [n, image, image, channels] input, normalisation fused as in vsc_encoder_forward_u8 */
int vsc_swin_forward_u8(vsc_swin *enc, const uint8_t *frames_u8_dev, int64_t n, const float *mean, const float *std,
                        float *desc_dev, void *stream);
/* also returns the last-stage tokens after the final LayerNorm, f32 [n, tokens_last, width_last] */
int vsc_swin_forward_debug(vsc_swin *enc, const float *frames_dev, int64_t n, float *desc_dev,
                           float *tokens_dev, void *stream);
int64_t vsc_swin_workspace_bytes(const vsc_swin *enc);

/* Per-kernel-class timing for bench.py's Swin roofline, as vsc_encoder_set_profiling: when on, every launch of
 * vsc_swin_forward is bracketed by HIP events on the stream it runs on, and the chunks of a call run back to back on the
 * caller's stream (no lanes), so every kernel is timed alone.  Classes: patchify, patch embedding (GEMM + LayerNorm), then
 * per stage s (0..3) at VSC_SWIN_PROF_STAGE0 + s * VSC_SWIN_PROF_PER_STAGE: qkv GEMM, window attention, proj GEMM with the
 * res-post-norm LayerNorm, fc1 GEMM (+GELU), fc2 GEMM with its LayerNorm, patch merging (gather + reduction GEMM +
 * LayerNorm); last the final LayerNorm + GeM + head.  vsc_swin_get_profile synchronises the device. */
enum {
    VSC_SWIN_PROF_PATCHIFY = 0, VSC_SWIN_PROF_PATCH_EMBED = 1, VSC_SWIN_PROF_POOL_HEAD = 2, VSC_SWIN_PROF_STAGE0 = 3,
    VSC_SWIN_PROF_QKV = 0, VSC_SWIN_PROF_ATTENTION = 1, VSC_SWIN_PROF_PROJ_LN = 2, VSC_SWIN_PROF_FC1 = 3,
    VSC_SWIN_PROF_FC2_LN = 4, VSC_SWIN_PROF_MERGE = 5, VSC_SWIN_PROF_PER_STAGE = 6, VSC_SWIN_PROF_CLASSES = 27
};
int vsc_swin_set_profiling(vsc_swin *enc, int32_t on);
int vsc_swin_get_profile(vsc_swin *enc, double ms_out[VSC_SWIN_PROF_CLASSES], int64_t launches_out[VSC_SWIN_PROF_CLASSES]);

/* ------------------------------------------------------------------------ *
 * CNN frame encoder: the VSC22 baseline's descriptor model, the SSCD ResNet-50 (infer/vsc/baseline: a TorchScript model adapted
 * from sscd_disc_mixup.torchvision.pt) -- torchvision's ResNet-50 v1.5 without fc, GeM(p) over the last map, Linear, optional L2.
 * Convolutions run on the 16-bit matrix pipe in the library's operand type with fp32 accumulation (csrc/conv16.hip); BatchNorm is
 * folded into weight + bias by the caller.  Tensor names: conv1.{weight,bias}, layerL.B.conv{1,2,3}.{weight,bias} (L = 1..4),
 * layerL.0.downsample.{weight,bias}, head.{weight,bias}; convolution weights as [cout, cin, kh, kw] fp32.
 * Frames of ANY H, W >= 1 are taken, (n, H, W) per call; a frame's descriptor does not depend on what else is in the call.
 * ------------------------------------------------------------------------ */
typedef struct vsc_cnn_encoder vsc_cnn_encoder;

typedef struct vsc_cnn_encoder_config {
    int32_t stem_width;      /* 64 */
    int32_t widths[4];       /* stage output widths (256, 512, 1024, 2048): multiples of 256, the bottleneck width is a quarter */
    int32_t depths[4];       /* (3, 4, 6, 3) */
    int32_t head_in, head_out; /* head_in = widths[3] <= 2048; head_out <= 2048 */
    float gem_p;
    int32_t l2;              /* 0: the adapted model's un-normalised projection; 1: the original model's L2-normalised descriptor */
    int64_t max_pixels;      /* largest n * H * W of one call: sizes the workspace (for even H, W; odd extents grow it once) */
} vsc_cnn_encoder_config;

int vsc_cnn_encoder_create(const vsc_cnn_encoder_config *cfg, vsc_cnn_encoder **out);
void vsc_cnn_encoder_destroy(vsc_cnn_encoder *enc);
int vsc_cnn_encoder_set_weight(vsc_cnn_encoder *enc, const char *name, const float *host, size_t count);
int vsc_cnn_encoder_finalize(vsc_cnn_encoder *enc);
/* The stream comes first, as in the entries of the exact L2 search.
 * frames_dev f32 [n, 3, h, w], already normalised -> desc_dev f32 [n, head_out]; asynchronous on `stream` (a call whose odd extents
 * need a larger workspace than any call before waits for the device once).  Refused before anything is launched, with nothing
 * written: a null handle or pointer, n < 0, h or w < 1, n * h * w above max_pixels (VSC_ERR_INVALID); a handle that is not
 * finalized (VSC_ERR_STATE). */
int vsc_cnn_encoder_forward(void *stream, vsc_cnn_encoder *enc, const float *frames_dev, int64_t n, int32_t h, int32_t w, float *desc_dev);
/* uint8 [n, h, w, 3] input; mean / std: host arrays of 3; (v / 255 - mean) / std in fp32, the order of ToTensor + Normalize */
int vsc_cnn_encoder_forward_u8(void *stream, vsc_cnn_encoder *enc, const uint8_t *frames_u8_dev, int64_t n, int32_t h, int32_t w,
                               const float *mean, const float *std, float *desc_dev);
int64_t vsc_cnn_encoder_workspace_bytes(const vsc_cnn_encoder *enc);
/* Per-class timing as vsc_swin_set_profiling: stem rows, stem convolution, max-pool, the four stages, GeM + head. */
enum {
    VSC_CNN_PROF_STEM_ROWS = 0, VSC_CNN_PROF_STEM_CONV = 1, VSC_CNN_PROF_MAXPOOL = 2, VSC_CNN_PROF_STAGE0 = 3, VSC_CNN_PROF_POOL_HEAD = 7,
    VSC_CNN_PROF_CLASSES = 8
};
int vsc_cnn_encoder_set_profiling(vsc_cnn_encoder *enc, int32_t on);
int vsc_cnn_encoder_get_profile(vsc_cnn_encoder *enc, double ms_out[VSC_CNN_PROF_CLASSES], int64_t launches_out[VSC_CNN_PROF_CLASSES]);

/* Building blocks of the CNN encoder (csrc/conv16.hip), in the library's 16-bit operand type whatever the name's suffix says (as
 * vsc_gemm_bf16).  All NHWC, asynchronous on `stream` (their first argument), every refusal (VSC_ERR_INVALID) named before anything is launched.
 *
 * vsc_conv2d_nhwc_bf16: out[n, ho, wo, cout] = act(bias + conv(in[n, h, w, cin], w[cout, ksize, ksize, cin]) + residual), fp32
 * accumulation, one rounding to the operand type at the store.  ksize 1 or 3, stride 1 or 2, padding (ksize - 1) / 2 with zeros,
 * ho = (h + 2 pad - ksize) / stride + 1.  cin a multiple of 64, cout a multiple of 4.  bias_dev [cout] fp32 and residual_dev
 * [n, ho, wo, cout] may be NULL; relu != 0 clamps at zero last.  Alignment: in_dev, w_dev 16 bytes; residual_dev, out_dev 8 bytes.
 * vsc_maxpool3x3s2_nhwc_bf16: 3 x 3, stride 2, pad 1, the maximum over the taps inside the image; c a multiple of 8; 16-byte aligned.
 * vsc_stem_rows_u8: im2col rows of the 7 x 7 stride-2 pad-3 stem: rows_dev [n ho wo, 192], k = (r * 7 + s) * 3 + c, zeros for
 * k >= 147 and for taps outside the image.  Exactly one of frames_u8_dev [n, h, w, 3] (normalised with the host arrays mean / std as
 * above) and frames_f32_dev [n, 3, h, w] (already normalised).  rows_dev 16-byte aligned. */
int vsc_conv2d_nhwc_bf16(void *stream, const uint16_t *in_dev, const uint16_t *w_dev, const float *bias_dev, const uint16_t *residual_dev,
                         uint16_t *out_dev, int64_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t ksize, int32_t stride,
                         int32_t relu);
int vsc_maxpool3x3s2_nhwc_bf16(void *stream, const uint16_t *in_dev, uint16_t *out_dev, int64_t n, int32_t h, int32_t w, int32_t c);
int vsc_stem_rows_u8(void *stream, const uint8_t *frames_u8_dev, const float *frames_f32_dev, int64_t n, int32_t h, int32_t w,
                     const float *mean, const float *std, uint16_t *rows_dev);

/* ------------------------------------------------------------------------ *
 * Flat inner-product search: replaces faiss.IndexFlat(d, METRIC_INNER_PRODUCT)
 *   .search(x, k)        infer/vsc/index.py:167-175, infer/vsc/baseline/score_normalization.py:95,141,
 *                        infer/vsc/exhaustive_search.py:66 (the k = 1024 probe of range_search_gpu)
 *   .range_search(x, r)  infer/vsc/exhaustive_search.py:78,250
 * Scores are the ascending-k float32 fmaf chain (bit-identical to
 * oracle/knn_oracle.c); ties rank the lower reference index first.
 * ------------------------------------------------------------------------ */

/* q_dev [nq,d], r_dev [nr,d] float32 row-major, 1 <= d <= 4096, 1 <= k <= 1024.  out_scores_dev [nq,k] float32 descending, out_ids_dev [nq,k]
 * int64; slots beyond nr hold (-FLT_MAX, -1).  ref_id_offset is added to every
 * reported id (a shard of a larger bank).
 * Workspace: allocated internally, grow-only, cached per device (bf16 copies of both banks, candidate lists, partial
 * results: ~7 GB after a 1M x 1M call); vsc_search_release_scratch() returns it.  One search call per device at a time.
 * Host synchronisation: on the bf16 pre-filter path (nq * nr >= 2^24, nr >= 4096, k <= 512) the call waits for `stream`
 * once, after the merge, to read the per-block fallback flags -- on return the results are complete; on the exact path
 * (everything smaller) the call only enqueues.
 * Alignment: q_dev, r_dev and the outputs at their element type -- except rows narrower than 32 floats whose width is a multiple of 4
 * (d = 4, 8, .. 28): r_dev 16 bytes (the pre-filter path's re-scoring reads such rows as float4).  The same holds for
 * vsc_knn_ip_floor_f32, vsc_range_search_ip_f32 and vsc_video_pair_max_f32. */
int vsc_knn_ip_f32(const float *q_dev, int64_t nq, const float *r_dev, int64_t nr, int32_t d,
                   int32_t k, int64_t ref_id_offset, float *out_scores_dev,
                   int64_t *out_ids_dev, void *stream);

/* vsc_knn_ip_f32 with a per-query floor: the k best of {r : <q, r> >= floor_dev[q]}, unused slots (-FLT_MAX, -1).  For a bank swept
 * shard by shard (the pipelined form of the sharded search, infer/vsc/baseline/score_normalization.py:107-150 at configs[3]'s
 * size): floor = the k-th best score of the shards merged so far -- nothing below it can enter the final list, ties at the floor
 * still can (lower id first) -- so a later shard's lists start with a threshold instead of paying their warm-up appends again
 * (a 1M x 125k sweep runs at 870 TFLOP/s, the same rows as one of eight shards behind a floor at the whole bank's rate).
 * floor_dev NULL: vsc_knn_ip_f32.  -FLT_MAX / -inf entries: no floor for that query. */
int vsc_knn_ip_floor_f32(const float *q_dev, int64_t nq, const float *r_dev, int64_t nr, int32_t d, int32_t k,
                         int64_t ref_id_offset, const float *floor_dev, float *out_scores_dev, int64_t *out_ids_dev,
                         void *stream);

/* Merge of per-shard results of vsc_knn_ip_f32 (a bank swept shard by shard, each with its ref_id_offset -- the pipelined form of
 * the sharded search, where shard s is swept while shard s + 1 is still arriving over xGMI): scores / ids [parts][nq][k], every
 * list in the search's order (score descending, equal scores by ascending id; unused slots (-FLT_MAX, -1)) -> the k best of the
 * union in that same order.  parts <= 64.  Equals one vsc_knn_ip_f32 call over the concatenated bank bit for bit
 * (reference: faiss merges its shards' heaps the same way; infer/vsc/index.py:167-175 searches one flat index). */
int vsc_knn_merge_parts_f32(const float *scores_dev, const int64_t *ids_dev, int32_t parts, int64_t nq, int32_t k,
                            float *out_scores_dev, int64_t *out_ids_dev, void *stream);

/* Frees the search scratch (top-k, range search, video-pair maxima) of the current device after waiting for the device;
 * returns the bytes released.  The next search call allocates again. */
int64_t vsc_search_release_scratch(void);

/* Diagnostic: which sweep the last vsc_knn_ip_f32 call of this process took -- 1 the exact fp32 MFMA sweep, 2 the
 * bf16 pre-filter sweep + exact re-scoring (large problems, k <= 512; results are bit-identical to 1; synchronises
 * `stream` once to read its fallback flag), 3 the pre-filter ran, but some 256-query blocks (a candidate band did not fit,
 * or non-finite operands) were redone on the exact sweep.  vsc_set_option("VSC_KNN_PATH", "exact"|"bf16") forces a path. */
int vsc_knn_last_path(void);

/* Diagnostic (bench.py): with profiling on, every vsc_knn_ip_f32 call records HIP events on its stream around its phases;
 * vsc_knn_last_profile waits for the last call and returns ms_out = {pack, sweep (the dominant kernel: knn_sweep_bf16_kernel
 * on path 2, knn_kernel on path 1), exact re-scoring (0 on path 1), merge}. */
void vsc_knn_set_profiling(int on);
int vsc_knn_last_profile(float ms_out[4]);

/* Range search: every pair with <q,r> > radius -- faiss IndexFlat.range_search
 * (infer/vsc/exhaustive_search.py:78,250; the radius sweep behind
 * infer/vsc/index.py:145-165).  lims_dev [nq+1] int64 receives the CSR offsets, *total_out
 * (host) the number of hits.  Hits of query i go to [lims[i], lims[i+1]) of out_scores_dev /
 * out_ids_dev in ascending reference id, but only if total <= capacity; otherwise nothing is
 * written and the caller calls again with capacity >= *total_out (capacity 0 = count only).
 * Synchronises `stream` once (to read the total). */
int vsc_range_search_ip_f32(const float *q_dev, int64_t nq, const float *r_dev, int64_t nr,
                            int32_t d, float radius, int64_t ref_id_offset, int64_t *lims_dev,
                            float *out_scores_dev, int64_t *out_ids_dev, int64_t capacity,
                            int64_t *total_out, void *stream);
/* Which path the last vsc_range_search_ip_f32 call took: 1 = exact (two fp32 sweeps: count, fill), 2 = bf16 pre-filter (one bf16
 * sweep with the radius as a fixed threshold, survivors re-scored with the exact fp32 chain, scan, emit: same CSR output bit for
 * bit), 3 = pre-filter abandoned because a (query, reference split) list held more than 1024 survivors, then exact.  Chosen like
 * vsc_knn_ip_f32's path; VSC_RANGE_PATH=exact|bf16 forces one. */
int vsc_range_search_last_path(void);

/* ------------------------------------------------------------------------ *
 * Flat squared-L2 search: replaces faiss.IndexFlat(d, METRIC_L2).search / .range_search (infer/vsc/index.py:76-99; the
 * reference's tests/test_index.py builds one).  Contract (executable form: tests/l2_search_contract.py):
 *
 *   Distance.  dist(q, r) = c_d with c_0 = +0.0f, t_j = q_j - r_j (one float32 rounding), c_{j+1} = fmaf(t_j, t_j, c_j), j
 *   ascending; nothing is reassociated -- the L2 twin of the ascending-k float32 fmaf chain of vsc_knn_ip_f32.  A distance is a
 *   function of its pair alone: it equals any slice of a larger call bit for bit, whichever path found the pair.
 *   Top-k.  The k smallest distances over ALL nr rows, ascending, equal distances by ascending id; unused slots hold
 *   (FLT_MAX, -1), as faiss pads.  A NaN or infinite distance is never reported (faiss's heap comparison rejects both).
 *   ref_id_offset is added to every reported id.  The result equals brute force for every input, far clusters included:
 *   the inner-product sweep on augmented operands only SELECTS candidates, and a row's list is taken from it only when
 *   D_k < -s'_kk - slack(q), strictly (D_k: the k-th chain distance among the kk candidates, s'_kk: the kk-th expanded score,
 *   slack(q): a bound on |expanded score + chain distance| over the bank) -- then no row outside the probe can beat
 *   or tie the list -- or when the probe held the whole bank.  Every other row gets one wider probe under the same rule and is
 *   then answered by a direct path that depends on no bound (chain distances against all rows, radix select on the bits, lower id first among equals).
 *   Range.  Every pair with dist < radius, strict; CSR output query-major, ascending id inside a query; the count / capacity
 *   protocol of vsc_range_search_ip_f32.
 *
 * The stream is the FIRST parameter of these entries.  Scratch: the search's grow-only per-device buffers (slots of their own,
 * beside those of the inner-product sweep they call; vsc_search_release_scratch frees them).  One search call per device at a time.
 * Alignment: every pointer at its element type, except r_aug_dev: 16 bytes when d + 2 is a multiple of 4 below 32 (it is the
 * bank of a vsc_knn_ip_f32 sweep).  VSC_L2_PATH=probe|direct forces a path (probe: the sweep even for a bank one probe holds
 * whole; rows it cannot certify still take the wider probe and the direct path).
 * ------------------------------------------------------------------------ */

/* Augmented rows for the sweep, from plain rows x_dev [n, d], 1 <= d <= 4094: aug_dev [n, d + 2] = [x, |x|^2, 1] (as_query == 0: bank
 * rows) or [2x, -1, -|x|^2] (queries); norms_dev [n] = |x|^2; max_norm_dev [1] = the largest |x|^2 of the rows (non-finite if any row's
 * is).  Each output may be NULL.  |x|^2 is a float32 sum of fmaf partial sums; a row whose |x|^2 is not finite is written as a zero
 * row ([0, FLT_MAX, 1] / [0, -1, 0]).  These values only steer the selection: their bits are no part of the contract, their
 * rounding is part of slack.  Done once per bank.  Only enqueues on `stream`; no host synchronisation. */
int vsc_l2_augment_f32(void *stream, const float *x_dev, int64_t n, int32_t d, int32_t as_query, float *aug_dev, float *norms_dev,
                       float *max_norm_dev);

/* q_dev [nq, d], r_dev [nr, d] float32 row-major (the PLAIN rows), 1 <= k <= 1024; 1 <= d <= 4094 on the probe path, d <= 4096 on the
 * direct path (d = 4095, 4096: always direct).  r_aug_dev [nr, d + 2] / r_max_norm_dev [1]: the bank's vsc_l2_augment_f32 outputs
 * (aug_dev, max_norm_dev), or both NULL: the bank is augmented into scratch for this call.  out_dist_dev [nq, k] float32 ascending,
 * out_ids_dev [nq, k] int64.  nq == 0: nothing is written; nr == 0: every slot (FLT_MAX, -1).  Anything else is refused by name with
 * nothing written.
 * Host synchronisation: a call that probes waits for `stream` once after the re-scoring, to read one certificate flag per query
 * row (plus whatever the vsc_knn_ip_f32 sweep inside waits for), and, if some rows are not certified, once more to upload their
 * list; the wider probe of those rows repeats the two; the direct path itself (banks of at most max(k + 8, 2k) rows,
 * VSC_L2_PATH=direct) only enqueues. */
int vsc_knn_l2_f32(void *stream, const float *q_dev, int64_t nq, const float *r_dev, int64_t nr, int32_t d, int32_t k,
                   int64_t ref_id_offset, const float *r_aug_dev, const float *r_max_norm_dev, float *out_dist_dev,
                   int64_t *out_ids_dev);

/* Diagnostic: the query rows of the last vsc_knn_l2_f32 call of this process by path -- rows_out[0] certified at the first probe
 * (kk = max(k + 8, 2k) ranks, at most 1024), rows_out[1] certified at the one wider probe (4 kk ranks, at least 256, at most 1024; there
 * is none when that would hold the whole bank, or with VSC_L2_WIDE=0), rows_out[2] answered by the direct path. */
int vsc_knn_l2_last_path(int64_t rows_out[3]);

/* Range search, operands as vsc_knn_l2_f32, outputs as vsc_range_search_ip_f32: lims_dev [nq + 1] int64 CSR offsets, *total_out
 * (host) the number of hits; hits are written only if total <= capacity, otherwise the caller calls again with capacity >=
 * *total_out (capacity 0 = count only).  Sweep: the inner-product range sweep on the augmented operands at radius + slack (a
 * superset by the bound), the chain on the survivors, dist < radius, a prefix sum; the direct form (VSC_L2_PATH=direct, d > 4094,
 * no finite bound) materialises chain distances instead.  No hit goes to the host, only the totals.
 * Host synchronisation: on the sweep path the call waits for `stream` once to read the two norm maxima, once per
 * vsc_range_search_ip_f32 sweep inside (one, or two when the survivors outgrow the scratch) and once to read the total; on the
 * direct path once, to read the total. */
int vsc_range_search_l2_f32(void *stream, const float *q_dev, int64_t nq, const float *r_dev, int64_t nr, int32_t d, float radius,
                            int64_t ref_id_offset, const float *r_aug_dev, const float *r_max_norm_dev, int64_t *lims_dev,
                            float *out_dist_dev, int64_t *out_ids_dev, int64_t capacity, int64_t *total_out);

/* Per-candidate-pair frame similarity matrices -- the temporal alignment input of the matching track
 * (VSC22-Matching-Track-1st/infer/src/utils.py:29-51,66: np.matmul(qfeat, rfeat.T) per candidate).
 * q_dev [nq, d], r_dev [nr, d]: row banks (all query / reference videos' frames, concatenated).
 * pairs_host [n_pairs][4] = {q_row0, q_rows, r_row0, r_rows} (HOST memory).  Writes out_offsets_host
 * [n_pairs + 1] (element offsets; HOST memory) and out_dev[out_offsets[p] + i * r_rows + j] =
 * <q[q_row0 + i], r[r_row0 + j]> as the ascending-k fp32 fma chain of vsc_knn_ip_f32, so a matrix equals any
 * slice of a larger product bit for bit.  capacity = floats available at out_dev (>= sum q_rows * r_rows;
 * call with out_dev = NULL, capacity = 0 is an error unless the total is 0). */
int vsc_pair_similarity_f32(const float *q_dev, int64_t nq, const float *r_dev, int64_t nr, int32_t d,
                            const int64_t *pairs_host, int64_t n_pairs, int64_t *out_offsets_host,
                            float *out_dev, int64_t capacity, void *stream);

/* Video-pair maxima -- the candidate retrieval of the matching track
 * (VSC22-Matching-Track-1st/infer/infer_matching.py:229-262: per query frame top-1024, range_search where the
 * 1024th score still clears SEARCH_THRESHOLD, then max per (query video, reference video) in a dict).  The
 * union of the two faiss branches is {(qf, rf): <qf, rf> > threshold}; this entry point sweeps all pairs once
 * and keeps, per video pair, the largest frame score above `threshold` (strict, as in the reference).
 * q_video_dev [nq] / r_video_dev [nr]: int32 video index of every row (0 <= index < n_*_videos).
 * lims_dev [n_q_videos + 1] int64 receives CSR offsets over query videos, *total_out (host) the number of
 * video pairs.  Pairs of query video v go to [lims[v], lims[v+1]) of out_rvideo_dev / out_score_dev in
 * ascending reference video, but only if total <= capacity; otherwise nothing is written and the caller
 * calls again with capacity >= *total_out (capacity 0 = count only).  Scores are the fp32 chains of
 * vsc_knn_ip_f32 (bit-exact).  Uses a dense n_q_videos x n_r_videos uint32 table in scratch.
 * Synchronises `stream` once (to read the total). */
int vsc_video_pair_max_f32(const float *q_dev, int64_t nq, const int32_t *q_video_dev, int32_t n_q_videos,
                           const float *r_dev, int64_t nr, const int32_t *r_video_dev, int32_t n_r_videos,
                           int32_t d, float threshold, int64_t *lims_dev, int32_t *out_rvideo_dev,
                           float *out_score_dev, int64_t capacity, int64_t *total_out, void *stream);
/* Which sweep the last vsc_video_pair_max_f32 call ran: 1 = exact fp32 sweep, 2 = bf16 pre-filter (fixed-threshold variant of the
 * top-k pre-filter: survivors of s~ >= threshold - eps are re-scored with the exact fp32 chain before they reach the table, so
 * the result is the same table), 3 = pre-filter with some blocks of 256 queries redone on the exact sweep (a (query, reference
 * split) list held more than 1024 survivors).  Chosen like vsc_knn_ip_f32's path; VSC_PAIRMAX_PATH=exact|bf16 forces one. */
int vsc_video_pair_max_last_path(void);

/* Global top-k of frame pairs -- the selection behind the descriptor track's candidates (infer/vsc/index.py:145-165: every hit
 * inside the radius sorted by score and cut to global_k; infer/vsc/candidates.py:24-40 consumes the list) -- over a probe that
 * stays on the device: the search's [nq, k'] result, a range sweep's CSR hits, or the union of several ranks' selections.
 * scores_dev / ids_dev [n]; rows_dev [n] int64, or NULL: the row of entry p is p / row_stride (a row-major [nq, row_stride]
 * probe).  Entries with ids[p] < 0 are not candidates (the search's (-FLT_MAX, -1) padding).  Among the rest the
 * m = min(want, valid) entries with the largest score are written best first to out_rows_dev / out_ids_dev / out_scores_dev
 * (each [min(want, n)]; scores keep their bits) and m to out_count_dev [1] (device).  Equal scores keep their input order, and
 * -0.0f equals +0.0f: the list is the head of a stable descending sort by score.  Scores are finite or infinite; NaN is
 * outside the contract (it neither faults nor hangs, its place in the order is unspecified).  n < 2^31.  n == 0 or want == 0
 * writes count 0 and launches nothing that reads the inputs.
 * The result is a pure function of the inputs: integer atomics only accumulate histogram counts, every output position comes
 * from a prefix scan.  Passes: radix select of the want-th key (4 histogram sweeps), stable compaction of the entries above it
 * and of the first entries equal to it, stable 8-bit LSD radix sort of the survivors, gather.  The compaction works on tiles
 * of VSC_GLOBAL_TOPK_TILE entries.  Scratch: the search's grow-only per-device buffers (8 bytes per 2048 entries + 16 bytes
 * per selected entry), freed by vsc_search_release_scratch.  Only enqueues on `stream`; no host synchronisation. */
#define VSC_GLOBAL_TOPK_TILE 2048
int vsc_global_topk_f32(const float *scores_dev, const int64_t *rows_dev, const int64_t *ids_dev, int64_t n, int32_t row_stride,
                        int64_t want, int64_t *out_rows_dev, int64_t *out_ids_dev, float *out_scores_dev, int64_t *out_count_dev,
                        void *stream);

/* First hit of every video pair in a best-first hit list -- the grouping of infer/vsc/candidates.py:24-40 under
 * MaxScoreAggregation over the list of infer/vsc/index.py:145-165: in best-first order a video pair's first hit is its maximum.
 * rows_dev / ids_dev [n]: query row and reference row of every hit; q_video_dev [number of query rows] / r_video_dev [number of
 * reference rows]: int32 video index of a row, 0 <= r video < n_r_videos; every rows[p] / ids[p] >= 0 must index its table --
 * the entry has no table lengths and checks nothing: the lists come from the library's own search and selection -- (a hit with a
 * negative row or id belongs to no pair).  The pair key is q_video[rows[p]] * n_r_videos + r_video[ids[p]] in 64
 * bits.  Writes to out_pos_dev [min(n, limit)] the positions p, ascending, of the first hit of every distinct key -- only the first
 * `limit` of them (limit < 0: all) -- and their number to out_count_dev [1] (device): np.unique(key, return_index=True), sort,
 * [:limit].  n < 2^31.  n == 0 or limit == 0 writes count 0 and launches nothing.  Deterministic: an open-addressing table keeps
 * the atomicMin of the positions per key (order-independent), the positions are written through a prefix scan.  Scratch: the
 * search's grow-only buffers (12 bytes per table slot, 2 n rounded up to a power of two slots, + n bytes).  Only enqueues. */
int vsc_pair_first_hits(const int64_t *rows_dev, const int64_t *ids_dev, int64_t n, const int32_t *q_video_dev,
                        const int32_t *r_video_dev, int32_t n_r_videos, int64_t limit, int64_t *out_pos_dev,
                        int64_t *out_count_dev, void *stream);

/* Temporal-network (TN) alignment -- VCSL's `tn` (VSC22-Descriptor-Track-1st/infer/vcsl/vta.py:244-363, with `iou` :80-95),
 * the alignment step of sscd_baseline's localize_and_verify -- over the matrices of vsc_pair_similarity_f32, one wave per pair.
 * sims_dev: fp32 similarities (sims_len floats); pairs_host [n_pairs][3] = {element offset, q_rows, r_rows} (HOST memory):
 * pair p is the row-major [q_rows, r_rows] matrix at sims_dev + offset.  Every element is used as s + bias (fp32 add).
 * Outputs (device): boxes_dev int32 [n_pairs][max_path + 1][4] = {q from, r from, q to, r to} in acceptance order (unused
 * slots 0), counts_dev int32 [n_pairs], maxsim_dev float [n_pairs][max_path + 1] = max of (s + bias) over the half-open box
 * [q from:q to, r from:r to], minus bias (fp32; unused slots 0).
 * Contract (the reference under numpy 2 / networkx 3.4, with one fixed tie rule):
 *   nodes: 0 = source (-1,-1); 1 + q*top + k = (q, k-th best column of row q), top = min(top_k, r_rows), best = descending
 *     biased similarity with ties to the LOWER column (the reference's np.argsort leaves tie order unspecified); sink = N-1.
 *   regular edges (q_i, c) -> (q_j, r): q_i < q_j < q_i + max_step; C2 0 < col_j - col_i < max_step; C3 no column of the
 *     running intermediate set of q_i (targets of its valid edges to earlier q_j) strictly between col_i and col_j; C4
 *     sim_j >= float32(min_sim); weight sim_j; predecessor order (q_i, c) ascending.
 *   sink edges: every node i < N-1 (source included) with q_sink > q_i, col_sink > col_i, both gaps <= max_step, weight 0
 *     (a regular edge keeps its place, its weight becomes 0; new ones follow in node-id order).
 *   longest path: dist(v) = first maximum over predecessors of dist(u) + w in fp32, (0, v) without predecessors or when
 *     negative; the path ends at the first node of maximal dist in networkx's topological order (Kahn by generations,
 *     generation 0 in node-id order, successors in (q_j, k) order, the sink edge last); traceback through stored predecessors.
 *   rounds (at most max_path + 1): zero the path's edges; drop nodes 0 and N-1 (stop if nothing is left); score = fp32 sum
 *     of the biased sims in path order; box = min / max of q and col if score > 0, else zeros; accept if
 *     (double)score / ((dcol + dq) / 2) > min_sim (float64), min(dcol, dq) > min_length and the largest IoU ("+1" integer
 *     areas, float64 division; 0 with no box yet) against the accepted boxes < max_iou.
 *   A pair with an empty side yields no boxes.  Non-finite similarities are outside the contract.
 * Limits: 1 <= top_k <= 16; max_step >= 1; (max_step - 1) * top_k <= 64 (predecessor bits per node); 0 <= max_path < 4096;
 * min_length >= 0; q_rows <= 65536; r_rows <= 2^24.  Scratch: the search path's grow-only per-device buffers (40 bytes per
 * graph node); vsc_search_release_scratch frees them.  Synchronises `stream` once (to upload the pair table). */
int vsc_tn_align_f32(const float *sims_dev, int64_t sims_len, const int64_t *pairs_host, int64_t n_pairs, float bias,
                     int32_t max_step, int32_t top_k, int32_t max_path, double min_sim, int32_t min_length, double max_iou,
                     int32_t *boxes_dev, int32_t *counts_dev, float *maxsim_dev, void *stream);

/* DP and HV temporal alignment -- VCSL's `dp` (with `njit_dp_matrix`, `find_path`, `cut_path`; VSC22-Descriptor-Track-1st/
 * infer/vcsl/vta.py:98-127,153-241) and `hv` (:366-426) -- over the matrices of vsc_pair_similarity_f32, beside TN: one wave per
 * pair, the pair list of a call in as few launches as the scratch cap allows.  A handle API: every call of a handle enqueues on
 * the stream given at create.  sims_dev / sims_len / pairs_host [n_pairs][3] / bias are vsc_tn_align_f32's; every element is used
 * as s + bias (fp32 add).  Outputs (device), TN's layout: boxes_dev int32 [n_pairs][max_boxes][4] = {q from, r from, q to, r to}
 * in acceptance order (unused slots 0); counts_dev int32 [n_pairs] = the number FOUND, which may exceed max_boxes (only the first
 * max_boxes are stored); maxsim_dev float [n_pairs][max_boxes] = max of (s + bias) over the half-open box [q from:q to,
 * r from:r to], minus bias in fp32, -inf when that extent is empty (HV, on a one-cell diagonal); unused slots 0.
 *
 * vsc_align_dp_f32 -- contract (the reference's text run undecorated under numpy 2 scalar rules: everything float32; under
 * numba's typing the two half-weight candidates and the min_sim comparison are float64, which agrees wherever rounding does not
 * decide).  sim = (s + bias) + 1.0f.
 *   matrix: dp = sim, acc = 0, bt = -1.  For i, j >= 1 in row-major dependency order the candidates are {dp[i-1,j-1] + sim[i,j],
 *     dp[i-1,j] + 0.5f * sim[i,j], dp[i,j-1] + 0.5f * sim[i,j]}, each rounded to fp32; the FIRST maximum wins, k its index.  If
 *     sim[i,j] < float32(min_sim): acc[i,j] = acc[prev_k] + 1.  If acc[i,j] <= discontinue: bt[i,j] = k, dp[i,j] = value_k;
 *     otherwise the cell keeps dp = sim, bt = -1 and its acc.
 *   rounds (exactly 100 at most): take the cell of the first maximum of dp in row-major order, stop all rounds if it is -inf;
 *     walk bt back until bt == -1 or until the next cell's dp is -inf (that cell is not appended); path = the walk reversed;
 *     dp[r1:r2+1, c1:c2+1] = -inf over the path's first and last cell; cut_path(path, diagonal_thres): the maximal runs of steps
 *     that keep the row index, and those that keep the column index, covering more than diagonal_thres path cells are
 *     discarded, the ranges [s, e) between consecutive discarded ranges (from 0, up to len(path)) are kept -- a run of one kind
 *     followed at once by one of the other shares a cell with it and gives s > e --; keep the ranges with e - s > min_length;
 *     mean = numpy's float32 np.mean of sim along the sub-path (pairwise sum, one fp32 division by the count); emit
 *     [q0, r0, q1, r1] of the sub-path's ends if mean > float32(ave_sim) and both extents > min_length.
 * vsc_align_hv_f32 -- contract; max_boxes = max_peaks.
 *   s' = s + bias, cells with s' < float32(min_sim) become 0.  A diagonal sigma = r - q is a peak if it holds a cell
 *   >= float32(min_sim) after zeroing; its extent is q in [max(-sigma, 0), min(max(R - sigma, 0), Q)); its score is numpy's
 *   float32 pairwise np.sum of the WHOLE diagonal.  Peaks in descending score, stable (ties in ascending sigma), the first
 *   max_peaks of them, those with score <= 0 skipped; box = the diagonal's whole extent [a, a + sigma, e - 1, e - 1 + sigma];
 *   accepted unless the IoU ("+1" integer areas, float64 division, vsc_tn_align_f32's; 0 with no box yet) against an accepted box
 *   is > iou_thresh.  (The reference holds the accepted corners in float32 arrays: areas above 2^24 cells round there, not here.)
 * A pair with an empty side yields no boxes.  Non-finite similarities are outside the contracts.
 * Limits (refused by name): q_rows, r_rows <= 65536; q_rows * r_rows <= 2^26; 0 <= discontinue <= 254 (acc is kept as a saturating
 * 8-bit count, which is exact for these: acc only feeds `<= discontinue` and `+ 1`); min_length, diagonal_thres >= 0;
 * 1 <= max_boxes, max_peaks <= 4096.  Scratch: two of the search path's grow-only per-device buffers (callers on one device are
 * ordered; vsc_search_release_scratch frees them): 6 bytes per cell + 16 per row + 8 per column (DP), 5 bytes per diagonal (HV), each
 * pair's rounded up to 16, for the pairs of a launch; a launch takes pairs while they fit the handle's cap (default 256 MiB) and always at least one.
 * vsc_align_scratch sets the cap (cap_bytes > 0; 0 keeps it) and reports the launches and the arena bytes of the handle's last
 * call (either pointer may be null).  The entries synchronise the stream once (to upload the pair table). */
typedef struct vsc_align vsc_align;
int vsc_align_create(void *stream, vsc_align **out);   /* every call of the handle enqueues on this stream */
void vsc_align_destroy(vsc_align *h);
int vsc_align_scratch(vsc_align *h, int64_t cap_bytes, int64_t *last_launches, int64_t *scratch_bytes);
int vsc_align_dp_f32(vsc_align *h, const float *sims_dev, int64_t sims_len, const int64_t *pairs_host, int64_t n_pairs, float bias,
                     int32_t discontinue, double min_sim, double ave_sim, int32_t min_length, int32_t diagonal_thres,
                     int32_t max_boxes, int32_t *boxes_dev, int32_t *counts_dev, float *maxsim_dev);
int vsc_align_hv_f32(vsc_align *h, const float *sims_dev, int64_t sims_len, const int64_t *pairs_host, int64_t n_pairs, float bias,
                     double min_sim, double iou_thresh, int32_t max_peaks, int32_t *boxes_dev, int32_t *counts_dev,
                     float *maxsim_dev);

/* Matching-track localisation -- the reference's generate_matching_result (VSC22-Matching-Track-1st/infer/src/utils.py:76-117:
 * threshold, cv2.connectedComponentsWithStats, one sklearn RANSACRegressor fit per component group) -- over the refinement
 * networks' probability maps, one workgroup per (map, threshold) item, all items of a call in one launch.
 * maps_dev: fp32 probabilities (maps_len floats); items_host [n_items][3] = {element offset, h, w} (HOST memory): map i is the
 * row-major [h, w] matrix at maps_dev + offset, x = row = query frame, y = column = reference frame.  thresholds / std_ratios
 * [n_thr] (HOST): item (i, t) is map i at thresholds[t] with std_ratios[t].  Outputs (device), item index i * n_thr + t:
 * out_segments_dev int32 [n_items * n_thr * max_segments][4] = {x first, y first, x last, y last}, out_scores_dev double
 * [n_items * n_thr * max_segments], out_counts_dev int32 [n_items * n_thr] = segments FOUND (uncapped: a count above
 * max_segments means only the first max_segments were stored -- call again wider).
 * Contract (executable: tests/seg_contract.py).  sklearn's float64 lstsq puts points whose exact residual EQUALS the residual
 * threshold at 2 +- 1e-14 and so decides them by rounding noise; here the trial phase is exact integer arithmetic and such
 * points are inliers.  Everything else is sklearn 1.7's loop:
 *   mask = P > threshold in fp32.  8-connected components; more than 10 pixels = large, all other masked pixels are loose.  One
 *     group per large component (its pixels + ALL loose pixels) in raster order of the components' first pixels; without a
 *     large component the single group is the loose pixels.  A group's points are taken in raster order (np.where).
 *   A group with 3 or fewer distinct x is skipped.  Trial loop: n_inliers_best = 1, score_best = -inf, max_trials = 200; trial t
 *     draws the 2-subset that sample_without_replacement(n, 2, random_state=rs) returns on its t-th call, rs = RandomState(2023)
 *     (MT19937, masked rejection): n < 200: rs.permutation(n)[:2]; n >= 200: rs.randint(n), the second redrawn while equal.  The
 *     trial is skipped if its inlier count k is below the best, or equal with R^2 below the best; otherwise it is kept and
 *     max_trials = min(max_trials, ceil(log(1 - 0.99) / log(max(eps, 1 - (k / n)^2)))).
 *   Trial model, dx = x2 - x1 != 0: inlier iff |(y - y1) dx - (y2 - y1)(x - x1)| <= 2 |dx| (integers).  Over the inliers
 *     A = sum of that residual squared, B = k sum y^2 - (sum y)^2 (integers); R^2 = 1 - ((double)A (double)k) / ((double)dx^2
 *     (double)B), every operation rounded on its own; B = 0: R^2 = 1 if A = 0, else 0.
 *   dx = 0: the line is y = c, c = y1 if y1 = y2, else (w1 y1 + w2 y2) / (w1 + w2) in float64 with w = (double)(p * p), the
 *     product in fp32; inlier iff |y - c| <= 2; res = ((double)sum y^2 - (2 c)(double)sum y) + ((double)k c) c; R^2 = 1 -
 *     (res (double)k) / (double)B; B = 0: R^2 = 1 if res = 0, else 0.
 *   Final model: float64 weighted least squares over the best inliers in closed form (weighted means, then sum w (x - xm)^2 and
 *     sum w (x - xm)(y - ym); slope 0 when the former is 0).  Rejected if slope <= 0.  A point is near iff |y - (slope x + icpt)|
 *     < 1; accepted iff more than 5 near points with more than 3 distinct x and more than 3 distinct y.  Segment = first and
 *     last near point in raster order; score = (max(top) - std(top) std_ratio) - |max(1 / slope, slope) - 1| / 10 in float64,
 *     top = the fp32 probabilities of the near points, std the population standard deviation.
 *   The float64 sums of the final model are taken in the kernel's own fixed order: two runs give the same bytes; against another
 *     summation order, decisions closer than ~1e-12 to their boundary may differ (tests/seg_contract.py reports that margin).
 * Limits: h, w <= 224; 1 <= n_thr <= 8.  Non-finite probabilities are outside the contract.  Synchronises `stream` once (to
 * upload the item table).  The item table lives in one per-device scratch slot that the kernel reads until it ends: calls on one
 * device are ordered -- one stream, or streams synchronised around the call (as for the search path's scratch). */
int vsc_match_segments_f32(const float *maps_dev, int64_t maps_len, const int64_t *items_host, int64_t n_items,
                           const float *thresholds, const double *std_ratios, int32_t n_thr, int32_t max_segments,
                           int32_t *out_segments_dev, double *out_scores_dev, int32_t *out_counts_dev, void *stream);

/* Matching-track network inputs -- the reference's best-view choice (VSC22-Matching-Track-1st/infer/src/utils.py:18-73: per query
 * view the mean of its ten largest row maxima, np.argmax over the views) and its padded 3-channel maps
 * (VSC22-Matching-Track-1st/infer/src/dataset.py:103-144: MatchClassifyDataset / MatchRefineDataset) -- built on the device from the
 * matrices of vsc_pair_similarity_f32, so that no similarity matrix and no network input crosses PCIe.
 * sims_dev: fp32 similarities (sims_len floats); items_host [n_items][4] = {element offset, q_rows, r_rows, frames} (HOST memory):
 * item p is the row-major [q_rows, r_rows] matrix s at sims_dev + offset, whose rows are views of `frames` rows each (frames = the
 * query video's frame count).  resolution R: side of the canvas, 1 <= R <= 1024.  with_transpose: 0 or 1.
 * Outputs (device): view_start_dev int32 [n_items] and out_dev float [n_items * (1 + with_transpose)][R][R][3] (channels last:
 * viewed as [.., 3, R, R] it is a channels-last network input).
 *   View: an item with q_rows <= frames has one view, view_start = 0, and is not read.  Otherwise, for view v = rows
 *     [v frames, (v + 1) frames): m_i = fp32 maximum of row i over all r_rows columns (starting from -inf: rows of negative
 *     similarities are legal); a[0 .. c-1] = the c = min(VSC_MATCH_TOP_ROWS, frames) largest m_i in ascending order; score =
 *     fl(S / c) in fp32 (correctly rounded division) with S summed in numpy's pairwise order: c < 8: (((a0 + a1) + a2) + ..);
 *     c = 8, 9, 10: ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)), then + a8, then + a9 -- np.sort(m)[-10:].mean() bit for
 *     bit.  view_start = v frames of the first view whose score is strictly greater than every earlier one (np.argmax).
 *   Canvas: slice p (1 + with_transpose): out[y][x][c] = s[view_start + y][x] for y < min(frames, q_rows, R) and x < min(r_rows, R),
 *     0 elsewhere, the same on the three channels c.  With with_transpose, slice 2 p + 1: out[y][x][c] = s[view_start + x][y] for
 *     y < min(r_rows, R) and x < min(frames, q_rows, R), 0 elsewhere.  EVERY element of out_dev is written.
 * Refused (VSC_ERR_INVALID): frames < 1; an item outside sims_len; a multi-view item (q_rows > frames) with r_rows < 1 or with
 * ragged views (q_rows % frames != 0) -- with whole views the valid height min(frames, R) is known on the host without a
 * synchronisation.  Similarities are finite; NaN is outside the contract (it neither faults nor hangs; the chosen view is
 * unspecified).  The item table travels in kernel arguments (128 items per pair of launches): no scratch, and the entry only
 * enqueues on `stream` -- no host synchronisation. */
#define VSC_MATCH_TOP_ROWS 10
int vsc_match_maps_f32(const float *sims_dev, int64_t sims_len, const int64_t *items_host, int64_t n_items, int32_t resolution,
                       int32_t with_transpose, int32_t *view_start_dev, float *out_dev, void *stream);

/* Query view preprocessing -- the reference's image_process (VSC22-Descriptor-Track-1st/infer/src/image_preprocess.py:252-275,
 * applied to every query video by infer/src/dataset.py:82-88): the two per-video maps its border / split decisions read, and the
 * crop + resize of every view.  The decisions themselves run on the host (src/image_preprocess.py) or, opt-in, in
 * vsc_view_decide_f64 below.  frames_dev: uint8
 * [n][h][w][3] (RGB, row-major) on the device.
 *
 * Variance map, image_preprocess.py:255-256 (np.stack(frames).var(axis=0).sum(-1)), bit-identical to numpy: out_dev float64
 * [h][w]; per channel mean = (frame-order sum, exact) / n, var = (frame-order sum of (x - mean)^2, each product rounded, no FMA)
 * / n, all fp64; out = (var0 + var1) + var2.  Limits: 1 <= n < 2^24, h * w <= 2^28. */
int vsc_frame_var_u8(const uint8_t *frames_dev, int64_t n, int32_t h, int32_t w, double *out_dev, void *stream);

/* Canny edge counts, image_preprocess.py:263-264 (cv2.Canny(frame, low, high) > 0 over the sampled frames): out_dev uint16
 * [h][w] = the number of frames frames_dev[idx_host[j]], j < m, where Canny marks the pixel an edge (idx_host: HOST memory, each
 * in [0, n)).  Contract: OpenCV 4.x's non-IPP Canny for 3-channel 8-bit input with the L1 gradient, restated from its algorithm
 * (not pinned against cv2; tests/canny_cpu.py is the same contract in numpy):
 *   Sobel 3x3 per channel, CV_16S, replicated border: dx = right - left column (1 2 1), dy = bottom - top row (1 2 1);
 *   per pixel the channel with the largest |dx| + |dy| (a tie goes to the lower channel), its dx, dy and m = |dx| + |dy|;
 *   only m > floor(low) enters non-maximum suppression, in fixed point: TG22 = 13573, x = |dx|, y = |dy| << 15,
 *     y < x * TG22: horizontal, kept if m > left && m >= right;  y > x * TG22 + (x << 16): vertical, m > up && m >= down;
 *     else diagonal with s = (dx ^ dy) < 0 ? -1 : 1, kept if m > prev_row[j - s] && m > next_row[j + s];
 *     magnitude outside the image counts as 0;
 *   a kept pixel is strong if m > floor(high), else weak; hysteresis: a weak or strong pixel is an edge exactly when its
 *   8-connected component of weak | strong pixels holds a strong pixel.
 * Hysteresis is union-find connected components in a fixed number of launches (five per chunk of up to 32 frames, no host
 * polling); labels may differ from run to run, the output does not.  Limits: h * w <= 2^25, 0 <= low <= high < 4096, m <= 65535.
 * Scratch: the search path's grow-only per-device buffers (8 bytes per pixel of a chunk). */
int vsc_canny_count_u8(const uint8_t *frames_dev, int64_t n, const int32_t *idx_host, int32_t m, int32_t h, int32_t w, double low,
                       double high, uint16_t *out_dev, void *stream);

/* Crop + bicubic resize of every view, PIL-exact: the reference resizes each view's frames with Resize([S, S], BICUBIC)
 * (infer/extract_query_feats.py:110-128) after image_process cut them (image_preprocess.py:267-271).  boxes_host int32 [k][4] =
 * {y0, y1, x0, x1} (HOST memory, 0 <= y0 < y1 <= h, 0 <= x0 < x1 <= w); out_dev uint8 [k * n][size][size][3]:
 * out[b * n + i] == Image.fromarray(frame_i[y0:y1, x0:x1]).resize((size, size), Image.BICUBIC), bit for bit.  That is Pillow's
 * 8-bit resample: bicubic a = -0.5, support 2 x max(1, in / out); coefficients in fp64 per (in length, out length), normalised,
 * rounded half away from zero to 22 fractional bits; horizontal pass first, then vertical, each clipped to 0..255 -- except, as
 * in Pillow 12's Image.resize, a crop more than 100 times taller than wide that shrinks in height: vertical first; taps clamp to
 * the CROP's edges (not the frame's: crop-then-resize differs from PIL's box= resize of the whole frame).  A whole-frame box is
 * src/dataset.py:vit_transform_u8(size, size).  Coefficient tables are built on the host and cached on the device for the life of
 * the process, never freed (a synchronous upload the first time a (device, length, size) triple is seen; ~21 KiB per length at
 * 1080p, at most ~150 MiB per size even if every length up to 4096 occurs).  Limits: 1 <= size <= 4096; n * h_crop * size and n * size^2 < 2^31.
 * Scratch: the search path's grow-only per-device buffers (n * max crop height * size * 3 bytes). */
int vsc_resize_bicubic_u8(const uint8_t *frames_dev, int64_t n, int32_t h, int32_t w, const int32_t *boxes_host, int32_t k,
                          int32_t size, uint8_t *out_dev, void *stream);

/* sklearn.preprocessing.normalize(x) in place (l2, axis=1; zero rows untouched):
 * infer/extract_query_feats.py:178, infer/vsc/baseline/score_normalization.py:84-88. */
int vsc_l2_normalize_f32(float *x_dev, int64_t n, int32_t d, void *stream);

/* Score normalisation on the device: what infer/vsc/baseline/score_normalization.py does per set of descriptors -- the
 * low-variance dimension (:74-76; infer/src/utils.py:2-5), np.delete of that column and the row normalisation (:84-88), the bias
 * -beta * mean of the nk best noise scores (:95-105) with the video-score gate (:141-150), and the appended column -- with the
 * BITS of that numpy chain (executable form of the contract: tests/score_norm_contract.py).  The three entries take a handle
 * that holds the caller's stream (vsc_score_norm_create; as vsc_segment_metric and vsc_pca_fit bind theirs): they only enqueue on it
 * and never synchronise with the host; the handle owns no device memory, a null handle is refused; operands are float32 rows with a row stride in elements, stride >= width.
 *
 * vsc_column_var_f32: var_dev[c] = x.var(axis=0)[c] as numpy computes it for a C-contiguous [n, d] float32 array.  Per column one
 * chain over the rows in ascending order:  s = ((x[0] + x[1]) + x[2]) + ... in fp32;  mean = (float)((double)s / (double)n);
 * acc = sum over the rows, in that order, of fl(fl(x - mean) * fl(x - mean)), the subtraction, the product and the sum each rounded
 * on their own (no fused multiply-add);  var = (float)((double)acc / (double)n).  The low-variance dimension is the host's
 * np.argmin of var_dev.  One workgroup per 64 columns, rows staged through LDS in tiles of VSC_COLUMN_VAR_TILE; rows past n and
 * columns past d are never read.  Refused: n < 1, d < 1, ld < d, a null pointer.
 *
 * vsc_score_norm_rows_f32: out = concatenate([normalize(delete(x, drop, axis=1)), last], axis=1).  drop in [0, d) or -1 (no column
 * dropped); normalize 0 or 1; append 0 (no column), 1 (the constant 1.0f) or 2 (last_dev[row]); the output has
 * d - (drop >= 0) + (append != 0) columns.  normalize = 1 is vsc_l2_normalize_f32 on the narrowed row: lane l of the row's wave sums
 * the squares of the narrowed row's columns l, l + 64, ... as fmaf(x, x, ss), the lanes are added by the xor butterfly 32 ... 1,
 * nrm = sqrtf(ss), and the row becomes x / nrm -- or stays exactly as it was when nrm == 0 (a zero row, and a row whose squares
 * underflow).  out_dev must not overlap x_dev (refused: the kernel is no in-place shift).  n == 0 launches nothing.  Refused: n < 0
 * or n >= 2^31, drop outside [-1, d), other values of normalize / append, a stride below its width, a null operand that is needed.
 *
 * vsc_score_norm_bias_f32: bias_dev[q] = fl32(neg_beta * mean(topk[q, 0:nk])) with numpy's row sum -- nk < 8: left to right from
 * the first element; 8 <= nk <= 128: eight accumulators r[j] = a[j], r[j] += a[i + j] for i = 8, 16, ... < nk - nk % 8, then
 * ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the remaining nk % 8 elements left to right -- and
 * mean = (float)((double)sum / (double)nk); neg_beta is the caller's (float)(-beta).  gate_dev: uint8 [nq] or NULL; a non-zero
 * entry makes the row's bias exactly -100.0f (a video below the score threshold).  nq == 0 launches nothing.  Refused: nk outside
 * [1, 128] (beyond it numpy's sum recurses), ldk < nk, nq < 0 or nq >= 2^31, a null operand. */
#define VSC_COLUMN_VAR_TILE 64
typedef struct vsc_score_norm vsc_score_norm;
int vsc_score_norm_create(void *stream, vsc_score_norm **out);   /* every call of the handle enqueues on this stream */
void vsc_score_norm_destroy(vsc_score_norm *h);
int vsc_column_var_f32(vsc_score_norm *h, const float *x_dev, int64_t n, int32_t d, int64_t ld, float *var_dev);
int vsc_score_norm_rows_f32(vsc_score_norm *h, const float *x_dev, int64_t n, int32_t d, int64_t ldx, int32_t drop, int32_t normalize,
                            int32_t append, const float *last_dev, float *out_dev, int64_t ldo);
int vsc_score_norm_bias_f32(vsc_score_norm *h, const float *topk_dev, int64_t nq, int64_t ldk, int32_t nk, float neg_beta,
                            const uint8_t *gate_dev, float *bias_dev);

/* PCA fit, the part that grows with the number of rows -- the reference fits its PCA inside the reference-side chain
 * (infer/concat_pca_sn.py:42-54: PCA(n_components=512, random_state=2023).fit(train_features) on the concatenated, per-model
 * normalised descriptors of every training reference).  The handle accumulates the RAW MOMENTS of fp32 rows in fp64 on the matrix
 * pipe (v_mfma_f64_16x16x4_f64):  sum[d] = sum_rows x,  S2[d, d] = sum_rows x x^T.  Moments are additive: blocks of rows may arrive
 * in any number of calls (and moments of several handles / ranks may be added).  The d x d eigenproblem is the caller's
 * (vsc_hip/pca_fit.py: numpy.linalg.eigh in float64; contract in tests/pca_contract.py).
 * Accuracy: every element is an fp64 sum of exact fp32 x fp32 products, |S2 - exact| <= n 2^-52 (|X|^T |X|) element-wise.  Rows are
 * split over workgroups by (n, d) alone and partial sums are added in a fixed order, no atomics: the same sequence of calls gives
 * the same bits.  16 <= d <= 4096.  One stream at a time per handle.  Scratch for the partials (< 512 MiB) grows with the largest
 * update seen and is freed with the handle. */
typedef struct vsc_pca_fit vsc_pca_fit;
/* concat_pca_sn.py:42-54 (the PCA object before fit); needs a device */
int vsc_pca_fit_create(int32_t d, vsc_pca_fit **out);
/* concat_pca_sn.py:42-54 (fit's pass over the data): adds the n rows x_dev[i * ld .. i * ld + d), ld >= d, to the moments.  May be
 * called any number of times; n = 0 is a no-op. */
int vsc_pca_fit_update_f32(vsc_pca_fit *f, const float *x_dev, int64_t n, int64_t ld, void *stream);
/* concat_pca_sn.py:42-54 (what fit has seen): sum_dev [d], s2_dev [d, d] -- the full symmetric S2, lower triangle mirrored from the
 * upper, s2 == s2^T bit for bit -- and the row count in *n_out (HOST memory).  Any of the three may be null. */
int vsc_pca_fit_moments_f64(vsc_pca_fit *f, double *sum_dev, double *s2_dev, int64_t *n_out, void *stream);
/* concat_pca_sn.py:42-54 (fit's mean_ and the covariance its components diagonalise): mean_dev [d] = sum / n, cov_dev [d, d] =
 * (S2 - n mu mu^T) / (n - 1) in fp64, every operation rounded on its own, symmetric bit for bit; fewer than 2 rows are refused. */
int vsc_pca_fit_covariance_f64(vsc_pca_fit *f, double *mean_dev, double *cov_dev, void *stream);
void vsc_pca_fit_destroy(vsc_pca_fit *f);

/* Matching-track segment AP -- the reference's match_metric (VSC22-Matching-Track-1st/infer/vsc/metrics.py:120-383: Intervals,
 * Match.overlaps, VideoPair.add_prediction and the accumulation loop), the number sscd_baseline.py:224-225 logs as "Matching track
 * metric".  Two kernels; the divisions, square roots and the AP sum stay on the host (vsc_hip/segment_metric.py), so the device
 * arithmetic is fp64 add, subtract, compare, min / max and one multiply, every operation rounded on its own -- bit-equality with the
 * reference rests on IEEE arithmetic alone.  Executable contract: tests/segment_metric_contract.py.
 *
 * The handle owns the scratch and is bound to a stream at creation: every call of the handle enqueues on that stream and nothing
 * else (no host synchronisation, no table in host memory; growing the scratch frees the smaller buffer, which waits for the
 * device, as vsc_pca_fit_update_f32 does).  One host thread at a time per handle.  The results are pure functions of the operands.
 *
 * vsc_segment_metric_deltas_f64, one wave per video pair.  pred_boxes_dev [n_preds][4] = {q_start, q_end, r_start, r_end} in RANK
 * order (rank = position in the stable descending sort by score); pred_ptr_dev [n_pairs + 1] / pred_rank_dev [n_preds]: CSR listing
 * each pair's ranks in ascending order; gt_boxes_dev [n_gts][4] grouped by pair in file order, gt_ptr_dev [n_pairs + 1].  Outputs:
 * deltas_dev [n_preds][4] = {dI_q, dI_r, dT_q, dT_r} written at the prediction's rank, gt_len_dev [n_pairs][2].  Per pair, with its
 * predictions taken in rank order:
 *   Considered ground truths: a ground truth becomes considered once
 *     fabs(max(min(qe, qe') - max(qs, qs'), 0) * max(min(re, re') - max(rs, rs'), 0)) > 0.0
 *     holds against any prediction so far -- that fp64 product as written (an underflowing product is "no overlap" in the reference
 *     too).  The flag never clears.
 *   Merged set of a list of intervals: its connected components under start <= current_end (touching intervals merge), each from
 *     its least start to its greatest end.
 *   len(S) = (((0.0 + (e0 - s0)) + (e1 - s1)) + ...) over the components in ascending start order; order and association are fixed.
 *   Per axis: U = merged set of the predictions so far, G = merged set of the considered ground truths, W = merged set of U's and
 *     G's components together; T = len(U); I = (T + len(G)) - len(W); dI = I - I_prev, dT = T - T_prev, both starting at 0.0.
 *   gt_len[p][axis] = len(merged set of ALL the pair's ground truths).
 * Lists longer than a wave go in chunks of 64: no limit on a pair's size below the global one, n_preds, n_gts, n_pairs < 2^31.
 * Scratch: 128 (n_preds + n_gts) + 4 n_gts bytes, owned by the handle, initialised by every call.  Boxes are finite with
 * end >= start (the host refuses others; on the device they neither fault nor hang, the result is unspecified); tables that point
 * outside the operands leave their pair unwritten.  n_preds == 0 (or n_pairs == 0) launches nothing and writes nothing.
 *
 * vsc_segment_metric_scan_f64, one workgroup: out_dev[e][c] = ((0.0 + rows[0][c]) + rows[1][c]) + ... + rows[ends[e]][c] for
 * rows_dev [n][cols] fp64, 1 <= cols <= 8, ends_dev [n_ends] int64 ascending (repeats allowed) in [0, n): strictly left to right,
 * no tree, no atomics, no reassociation (np.cumsum(rows, axis=0)[ends]).  Serves the running {I_q, I_r, T_q, T_r} at the end of
 * every tie group of scores, and the two ground-truth totals (rows = gt_len of the pairs that have ground truth, in order of first
 * appearance in the ground-truth file: the insertion order of the reference's dict).  n == 0 or n_ends == 0 launches nothing.
 *
 * Refused (VSC_ERR_INVALID): a null handle, negative counts, counts of 2^31 or more, cols outside 1 .. 8, a null operand of a call
 * that launches. */
typedef struct vsc_segment_metric vsc_segment_metric;
/* metrics.py:309-336 (the state match_metric sets up); every call of the handle enqueues on this stream */
int vsc_segment_metric_create(void *stream, vsc_segment_metric **out);
void vsc_segment_metric_destroy(vsc_segment_metric *m);
/* metrics.py:243-306 (VideoPair.add_prediction for every prediction of every pair) and :262-263 (total_gt_length) */
int vsc_segment_metric_deltas_f64(vsc_segment_metric *m, const double *pred_boxes_dev, const int64_t *pred_ptr_dev,
                                  const int64_t *pred_rank_dev, int64_t n_preds, const double *gt_boxes_dev,
                                  const int64_t *gt_ptr_dev, int64_t n_gts, int64_t n_pairs, double *deltas_dev, double *gt_len_dev);
/* metrics.py:331-335 and :357-360 (the running sums, in dict order and in score order) */
int vsc_segment_metric_scan_f64(vsc_segment_metric *m, const double *rows_dev, int64_t n, int32_t cols,
                                const int64_t *ends_dev, int64_t n_ends, double *out_dev);

/* Descriptor-track micro-AP -- the reference's average_precision (VSC22-Descriptor-Track-1st/infer/vsc/metrics.py:423-494), the
 * number it logs as "Candidate uAP" -- in two entries (executable contract: tests/uap_contract.py).  A pair is a 64-bit key
 * query_index << ref_bits | ref_index of the indices the caller interned (ref_bits = 32 in general); every key is below
 * 2^key_bits, and the key sorts skip the digit passes above that.  Both entries take a handle, which holds the stream it was made
 * with and owns no device memory, and only enqueue on that stream; scratch is the search's grow-only per-device buffers (callers
 * on one device are ordered; vsc_search_release_scratch frees it): about 48 n + 16 g bytes.
 * n, g < 2^31.  n == 0 launches nothing, writes nothing and returns 0.  The outputs are a pure function of the inputs: integer
 * atomics only count, every position is a scan result, every floating-point sum has a fixed association.
 *
 * vsc_uap_rank_f64: scores_dev f64 [n], pred_keys_dev u64 [n], gt_keys_dev u64 [g] in any order.
 *   perm_dev i64 [n]          the stable descending order of the scores: perm[i] = input position of rank i; equal scores keep
 *                             their input order and -0.0 equals +0.0 (sorted(reverse=True), argsort(-s, kind="mergesort"))
 *   scores_ranked_dev f64 [n] scores[perm] (bits kept), correct_dev u8 [n]: 1 where pred_keys[perm[i]] is a ground-truth key
 *   status_dev i64 [4]        {non-finite scores, adjacent equal keys in the sorted predictions, the same in the sorted ground
 *                             truth, correct rows}; the first three are the reference's refusals ("Scores must be finite.",
 *                             "Duplicates detected in ..."), which stay the caller's to raise: the call completes either way (a NaN
 *                             orders by its bit pattern).
 *   Sorts are stable 8-bit LSD radix sorts over tiles of VSC_UAP_TILE entries (the scheme of vsc_global_topk_f32 on 64-bit keys).
 *
 * vsc_uap_curve_f64: scores_ranked_dev / correct_dev [n] as written above, n_gt >= 1 the number of ground-truth pairs.  With
 *   cum_i the inclusive count of correct rows and a tie group a maximal run of == scores ending at row last_j with tps_j = cum:
 *   curve_dev f64 [3][n]      at the k-th correct row i (k = cum_i - 1): [0][k] = cum_i / (i + 1), [1][k] = cum_i / n_gt,
 *                             [2][k] = score_i; the columns from n_pos on are not touched
 *   counts_dev i64 [2]        {n_pos, n_groups}
 *   sums_dev f64 [2]          [0] = np.sum([t_G, ..., t_1]), t_j = (R_j - R_{j-1}) P_j, R_j = tps_j / n_pos (R_0 = 0),
 *                             P_j = tps_j / (last_j + 1) -- the order in which sklearn's average_precision_score sums its
 *                             reversed curve; all t_j = 0 when n_pos = 0.  [1] = np.sum(cum_i / (i + 1) * correct_i) over the n
 *                             rows.  np.sum of a float64 vector: consecutive chunks of 8192 elements (numpy's buffer size) are
 *                             summed pairwise and the chunks' sums added one after the other, starting from 0.0.  Pairwise:
 *                             below 8 elements a running sum from 0.0; up to 128 eight interleaved accumulators combined
 *                             ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) and the remainder added one by one; above, split at
 *                             n2 = n / 2, n2 -= n2 % 8.  The divisions are IEEE fp64 divisions, nothing is contracted.
 *   What the reference does next stays with the caller, in host floats: ap = max(0.0, sums[0]) * (n_pos / n_gt) (0.0 when
 *   n_pos = 0), simple_ap = sums[1] / n_gt. */
#define VSC_UAP_TILE 2048
typedef struct vsc_uap vsc_uap;
int vsc_uap_create(void *stream, vsc_uap **out);   /* every call of the handle enqueues on this stream */
void vsc_uap_destroy(vsc_uap *h);
int vsc_uap_rank_f64(vsc_uap *h, const double *scores_dev, const uint64_t *pred_keys_dev, int64_t n, const uint64_t *gt_keys_dev,
                     int64_t g, int32_t key_bits, int64_t *perm_dev, double *scores_ranked_dev, uint8_t *correct_dev,
                     int64_t *status_dev);
int vsc_uap_curve_f64(vsc_uap *h, const double *scores_ranked_dev, const uint8_t *correct_dev, int64_t n, int64_t n_gt,
                      double *sums_dev, int64_t *counts_dev, double *curve_dev);

/* Near-duplicate frame filter of the query ensemble -- the reference's greedy pass over a video's frame x frame similarities
 * (VSC22-Descriptor-Track-1st/infer/extract_query_feats.py:190-199; here src/query_postprocess.py: greedy_select) -- over the
 * matrices of vsc_pair_similarity_f32, one workgroup per video, all videos of a call in one launch per VSC_FRAME_FILTER_CHUNK
 * items.  Executable contract: tests/frame_filter_contract.py.
 * sims_dev: fp32 similarities (sims_len floats); items_host [n_items][2] = {element offset, rows} (HOST memory): item p is the
 * row-major [rows, rows] matrix s at sims_dev + offset (any element offset; matrices may be asymmetric).  threshold: float32.
 * Item p owns the slice [P, P + rows) of kept_dev / means_dev / order_dev, P = the sum of the rows of the items before it.
 *   v[i][j] = s[i][j] for i != j, v[i][i] = s[i][i] - 1.0f (fp32).
 *   mean[j] = (((v[0][j] + v[1][j]) + v[2][j]) + ...) / (float)rows: one fp32 add chain per column over the rows in ascending
 *     order that starts from v[0][j] itself, then one correctly rounded fp32 division -- sim.mean(0) of numpy for float32, bit
 *     for bit (rows < 2^24; numpy starts from +0.0, which differs only on a column of nothing but -0.0, and v[j][j] is never -0.0).
 *   Visit order: mean descending; EQUAL means are visited in DESCENDING index -- mean.argsort(kind="stable")[::-1].  -0.0 equals
 *     +0.0.  The host path's argsort() is numpy's unstable sort and leaves the order of equal means to the numpy build: the
 *     device equals the host path wherever a video's means are pairwise distinct, and this contract everywhere.
 *   Greedy pass: removed = {}; for i in visit order, unless i is removed: every j with v[i][j] > threshold (ROW i, fp32 compare,
 *     j = i included: it matters only for thresholds below about 0) becomes removed.  Kept = the rows not removed, ascending.
 * Outputs (device): kept_dev int32: the first counts_dev[p] entries of the slice = the kept rows ascending, the rest -1;
 * counts_dev int32 [n_items]; means_dev float (or NULL): mean[j]; order_dev int32 (or NULL): the visit order.  rows == 0 gives
 * count 0 and touches nothing else; n_items == 0 launches nothing.  No atomics: the outputs are a pure function of the inputs.
 * Refused (VSC_ERR_INVALID) before anything is launched: a null handle, rows above VSC_FRAME_FILTER_MAX_ROWS, an item that runs
 * past sims_len, negative sizes, 2^31 or more rows in all, a null pointer that is needed, a non-finite threshold.  NaN
 * similarities are outside the contract (they neither fault nor hang; the result is unspecified).
 * Scratch: a video's adjacency bit matrix, 8 rows ceil(rows / 64) bytes, sits in LDS while 8 rows (1 + ceil(rows / 64)) <=
 * VSC_FRAME_FILTER_LDS_BYTES (rows <= 1088); larger videos take that many bytes each, rounded up to 128, from the search path's
 * grow-only per-device buffers (callers on one device are ordered; vsc_search_release_scratch frees them).  The entry takes a
 * handle that holds the caller's stream (as vsc_score_norm and vsc_uap do) and only enqueues on it: the item table travels in
 * kernel arguments, nothing is uploaded and the host never waits. */
#define VSC_FRAME_FILTER_MAX_ROWS 4096
#define VSC_FRAME_FILTER_CHUNK 128
#define VSC_FRAME_FILTER_LDS_BYTES (160 * 1024 - 1024)
typedef struct vsc_frame_filter vsc_frame_filter;
int vsc_frame_filter_create(void *stream, vsc_frame_filter **out);   /* every call of the handle enqueues on this stream */
void vsc_frame_filter_destroy(vsc_frame_filter *h);
int vsc_frame_filter_f32(vsc_frame_filter *h, const float *sims_dev, int64_t sims_len, const int64_t *items_host, int64_t n_items,
                         float threshold, int32_t *kept_dev, int32_t *counts_dev, float *means_dev, int32_t *order_dev);

/* View decisions of the query preprocessing -- the reference's remove_edges, split_imgs and the recursive clean_imgs
 * (VSC22-Descriptor-Track-1st/infer/src/image_preprocess.py; here src/image_preprocess.py: decide_views and the _borders, _trim,
 * _static_side, _bands, _line_cuts, _split and _clean it calls) -- on the two maps where vsc_frame_var_u8 and vsc_canny_count_u8
 * wrote them, one workgroup per video, all videos of a call in one launch per VSC_VIEW_DECIDE_CHUNK items.  Executable contract:
 * tests/view_decide_contract.py.
 * var_dev: float64 variances (var_len doubles); count_dev: uint16 edge counts (count_len values); items_host [n_items][6] =
 * {element offset of the item's dense [h][w] variance map, element offset of its count map, h, w, m, n} (HOST memory; any element
 * offsets): m = the number of Canny samples behind the counts (counts above m are outside the contract: no fault, result
 * unspecified), n = the video's frames.
 * Outputs (device): boxes_dev int32 [n_items][max_views][4] = {y0, y1, x0, x1} of the views in the reference's order, the rest -1;
 * counts_dev int32 [n_items]; status_dev int32 [n_items]: 0 decided; 1 the item needs more than max_views views or more than
 * VSC_VIEW_DECIDE_STACK pending regions: count 0, every box -1, and the caller decides it on the host.  An unchanged video is one box
 * equal to the whole frame.  n < 5 gives the whole frame without reading the maps.  trace_dev (or NULL): float64 [n_items][8], for
 * the whole-frame _borders call np.quantile(avg, 0.95), avg.mean(), the threshold, edges.mean(), var.mean(1)[h / 2],
 * var.mean(0)[w / 2], edges.mean(1)[h / 2], edges.mean(0)[w / 2] (float32 values widened); an item with n < 5 leaves its row alone.
 * Arithmetic: the host path's, which is numpy's (2.2), bit for bit -- avg = count / m in fp64;
 *   a.mean(1): numpy's pairwise sum per row (under 8 elements a chain from 0.0; up to 128 eight strided accumulators combined
 *     ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the remainder in order; above that split at n / 2 rounded down to a multiple of 8),
 *     then one division;  a.mean(0): one add chain per column in row order from 0.0, then one division -- a region one column
 *     wide is summed pairwise down the column;  a.mean() of a region: its row-major flattening in chunks of 8192, pairwise inside,
 *     the chunk sums chained from 0.0;  np.quantile(avg, 0.95): pos = (N - 1) * 0.95, lo = floor(pos), t = pos - lo, A and B the
 *     order statistics lo and min(lo + 1, N - 1) (from the (m + 1)-bin histogram), A + (B - A) t below t = 0.5, else
 *     B - (B - A)(1 - t);  np.median: the middle order statistic, or (a + b) / 2 of the two middle ones;  the edge map is 0/1
 *     float32: its sums are integer counts, its means float32(count) / float32(size);  float32 too: 0.125 + edge_p.mean(),
 *     0.45 + edges.mean(), edge_p.mean() < 0.0225 (a float32 pairwise sum), edge_at > 0.65;  round((i - first) * 0.3): the fp64
 *     product rounded half to even.  No float atomics: the outputs are a pure function of the inputs.
 * Refused (VSC_ERR_INVALID) before anything is launched -- a bad item after a good one launches nothing: a null handle, h or w
 * outside 1..VSC_VIEW_DECIDE_MAX_SIDE, m outside 1..VSC_VIEW_DECIDE_MAX_SAMPLES, max_views outside 1..VSC_VIEW_DECIDE_MAX_VIEWS,
 * negative n, a map that runs past var_len / count_len, a null pointer that is needed.  NaN variances are outside the contract.
 * No scratch: the four profiles and a work array take 32 max(h, w) bytes of LDS.  The entry takes a handle that holds the caller's
 * stream and only enqueues on it: the item table travels in kernel arguments, nothing is uploaded and the host never waits. */
#define VSC_VIEW_DECIDE_MAX_SIDE 4096
#define VSC_VIEW_DECIDE_MAX_SAMPLES 255
#define VSC_VIEW_DECIDE_MAX_VIEWS 64
#define VSC_VIEW_DECIDE_STACK 64
#define VSC_VIEW_DECIDE_CHUNK 64
typedef struct vsc_view_decide vsc_view_decide;
int vsc_view_decide_create(void *stream, vsc_view_decide **out);   /* every call of the handle enqueues on this stream */
void vsc_view_decide_destroy(vsc_view_decide *h);
int vsc_view_decide_f64(vsc_view_decide *h, const double *var_dev, int64_t var_len, const uint16_t *count_dev, int64_t count_len,
                        const int64_t *items_host, int64_t n_items, int32_t max_views, int32_t *boxes_dev, int32_t *counts_dev,
                        int32_t *status_dev, double *trace_dev);

/* Every model input of a video from its uploaded frames, in one call: what src/dataset.py's vit_transform_u8 and
 * clip_transform_u8 do per frame with Pillow in the loader workers.  Executable contract: tests/frame_inputs_contract.py.
 * frames_dev: uint8 [n][h][w][3].  targets_host int32 [n_targets][10] (HOST memory), a row =
 * {y0, y1, x0, x1, out_h, out_w, top, left, crop_h, crop_w}; outs_host [n_targets] (HOST memory): device pointers, target t
 * writes uint8 [n][crop_h][crop_w][3], packed, to outs_host[t]:
 *   out[i] == np.asarray(Image.fromarray(frame_i[y0:y1, x0:x1]).resize((out_w, out_h), Image.BICUBIC))[top:top + crop_h,
 *   left:left + crop_w], bit for bit.  The resample is the one stated at vsc_resize_bicubic_u8 (same coefficient tables, same
 *   cache): taps clamp to the BOX's edges; horizontal pass first, its result rounded and clipped to uint8 as Pillow's intermediate
 *   image is, then the vertical pass -- except a box more than 100 times taller than wide with out_h below its height: vertical
 *   first; an axis whose length does not change passes through its identity coefficients.  Only the window is computed.
 * One fused launch per target, one workgroup per (frame, band of output rows, tile of 64 output columns): the band's horizontally
 * resampled rows stay in LDS, beside the tile's rows of the horizontal coefficient table, the band's rows of the vertical one and
 * the staged source rows.  A target for which not even one output row of a tile fits VSC_FRAME_INPUTS_LDS_BYTES that way (its
 * vertical support x 192 bytes + 64 x (2 + horizontal taps) x 4 bytes + one staged source row: downscales by some hundreds) and
 * the vertical-first shape run as two launches per chunk of frames over the search path's grow-only scratch (at most 256 MiB, or
 * one frame's first pass if that is larger; callers on one device are ordered).  The same bytes either way.  No limit on n.
 * Refused (VSC_ERR_INVALID) before anything is launched, with nothing written -- a bad target after a good one launches nothing:
 * a null handle, a box outside the frame or empty, out_h or out_w outside 1..VSC_FRAME_INPUTS_MAX_SIDE, a window outside
 * out_h x out_w or of negative size, a null output for a non-empty target, n below 0, a null pointer that is needed.  n == 0 or
 * n_targets == 0 launches nothing; a target with crop_h == 0 or crop_w == 0 writes nothing.  No alignment is required of
 * frames_dev or the outputs (dword-aligned outputs whose crop_w * 3 is a multiple of 4 take the fastest store path).
 * The entry takes a handle that holds the caller's stream and only enqueues on it, with one exception it shares with
 * vsc_resize_bicubic_u8: the first time a (device, length, size) triple is seen its coefficient table is built on the host and
 * uploaded with a synchronous copy; the table is then kept for the life of the process. */
#define VSC_FRAME_INPUTS_MAX_SIDE 4096
#define VSC_FRAME_INPUTS_LDS_BYTES (160 * 1024)
typedef struct vsc_frame_inputs vsc_frame_inputs;
int vsc_frame_inputs_create(void *stream, vsc_frame_inputs **out);   /* every call of the handle enqueues on this stream */
void vsc_frame_inputs_destroy(vsc_frame_inputs *h);
int vsc_frame_inputs_u8(vsc_frame_inputs *h, const uint8_t *frames_dev, int64_t n, int32_t fh, int32_t fw, const int32_t *targets_host,
                        int32_t n_targets, uint8_t *const *outs_host);

/* Baseline JPEG frames to uint8 [H][W][3] on the device, any number of frames of any sizes in one call: what
 * np.asarray(Image.open(f).convert("RGB")) does per frame in the loader workers (src/dataset.py), bit for bit (Pillow 12 on
 * libjpeg-turbo 3).  Executable contract: tests/jpeg_decode_contract.py.  The caller parses the headers (vsc_hip/jpeg.py does, and
 * refuses what this entry does not decode: anything but one sequential 8-bit Huffman scan of one or three components in one of the
 * four sampling classes) and passes
 *   bytes_dev    uint8 [bytes_len]: the files' bytes, or at least their entropy-coded segments;
 *   frames_host  int64 [n_frames][VSC_JPEG_FRAME_ROW] (HOST memory), a row = {segment offset in bytes_dev, segment length (from
 *                behind the SOS header to the marker that ends the scan), height, width, sampling class (0 one component, 1 4:4:4,
 *                2 4:2:2 = h2v1, 3 4:2:0 = h2v2), restart interval in MCUs (0: none), table set, output byte offset in out_dev,
 *                component word (byte c = quantisation table | DC Huffman table << 2 | AC Huffman table << 3 of component c), 0};
 *   tables_host  uint8 [n_table_sets][VSC_JPEG_TABLE_SET_BYTES] (HOST memory), a set = uint16 quant[4][64] little endian in the
 *                file's zigzag order, uint8 bits[4][16] and uint8 vals[4][256] as in DHT for the tables DC0, DC1, AC0, AC1, one byte
 *                whose bit t says quantisation table t is present, one byte whose bit (2 * class + id) says that Huffman table is,
 *                six zero bytes.  Sets are keyed by content: the lookup tables of a set are built on the host the first time the
 *                handle sees it; every call uploads its sets and its frame table with one copy.
 * Frame i is written packed at out_dev + its output offset; status_dev int32 [n_frames] gets 0 or the VSC_JPEG_STATUS_* of the
 * first fault of its scan.  The decode path: sequential Huffman scan (restart: byte-align, RSTn in sequence, DC predictors to 0),
 * dequantisation, jpeg_idct_islow (13-bit constants, PASS1_BITS 2), libjpeg's range-limit table read through its 10-bit mask,
 * "fancy" triangle upsampling of subsampled chroma (edges replicated at the real down-sampled width and height = ceil; rounding
 * +1 / +2 before >> 2 in h2v1, +8 / +7 before >> 4 in h2v2; plain replication when the down-sampled width is 2 or less), the
 * 16-bit fixed-point YCbCr -> RGB; one component is replicated to three channels.
 * Two launches per chunk of frames: one wave per frame decodes the scan and runs the IDCT into uint8 planes in the handle's
 * scratch (grow-only, at most the cap of vsc_jpeg_decode_scratch per chunk -- 1 GiB unless set -- or one frame's planes if that is
 * more); one workgroup per (frame, 16 rows, 64 columns) upsamples, converts and stores dwords.  No limit on n_frames (below 2^31).
 * A frame whose scan is damaged (a code in no table, a run past coefficient 63, a missing or wrong RSTn, no bytes left) stops
 * with its status set; its pixels are unspecified, nothing outside its own planes and output is written and no byte outside its
 * segment is read.  Refused (VSC_ERR_INVALID) before anything is launched, with nothing written: a null handle or needed pointer,
 * a segment or an output outside bytes_len / out_len, a side outside 1..VSC_JPEG_MAX_SIDE, an unknown sampling class, a table set
 * index outside n_table_sets, a component that uses a table its set does not hold, Huffman code lengths that describe no prefix
 * code.  n_frames == 0 launches nothing.  No alignment is required of bytes_dev, out_dev or the offsets.
 * The handle holds the caller's stream and only enqueues on it; it owns the scratch and the uploaded tables, so calls of one
 * handle are ordered by its stream, and growing either buffer frees the old one (which waits for the device, once per size).
 * vsc_jpeg_decode_scratch: cap_bytes > 0 sets the cap of later calls; last_chunks / scratch_bytes (either may be null) receive the
 * number of chunks of the handle's last call and the size of its plane scratch. */
#define VSC_JPEG_FRAME_ROW 10
#define VSC_JPEG_TABLE_SET_BYTES 1608
#define VSC_JPEG_MAX_SIDE 16384
#define VSC_JPEG_STATUS_DATA 1     /* the scan ran out of bytes */
#define VSC_JPEG_STATUS_CODE 2     /* a code that is in no table */
#define VSC_JPEG_STATUS_RUN 3      /* a zero run past coefficient 63 */
#define VSC_JPEG_STATUS_RESTART 4  /* a missing or wrong RSTn */
typedef struct vsc_jpeg_decode vsc_jpeg_decode;
int vsc_jpeg_decode_create(void *stream, vsc_jpeg_decode **out);   /* every call of the handle enqueues on this stream */
void vsc_jpeg_decode_destroy(vsc_jpeg_decode *h);
int vsc_jpeg_decode_scratch(vsc_jpeg_decode *h, int64_t cap_bytes, int64_t *last_chunks, int64_t *scratch_bytes);
int vsc_jpeg_decode_u8(vsc_jpeg_decode *h, const uint8_t *bytes_dev, int64_t bytes_len, const int64_t *frames_host, int64_t n_frames,
                       const uint8_t *tables_host, int32_t n_table_sets, uint8_t *out_dev, int64_t out_len, int32_t *status_dev);

/* The same decode in parallel inside a frame (csrc/jpeg_split.hip; executable contract: tests/jpeg_split_contract.py): the bytes
 * of out_dev and the status of every frame are those of vsc_jpeg_decode_u8, bit for bit.  The unit of work is the item, a run of
 * consecutive blocks of one frame with a known start state (bit position in the segment, first block in scan order, number of
 * blocks, DC predictors), one wave each; vsc_jpeg_decode_u8 is "one item per frame from bit 0".
 * vsc_jpeg_decode_split sets how frames are cut: mode bit 1 (value 1) by restart markers, bit 2 (value 2) by self-synchronising
 * sub-streams, 0 not at all; sub_bytes (a multiple of 4, >= 32; default 1024) the raw bytes of a sub-stream; rounds (1 .. 128;
 * default 2) the verification rounds; item_bytes (default 1024) the entropy bytes consecutive restart intervals are grouped up
 * to.  0 keeps sub_bytes, rounds or item_bytes as they are.  A new handle has mode 3.
 * vsc_jpeg_decode_split_u8 takes vsc_jpeg_decode_u8's operands plus a CSR of restart-marker offsets in HOST memory:
 * restart_ptr_host int64 [n_frames + 1] (null: no frame has any), restart_off_host int32 [ptr[n_frames]], row i = the offsets in
 * frame i's segment of its FF D0..D7, ascending.  Every row is checked before anything is launched (VSC_ERR_INVALID: an offset
 * outside [0, segment length - 2] or less than two bytes behind its predecessor).  A frame with a restart interval Ri is cut at
 * its markers only if its row holds ceil(MCUs / Ri) - 1 offsets; any other such frame is one item (and a missing marker is
 * VSC_JPEG_STATUS_RESTART, as in vsc_jpeg_decode_u8).  An item that is not its frame's last ends with the check made before a
 * marker is crossed (byte-aligned, less than a byte of padding, the RSTn in sequence) and the marker must stand at the offset
 * the row gives: an offset that lies is VSC_JPEG_STATUS_RESTART.  A frame without restart interval is cut every sub_bytes raw
 * bytes: one wave per sub-stream decodes symbols only from (raw bit position of a block start, slot of the block in its MCU) to
 * the first block start at or behind its end, moving the block start one bit on at a code in no table, a run past coefficient 63
 * or when the bytes run out; round 0 starts sub-stream i at (8 i sub_bytes, 0), each verification round at its predecessor's
 * exit of the round before.  The frame keeps its cut iff the last round changed no exit, the block counts add up to the frame's
 * and every start slot fits; otherwise it is decoded as one item in the same launch.  rounds >= the number of sub-streams always
 * converges.  No host synchronisation anywhere; launches per call: rounds + 1 (if any frame has sub-streams) + 1, then three per
 * chunk.  vsc_jpeg_decode_stats waits for the handle's stream and reports its last split call: out[0] frames cut at markers,
 * out[1] frames cut into sub-streams, out[2] frames the mode wanted cut that were decoded as one item, out[3] items launched
 * (empty ones included).  For tests and measurements. */
int vsc_jpeg_decode_split(vsc_jpeg_decode *h, int32_t mode, int32_t sub_bytes, int32_t rounds, int32_t item_bytes);
int vsc_jpeg_decode_split_u8(vsc_jpeg_decode *h, const uint8_t *bytes_dev, int64_t bytes_len, const int64_t *frames_host, int64_t n_frames,
                             const uint8_t *tables_host, int32_t n_table_sets, const int64_t *restart_ptr_host, const int32_t *restart_off_host,
                             uint8_t *out_dev, int64_t out_len, int32_t *status_dev);
int vsc_jpeg_decode_stats(vsc_jpeg_decode *h, int64_t *out);

/* JPEG files of SEVERAL SCANS, and single-scan frames beside them, in one call (csrc/jpeg_scans.hip; executable contract:
 * tests/jpeg_scans_contract.py): progressive files (SOF2), sequential files of more than one scan, Huffman table ids 0 .. 3.  The
 * pixels are what Pillow gives for the file, bit for bit: the scans of a COMPLETE file accumulate the quantised coefficients its
 * sequential twin holds, and from the coefficients on the decode path is vsc_jpeg_decode_u8's (libjpeg smooths blocks only while
 * some coefficient's precision is unknown; files that end so are refused).  A frame whose scan list is one sequential scan of all
 * its components gets vsc_jpeg_decode_u8's bytes and status.  Operands as in vsc_jpeg_decode_u8 except:
 *   frames_host    int64 [n_frames][VSC_JPEG_FRAME_ROW], a row = {0, 0, height, width, sampling class, 0, the table set that holds
 *                  the frame's quantisation tables, output byte offset, component word (byte c = quantisation table of component
 *                  c), 0};
 *   scans_host     int64 [scan_ptr_host[n_frames]][VSC_JPEG_SCAN_ROW] (HOST memory), a row = {segment offset in bytes_dev, segment
 *                  length (from behind the SOS header to the next marker that is neither RSTn nor a stuffed zero), component mask
 *                  (bit c = component c of the frame is in the scan; the scan header lists them in frame order), Ss, Se, Ah, Al,
 *                  the restart interval in force at the scan (0: none), the table set in force at the scan, Huffman word (byte c =
 *                  DC table | AC table << 2 of component c; 0 for a component outside the scan)};
 *   scan_ptr_host  int64 [n_frames + 1] (HOST memory), CSR: frame i's scans are rows ptr[i] .. ptr[i + 1], in file order, at least one;
 *   tables_host    uint8 [n_table_sets][VSC_JPEG_SCAN_TABLE_SET_BYTES], a set = uint16 quant[4][64] as above, uint8 bits[8][16] and
 *                  uint8 vals[8][256] of the tables DC0 .. DC3, AC0 .. AC3, one byte of quantisation tables present, one whose bit
 *                  (4 * class + id) says that Huffman table is, six zero bytes.  A DHT between two scans gives the later scan another
 *                  set; quantisation tables are taken from the frame row's set alone (a DQT behind the first scan is refused by
 *                  the parser).
 * The points that are easy to get wrong, all part of the contract:
 *   - a scan is sequential (Ss 0, Se 63, Ah = Al = 0), DC (Ss = Se = 0) or AC (Ss > 0, one component); DC first: predictor += difference,
 *     coefficient = predictor << Al; DC refine: ONE BIT per block, no Huffman code, ORed in at 1 << Al;
 *   - AC first: EOBn (run r < 15, size 0) sets EOBRUN = (1 << r) + r more bits and ends this block and EOBRUN - 1 more; values << Al;
 *   - AC refine: size is 0 or 1; for size 1 the SIGN bit comes before the correction bits; the run r counts ZERO-history
 *     coefficients only, every non-zero one that is passed takes one correction bit (1: add 1 << Al away from zero), and the
 *     new +-(1 << Al) lands on the (r + 1)-th zero one; ZRL passes 16 zero ones; the blocks of an EOBRUN, the rest of the block
 *     that starts it included, still take a correction bit per non-zero coefficient of the band;
 *   - a scan of ONE component walks that component's own blocks, ceil(component width / 8) x ceil(component height / 8) row-major
 *     (13 x 17 in 4:2:0: chroma 1 x 2 blocks, not the 2 x 2 of the MCU grid); a scan of several walks the frame's MCUs;
 *   - the restart interval counts those units; a restart byte-aligns, wants RSTn in sequence, zeroes the DC predictors AND EOBRUN;
 *   - coefficients wrap to 16 bits (libjpeg's JCOEF).
 * The scan script of every frame is checked on the host as libjpeg checks it (jdphuff start_pass) before anything is launched:
 * Ss <= Se <= 63, Al and Ah <= 13, a scan with Ss = 0 has Se = 0 or is sequential, an AC scan has one component and follows the
 * component's DC first scan, Ah is 0 for coefficients not yet coded and otherwise their last Al with Al = Ah - 1, and the scans
 * together bring every coefficient of every component to Al = 0 exactly once.  Anything else, and every fault vsc_jpeg_decode_u8
 * refuses, is VSC_ERR_INVALID with nothing written.
 * Three launches per chunk of frames: one wave per frame zeroes the frame's int16 coefficient planes (64 per block, MCU-padded,
 * in the handle's scratch) and decodes its scans into them in file order; eight lanes per block dequantise and run jpeg_idct_islow
 * over all blocks of the chunk; the colour launch is vsc_jpeg_decode_u8's.  Scratch per frame: 3 bytes per sample of its padded
 * planes (1 for the pixel planes, 2 for the coefficients), chunked under the cap of vsc_jpeg_decode_scratch as there.
 * Status: VSC_JPEG_STATUS_DATA / CODE (also a DC size above 16, an AC-refine size above 1) / RUN (also a run past the end of the
 * band or past the last zero coefficient, and an EOBRUN longer than the blocks left in its restart interval or scan -- libjpeg
 * drops the excess silently; here the file is damaged) / RESTART, and VSC_JPEG_STATUS_SCRIPT for a scan the host check should
 * have excluded.  The frame stops at its first fault; no byte outside a scan's segment is read, nothing outside the frame's own
 * planes and output is written, no other frame is disturbed.  No host synchronisation. */
#define VSC_JPEG_SCAN_ROW 10
#define VSC_JPEG_SCAN_TABLE_SET_BYTES 2696
#define VSC_JPEG_STATUS_SCRIPT 5   /* a scan that fits no sequential or progressive script */
int vsc_jpeg_decode_scans_u8(vsc_jpeg_decode *h, const uint8_t *bytes_dev, int64_t bytes_len, const int64_t *frames_host, int64_t n_frames,
                             const int64_t *scans_host, const int64_t *scan_ptr_host, const uint8_t *tables_host, int32_t n_table_sets,
                             uint8_t *out_dev, int64_t out_len, int32_t *status_dev);

/* ------------------------------------------------------------------------ *
 * Building blocks, exported so the parity tests can check each kernel alone.
 * bf16 tensors are raw uint16 bit patterns.
 * ------------------------------------------------------------------------ */
typedef enum vsc_epilogue {
    VSC_EPI_BF16 = 0,        /* out bf16 = acc + bias */
    VSC_EPI_GELU_BF16 = 1,   /* out bf16 = gelu(acc + bias): erf GELU to 2.2e-6 + 6.6e-7 |x| absolute (polynomial) */
    VSC_EPI_QGELU_BF16 = 2,  /* out bf16 = quick_gelu(acc + bias) */
    VSC_EPI_RESADD_F32 = 3,  /* out f32  = residual + acc + bias (out may alias residual) */
    VSC_EPI_PATCH_F32 = 4,   /* out f32 row n*T+1+p = acc + bias + pos[1+p] (row = n*(T-1)+p) */
    VSC_EPI_F32 = 5          /* out f32  = acc + bias */
} vsc_epilogue;

/* out[M,N] = epi(A[M,K] . W[N,K]^T + bias[N]);  A, W bf16 row-major, K % 64 == 0,
 * N % 4 == 0.  bias may be NULL.  `aux_dev` = residual (RESADD) or pos (PATCH),
 * `tokens` = T for PATCH.  Alignment: a_dev, w_dev, bias_dev, aux_dev and out_dev 16 bytes (operands by LDS-DMA in 16-byte pieces,
 * every other access a dwordx4). */
int vsc_gemm_bf16(const uint16_t *a_dev, const uint16_t *w_dev, const float *bias_dev,
                  const float *aux_dev, void *out_dev, int64_t m, int32_t n, int32_t k,
                  int32_t epilogue, int32_t tokens, void *stream);
/* The plan vsc_gemm_bf16 would execute for this shape and epilogue now -- on the current device, with the switches as they stand
 * (csrc/gemm_plan.h); launches nothing and refuses what vsc_gemm_bf16 refuses of a shape.  out = { kernel, tiles_m, tiles_n,
 * N-tiles per group, grid, block, dynamic LDS bytes, 0 }; kernel: 0 the 128 x 128 kernel, 1..4 the 256-row configurations A..D,
 * 5 v3 (256 x 256, one tile per workgroup), 6 v4 (v3 persistent). */
int vsc_gemm_plan(int64_t m, int32_t n, int32_t k, int32_t epilogue, int32_t out[8]);

/* x_inout[M,N] += A[M,K] . W[N,K]^T + bias[N] (float32), y_out[M,N] = LayerNorm_row(x_inout) * gamma + beta in the operand type:
 * the residual GEMM of a transformer block and the LayerNorm behind it.  Where the persistent 256 x 256 kernel has that form
 * (N = 768, whole row blocks per XCD: ceil(M / 256) % 8 == 0, more tiles than CUs) AND the switch VSC_GEMM_LN_TAIL is 1, this
 * is ONE launch whose workgroups normalise every finished 256-row block as a tail; otherwise vsc_gemm_bf16(RESADD) followed by
 * vsc_layernorm_f32.  The same bits either way.  Launches on one stream share a workspace kept by the library.
 * Alignment: y_out_dev 8 bytes, every other pointer 16. */
int vsc_gemm_resadd_ln_bf16(const uint16_t *a_dev, const uint16_t *w_dev, const float *bias_dev, float *x_inout_dev,
                            const float *gamma_dev, const float *beta_dev, uint16_t *y_out_dev, int64_t m, int32_t n, int32_t k,
                            float eps, void *stream);
/* which form the last vsc_gemm_resadd_ln_bf16 / encoder residual GEMM took: 1 one launch with the LayerNorm tail, 2 two launches */
int vsc_gemm_resadd_ln_last_path(void);

/* qkv_dev bf16 [frames*tokens, 3*width] (q | k | v column blocks, head-major inside
 * each) -> out_dev bf16 [frames*tokens, width]; softmax(q k^T / 8) v per head;
 * head_dim 64.  Alignment: qkv_dev and out_dev 16 bytes. */
int vsc_attention_bf16(const uint16_t *qkv_dev, uint16_t *out_dev, int32_t frames, int32_t tokens,
                       int32_t heads, void *stream);

/* The same attention, same layouts and alignment, at any token count 1 .. VSC_ATTENTION_STREAM_MAX_TOKENS: K and V are streamed in
 * blocks of VSC_ATTENTION_STREAM_KEY_BLOCK keys with an online softmax whose row maximum is taken exactly at every block (the
 * accumulated context and row sum are multiplied by exp2(m_old - m_new) once per block); probabilities are rounded to the operand
 * type and the row sum is the sum of the rounded values, so the context is an exact weighted mean of V rows.  vsc_attention_bf16
 * (whole score rows in registers, <= 320 tokens) rounds in another order: the two agree within the operand type's rounding, not bit
 * for bit.  The stream is the FIRST argument.  Refused before anything is launched: tokens outside the range, frames or heads < 1,
 * frames * heads * ceil(tokens / 128) >= 2^31, a null or misaligned pointer.  The encoder uses it above 320 tokens, or everywhere
 * with vsc_set_option("VSC_ATTN_LONG", "1"). */
#define VSC_ATTENTION_STREAM_KEY_BLOCK 128
#define VSC_ATTENTION_STREAM_MAX_TOKENS 16384
int vsc_attention_stream_bf16(void *stream, const uint16_t *qkv_dev, uint16_t *out_dev, int32_t frames, int32_t tokens,
                              int32_t heads);

/* Row LayerNorm over `width` of float32 x [rows,width]; out is bf16 (out_f32 = 0)
 * or float32 (out_f32 = 1; may alias x).  Alignment: x_dev, gamma_dev, beta_dev 16 bytes; out_dev 16 (float32) or 8 (bf16). */
int vsc_layernorm_f32(const float *x_dev, const float *gamma_dev, const float *beta_dev,
                      void *out_dev, int64_t rows, int32_t width, float eps, int32_t out_f32,
                      void *stream);

/* frames float32 [n,C,H,W] -> patches bf16 [n*grid*grid, kpad], k = c*p*p + py*p + px,
 * zero-filled up to kpad (kpad % 64 == 0).  Alignment: patches_dev 16 bytes; frames_dev 16 when patch % 8 == 0 (other patch sizes are
 * gathered pixel by pixel). */
int vsc_patchify_bf16(const float *frames_dev, uint16_t *patches_dev, int64_t n, int32_t channels,
                      int32_t image, int32_t patch, int32_t kpad, void *stream);

/* Swin-V2 windowed cosine attention, head_dim 32.  qkv_dev bf16 [frames*res*res, 3*heads*32] in
 * image token order; the cyclic shift and window partition are index math.  bias_dev f32
 * [heads, (2*window-1)^2]: the compact relative-position table 16*sigmoid(cpb_mlp(coords)),
 * bias(i, j) = table[(yi-yj+window-1)*(2*window-1) + xi-xj+window-1]; scale_dev f32 [heads] =
 * exp(min(logit_scale, ln 100)).  window is 8, 12, 16 or 24 and divides res; shift is any 0 <= shift < window (the reference
 * uses 0 and window / 2; 1 and window - 1 are tested as well); every other value of either is refused.
 * Bounded form (optional, per head): cosine logits cannot exceed U = scale + max(table).  A caller that has subtracted U from a
 * head's table and knows 2 scale + max(table) - min(table) <= 69 (so that no probability underflows) passes -scale for that
 * head: the kernel then skips the row maximum of the softmax -- the same quotient, a sixth fewer vector instructions
 * (vsc_swin_finalize does this for its own tables).
 * Alignment: qkv_dev and out_dev 16 bytes (bias_dev and scale_dev are read element by element). */
int vsc_window_attention_bf16(const uint16_t *qkv_dev, uint16_t *out_dev, const float *bias_dev,
                              const float *scale_dev, int32_t frames, int32_t res, int32_t window,
                              int32_t shift, int32_t heads, void *stream);
/* x_out = (x_in ? x_in : 0) + LayerNorm(t) ; xb = bf16(x_out).  x_in may be NULL or alias x_out.
 * Alignment: xb_dev 8 bytes, every other pointer 16. */
int vsc_ln_residual_f32(const float *t_dev, const float *gamma_dev, const float *beta_dev,
                        const float *x_in_dev, float *x_out_dev, uint16_t *xb_dev, int64_t rows,
                        int32_t width, float eps, void *stream);
/* The same update with the LayerNorm input produced in place by a GEMM whose tile owns whole rows:
 * x_out = (x_in ? x_in : 0) + LayerNorm(A[m,k] W[n,k]^T + bias) ; xb = bf16(x_out).  n in {128, 256, 512},
 * k % 32 == 0 (torch2scripts.py:297-300, 361-362: Swin-V2 res-post-norm and the PatchMerging norm).
 * Alignment: xb_dev 8 bytes, every other pointer 16. */
int vsc_gemm_ln_bf16(const uint16_t *a_dev, const uint16_t *w_dev, const float *bias_dev,
                     const float *gamma_dev, const float *beta_dev, const float *x_in_dev,
                     float *x_out_dev, uint16_t *xb_dev, int64_t m, int32_t n, int32_t k, float eps,
                     void *stream);
/* The whole MLP of a Swin-V2 block in one kernel (c = 128, 256 or 512), in place on the residual stream:
 *   x += LayerNorm(GELU(xb W1[4c,c]^T + b1) W2[c,4c]^T + b2) * gamma + beta ;  xb = bf16(x)
 * (Mlp + norm2 + residual of SwinTransformerBlock.forward, torch2scripts.py:18-35, 190-215, 297-300) -- the hidden activations
 * [m, 4c] never reach memory.  w2p_dev is fc2.weight in the kernel's contraction order, as made by
 * vsc_swin_mlp_permute_hidden_f32 (host arrays of c * 4c floats, once per model load) and then converted to bf16: for
 * c = 128 / 256 the hidden axis of every row reordered inside its 32-blocks, for c = 512 additionally chunk-major
 * [64 chunks][512][32] (one wave per SIMD with the whole register file: csrc/swin_mlp512.hip; m < 2^21 rows per call).
 * Alignment (all three fused entries): the bf16 weight matrices, att_dev, x_dev, xb_dev and qkv_next_dev 16 bytes; the bias and
 * LayerNorm vectors are read element by element. */
int vsc_swin_mlp_bf16(const uint16_t *w1_dev, const float *b1_dev, const uint16_t *w2p_dev, const float *b2_dev,
                      const float *gamma_dev, const float *beta_dev, float *x_dev, uint16_t *xb_dev, int64_t m, int32_t c,
                      float eps, void *stream);
int vsc_swin_mlp_permute_hidden_f32(const float *w2_host, float *w2p_host, int32_t c);
/* The whole second half of a Swin-V2 block in one kernel (c = 128, 256 or 512), in place on the residual stream
 * (SwinTransformerBlock.forward after the window attention, torch2scripts.py:284-300):
 *   x1 = x + LayerNorm(att Wp[c,c]^T + bp) * gamma1 + beta1 ;  x = x1 + LayerNorm(GELU(bf16(x1) W1^T + b1) W2^T + b2) * gamma2 + beta2 ;  xb = bf16(x)
 * att_dev [m, c] bf16 is the attention output; xb_dev is written only (the MLP's input is formed in registers).  w2p_dev as for
 * vsc_swin_mlp_bf16.  At c = 512 x1 passes through x_dev once as fp32 between the two halves; m < 2^21. */
int vsc_swin_proj_mlp_bf16(const uint16_t *att_dev, const uint16_t *wp_dev, const float *bp_dev, const float *gamma1_dev, const float *beta1_dev,
                           const uint16_t *w1_dev, const float *b1_dev, const uint16_t *w2p_dev, const float *b2_dev, const float *gamma2_dev,
                           const float *beta2_dev, float *x_dev, uint16_t *xb_dev, int64_t m, int32_t c, float eps, void *stream);
/* ... and the NEXT block's qkv Linear behind it (c = 512 only -- the stage with 18 blocks, torch2scripts.py:284-300 followed by the
 * next block's WindowAttention.forward first line, :120-125):   qkv_next = bf16(x) Wq[3c,c]^T + bq   with x the block's output.
 * The bf16 shadow never leaves the registers (no xb_dev), the next block's qkv launch and its read of the shadow are gone.
 * bq_dev [3c] = (q_bias | 0 | v_bias).  Same bits as vsc_swin_proj_mlp_bf16 followed by vsc_gemm_bf16 on its shadow. */
int vsc_swin_proj_mlp_qkv_bf16(const uint16_t *att_dev, const uint16_t *wp_dev, const float *bp_dev, const float *gamma1_dev, const float *beta1_dev,
                               const uint16_t *w1_dev, const float *b1_dev, const uint16_t *w2p_dev, const float *b2_dev, const float *gamma2_dev,
                               const float *beta2_dev, const uint16_t *wq_dev, const float *bq_dev, float *x_dev, uint16_t *qkv_next_dev,
                               int64_t m, int32_t c, float eps, void *stream);
/* PatchMerging gather on bf16 tokens [frames, res, res, c] -> [frames*(res/2)^2, 4c].  Alignment: both pointers 16 bytes. */
int vsc_merge_gather_bf16(const uint16_t *xb_dev, uint16_t *out_dev, int64_t frames, int32_t res,
                          int32_t c, void *stream);

/* Measurement aid for vsc_swin_mlp_bf16 at c = 512: buf_dev (NULL: off) receives, per workgroup and wave, eight uint32 -- shader
 * cycles spent waiting for the wave's own LDS-DMA pieces, at the chunk barrier, in the chunk's work, before the epilogue, in the
 * epilogue -- when the timing variant of the kernel runs (vsc_set_option("VSC_SWIN_MLP_ABL", "5")); [ceil(m / 128)][4][8]. */
int vsc_debug_mlp512_timing(uint32_t *buf_dev);
/* Measurement aid: one wave spins for `ticks` shader cycles (s_memtime) and stores the elapsed count. */
int vsc_debug_spin_ticks(uint64_t ticks, uint64_t *out_dev, void *stream);

/* ------------------------------------------------------------------------
 * Matching track: the fp32 convolution layers of the pair classifier (timm mobilenetv3_small_100) and the refinement
 * net (timm hrnet_w18 features + 1x1 fuse head) that the reference runs as TorchScript modules on similarity maps
 *   VSC22-Matching-Track-1st/infer/infer_matching.py:158-175 (match_classify), :177-204 (match_refine),
 *   train/models.py:6-40 (ClassifyModel, HRnet).
 * Activations are NHWC float32; BatchNorm is folded into weight / bias by the host (vsc_hip/cnn.py).
 * ------------------------------------------------------------------------ */
enum { VSC_ACT_NONE = 0, VSC_ACT_RELU = 1, VSC_ACT_HARDSWISH = 2, VSC_ACT_HARDSIGMOID = 3, VSC_ACT_GELU = 4 };

/* floats per packed weight row: cin * kh * kw rounded up to a multiple of 32 */
int vsc_conv_packed_k(int32_t cin, int32_t kh, int32_t kw);
/* w_dev [cout, k] float32 with k = (kh, kw, cin) order (torch's [cout, cin, kh, kw] permuted to [cout, kh, kw, cin]) ->
 * packed_dev [cout, vsc_conv_packed_k]: rows zero-padded to a multiple of 32 floats for the fp32 MFMA tiles; done once per layer. */
int vsc_conv_pack_weight_f32(const float *w_dev, float *packed_dev, int32_t cout, int32_t k, void *stream);
/* out[n, ho, wo, 0:cout] (row stride ldo) = act(conv2d(x[n, h, w, 0:cin] (row stride ldx), W) + bias [+ res[.., 0:cout]
 * (row stride ldr)]) -- torch.nn.functional.conv2d(stride, padding) + the fused tail of a BN/ReLU/residual block.
 * Layers that materialise their patch matrix share ONE grow-only scratch buffer per device: issue the convolutions of a
 * device from one stream at a time (calls from several host threads are serialised on an internal mutex, their kernels
 * are not ordered against each other).
 * Arithmetic: fp32 products with fp32 accumulation on the fp32 matrix pipe.  These 3 x 3 / stride 1 / pad 1 layers instead multiply
 * bf16 triples (x = x1 + x2 + x3, six products per multiply, fp32 accumulation: the same error against float64 as the fp32 pipe):
 *     cin == 20 with cout <= 20, cin == 36 with cout <= 36           (cin as passed: HRNet's 18 channels come padded to 20)
 *     cin == 64 with cout <= 64, cin == 256 with cout <= 32          dense rows (ldx == cin), >= 65 536 output pixels
 *     cin == 72 or 144 with 48 <= cout <= 160                        dense rows, 8 192 <= pixels, <= 16 M input elements
 * each only with 16-byte aligned x / weights / out / res / bias (anything else takes the fp32 tile kernels); VSC_CONV_X3=0 or
 * VSC_CONV_DIRECT=0 (vsc_set_option) switch all of them off; vsc_conv_last_pipe() tells which pipe a call took.  The 72- / 144-
 * channel form keeps its split operands in a second per-device scratch buffer: the one-stream-at-a-time rule above covers it too. */
int vsc_conv2d_f32(const float *x_dev, int64_t n, int32_t h, int32_t w, int32_t cin, int32_t ldx, const float *w_packed_dev,
                   const float *bias_dev, int32_t cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad,
                   const float *res_dev, int32_t ldr, int32_t act, float *out_dev, int32_t ldo, void *stream);
/* depthwise convolution: w_dev [c, kh * kw], x / out dense NHWC */
int vsc_dwconv2d_f32(const float *x_dev, int64_t n, int32_t h, int32_t w, int32_t c, const float *w_dev,
                     const float *bias_dev, int32_t kh, int32_t kw, int32_t stride, int32_t pad, int32_t act,
                     float *out_dev, void *stream);
/* out[n, c] = mean over the hw positions of x[n, hw, c] (AdaptiveAvgPool2d(1)) */
int vsc_global_avgpool_f32(const float *x_dev, int64_t n, int32_t hw, int32_t c, float *out_dev, void *stream);
/* x[n, hw, c] *= scale[n, c] (squeeze-excite gate) */
int vsc_channel_scale_f32(float *x_dev, const float *scale_dev, int64_t n, int32_t hw, int32_t c, void *stream);
/* One squeeze-excite block in place (timm SqueezeExcite: x * gate_fn(conv_expand(act(conv_reduce(x.mean((2, 3)))))), as one launch for
 * maps whose image fits LDS ((hw c + 2 c + cr) * 4 <= 150 KiB; larger ones: vsc_global_avgpool_f32 + vsc_conv2d_f32 x 2 +
 * vsc_channel_scale_f32): x[n, hw, c] *= act2(W2 act1(W1 mean_hw(x) + b1) + b2), W1 [cr, c] / W2 [c, cr] as packed by
 * vsc_conv_pack_weight_f32 (1 x 1 kernels), biases may be null.  c a multiple of 4. */
int vsc_se_block_f32(float *x_dev, int64_t n, int32_t hw, int32_t c, const float *w1_packed_dev, const float *b1_dev, int32_t cr,
                     const float *w2_packed_dev, const float *b2_dev, int32_t act1, int32_t act2, void *stream);
/* out[n, y, x, coff + ch] = act((accumulate ? out : 0) + src[n, y / factor, x / factor, ch]) for the h x w output grid:
 * nn.Upsample(scale_factor, 'nearest') fused with the sum of an HRNet fuse layer or with torch.cat along channels. */
int vsc_upsample_add_f32(const float *src_dev, int64_t n, int32_t h, int32_t w, int32_t c, int32_t factor, float *out_dev,
                         int32_t ldo, int32_t coff, int32_t accumulate, int32_t act, void *stream);
/* One HRNet fuse node in one pass (timm HighResolutionModule.forward: y = relu(sum_j fuse_layers[i][j](x[j])), the sum taken in
 * order of j): out[n, y, x, ch] = act(((base[n, y, x, ch] + up(src0)) + up(src1)) + up(src2)), up = nearest upsampling by a
 * power-of-two factor, absent sources null.  base [n, h, w, ldb >= c] may be null or alias out [n, h, w, ldo >= c]; srcK
 * [n, h / factorK, w / factorK, c] dense.  c, ldb, ldo multiples of 4, operands 16-byte aligned. */
int vsc_upsample_sum_f32(const float *base_dev, int32_t ldb, const float *src0_dev, int32_t factor0, const float *src1_dev,
                         int32_t factor1, const float *src2_dev, int32_t factor2, int64_t n, int32_t h, int32_t w, int32_t c,
                         int32_t act, float *out_dev, int32_t ldo, void *stream);

/* Diagnostic (bench.py: FLOPs per pipe): which pipe the last vsc_conv2d_f32 call of this process ran on -- 0 the fp32 matrix / vector
 * pipe, 1 the bf16 matrix pipe on split operands (3 x 3 / stride 1 layers with 20, 36, 64, 72, 144 input channels and the 256 -> <= 32
 * transition, unless VSC_CONV_X3=0 / VSC_CONV_DIRECT=0: six bf16 products per multiply, fp32-level error). */
int vsc_conv_last_pipe(void);

/* fp32 multi-head self-attention for short sequences: out[t, h*dh:(h+1)*dh] = softmax(q k^T / sqrt(dh)) v per head, qkv
 * [tokens, 3 * heads * head_dim] float32 as q | k | v column blocks.  Used by the video-score head (BERT encoder over <= 258
 * tokens, infer/extract_query_feats.py:165-173), whose sigmoid gate is compared with 1e-3 and therefore runs in fp32. */
int vsc_attention_f32(const float *qkv_dev, float *out_dev, int32_t tokens, int32_t heads, int32_t head_dim, void *stream);
/* The same for `seqs` sequences of the same length stored back to back (qkv [seqs * tokens, 3 * heads * head_dim]): the video-score
 * heads of a group of query videos in one launch per layer (their Linears and LayerNorms are row-wise and take all rows at once). */
int vsc_attention_f32_batch(const float *qkv_dev, float *out_dev, int32_t tokens, int32_t heads, int32_t head_dim, int32_t seqs,
                            void *stream);
/* ... and for sequences of different lengths (the video-score heads of a group of query videos of any lengths in one launch per
 * layer; train_vid_score/video/model.py: one video per forward): sequence z = rows row_offsets_dev[z] .. row_offsets_dev[z + 1] of
 * qkv_dev / out_dev (int32 [seqs + 1] on the device), max_tokens = the longest sequence.  A row's result is the same bits as in
 * vsc_attention_f32 on its sequence alone. */
int vsc_attention_f32_varlen(const float *qkv_dev, float *out_dev, const int32_t *row_offsets_dev, int32_t seqs, int32_t max_tokens,
                             int32_t heads, int32_t head_dim, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VSC_HIP_H */
