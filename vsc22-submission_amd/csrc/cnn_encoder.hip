// vsc_cnn_encoder: weights, workspace and launch sequence of the CNN descriptor backbone -- a ResNet-50-shaped bottleneck network
// (torchvision's v1.5: the stride of a stage's first block sits on its 3 x 3 convolution) with the SSCD head: GeM(p) over the last map,
// Linear, optional L2 (reference model: infer/vsc/baseline, sscd_disc_mixup; head classes: train/train_v106/.../backbones/sscd.py:10-47).
//
// BatchNorm is folded into weight + bias by the caller (vsc_hip/weights.py: from_sscd_torchvision), so every tensor here is a
// convolution weight [cout, cin, kh, kw] with its bias [cout]:
//   conv1.{weight,bias}                                   7 x 7 stride 2, 3 -> stem_width
//   layerL.B.conv{1,2,3}.{weight,bias}                    1 x 1 -> 3 x 3 (stride 2 in block 0 of layers 2..4) -> 1 x 1
//   layerL.0.downsample.{weight,bias}                     1 x 1 projection of the identity (same stride)
//   head.{weight,bias}                                    [head_out, widths[3]] fp32
// finalize reorders every weight to [cout, kh, kw, cin] (the implicit GEMM's K order) and rounds it to the operand type.
//
// HBM layout of one call of n frames of H x W (NHWC, operand type): rows [n H1 W1, 192] stem im2col -> S [n H1 W1, stem] -> max-pool ->
// X [n H2 W2, stem]; per block T1 = relu(conv1 X), T2 = relu(conv2 T1), D = downsample X (block 0), Y = relu(conv3 T2 + identity);
// X and Y change roles.  Block outputs and the residual stay in the operand type: measured against the fixtures, fp16 operands meet
// the 1e-3 tolerance by a factor of 8 that way.
// The workspace is sized by finalize for max_pixels = n H W of even extents and grows (never shrinks) when a call with odd extents
// needs a few rows more; a call above max_pixels is refused.
#include <string>

#include "conv16.h"
#include "model_host.h"

struct CnnConvW {
    uint16_t *w = nullptr;
    float *b = nullptr;
};
struct CnnBlockW {
    CnnConvW c1, c2, c3, down;
};

struct vsc_cnn_encoder : ModelHost {
    vsc_cnn_encoder() : ModelHost("cnn_encoder", "cnn_encoder ") {}
    vsc_cnn_encoder_config cfg;
    CnnConvW stem;
    std::vector<CnnBlockW> blocks[4];
    float *head_w = nullptr, *head_b = nullptr;
    // workspace (grow-only, freed with the handle)
    enum { ROWS, S, X, Y, T1, T2, D, POOLED, NBUF };
    void *buf[NBUF] = {nullptr};
    size_t cap[NBUF] = {0};
    int64_t ws_bytes = 0;

    int cin_of(int s, int b) const { return b ? cfg.widths[s] : (s ? cfg.widths[s - 1] : cfg.stem_width); }
    int stride_of(int s, int b) const { return (b == 0 && s > 0) ? 2 : 1; }
    ~vsc_cnn_encoder() {
        for (int i = 0; i < NBUF; ++i)
            if (buf[i]) (void)hipFree(buf[i]);
    }
};

static_assert(VSC_CNN_PROF_CLASSES <= ModelHost::MAX_CLASSES, "profile classes");

namespace {

std::string block_name(int s, int b) { return "layer" + std::to_string(s + 1) + "." + std::to_string(b) + "."; }

}  // namespace

// positions of every map of a call: stem (H1 x W1), pooled / stage 0 (H2 x W2), stages 1..3
struct CnnShape {
    int h1, w1, hs[4], ws[4];
};
static CnnShape cnn_shape(int h, int w) {
    CnnShape g;
    g.h1 = (h - 1) / 2 + 1;
    g.w1 = (w - 1) / 2 + 1;
    g.hs[0] = (g.h1 - 1) / 2 + 1;
    g.ws[0] = (g.w1 - 1) / 2 + 1;
    for (int s = 1; s < 4; ++s) {
        g.hs[s] = (g.hs[s - 1] - 1) / 2 + 1;
        g.ws[s] = (g.ws[s - 1] - 1) / 2 + 1;
    }
    return g;
}

// element counts of the workspace buffers for n frames of h x w
static void cnn_need(const vsc_cnn_encoder *e, int64_t n, int h, int w, size_t need[vsc_cnn_encoder::NBUF]) {
    typedef vsc_cnn_encoder E;
    const vsc_cnn_encoder_config &c = e->cfg;
    const CnnShape g = cnn_shape(h, w);
    const int64_t p1 = n * g.h1 * g.w1;
    int64_t xy = n * g.hs[0] * g.ws[0] * c.stem_width, t1 = 0, t2 = 0, d = 0;
    for (int s = 0; s < 4; ++s) {
        const int64_t p_in = n * (s ? (int64_t)g.hs[s - 1] * g.ws[s - 1] : (int64_t)g.hs[0] * g.ws[0]);
        const int64_t p_out = n * (int64_t)g.hs[s] * g.ws[s];
        const int64_t mid = c.widths[s] / 4;
        if (p_in * mid > t1) t1 = p_in * mid;
        if (p_out * mid > t2) t2 = p_out * mid;
        if (p_out * c.widths[s] > xy) xy = p_out * c.widths[s];
        if (p_out * c.widths[s] > d) d = p_out * c.widths[s];
    }
    for (int i = 0; i < E::NBUF; ++i) need[i] = 0;
    need[E::ROWS] = (size_t)p1 * VSC_STEM_KPAD * 2;
    need[E::S] = (size_t)p1 * c.stem_width * 2;
    need[E::X] = need[E::Y] = (size_t)xy * 2;
    need[E::T1] = (size_t)t1 * 2;
    need[E::T2] = (size_t)t2 * 2;
    need[E::D] = (size_t)d * 2;
    need[E::POOLED] = (size_t)n * c.widths[3] * 4;
}

static int cnn_grow(vsc_cnn_encoder *e, const size_t need[vsc_cnn_encoder::NBUF]) {
    for (int i = 0; i < vsc_cnn_encoder::NBUF; ++i) {
        if (need[i] <= e->cap[i]) continue;
        if (e->buf[i]) {
            VSC_CHECK_HIP(hipFree(e->buf[i]));   // (waits for the device: nothing in flight still reads the old buffer)
            e->ws_bytes -= (int64_t)e->cap[i];
            e->buf[i] = nullptr;
            e->cap[i] = 0;
        }
        hipError_t err = hipMalloc(&e->buf[i], need[i]);
        if (err != hipSuccess) {
            e->buf[i] = nullptr;
            vsc_set_error("cnn_encoder: hipMalloc(%zu) failed: %s", need[i], hipGetErrorString(err));
            return VSC_ERR_NOMEM;
        }
        e->cap[i] = need[i];
        e->ws_bytes += (int64_t)need[i];
    }
    return VSC_OK;
}

extern "C" int vsc_cnn_encoder_create(const vsc_cnn_encoder_config *cfg, vsc_cnn_encoder **out) {
    VSC_REQUIRE(cfg && out, "cnn_encoder create: null argument");
    const vsc_cnn_encoder_config &c = *cfg;
    VSC_REQUIRE(c.stem_width >= 64 && c.stem_width % 64 == 0, "cnn_encoder: stem width %d must be a multiple of 64", c.stem_width);
    for (int s = 0; s < 4; ++s) {
        VSC_REQUIRE(c.widths[s] >= 256 && c.widths[s] % 256 == 0, "cnn_encoder: stage %d width %d must be a multiple of 256 (its bottleneck width a multiple of 64)", s, c.widths[s]);
        VSC_REQUIRE(c.depths[s] >= 1 && c.depths[s] <= 64, "cnn_encoder: stage %d depth %d", s, c.depths[s]);
    }
    VSC_REQUIRE(c.head_in == c.widths[3], "cnn_encoder: head_in %d is not the last stage's width %d", c.head_in, c.widths[3]);
    VSC_REQUIRE(c.head_in <= 2048 && c.head_out >= 1 && c.head_out <= 2048, "cnn_encoder: head %d -> %d unsupported (at most 2048 each)", c.head_in, c.head_out);
    VSC_REQUIRE(c.gem_p > 0.f, "cnn_encoder: gem_p %g", (double)c.gem_p);
    VSC_REQUIRE(c.l2 == 0 || c.l2 == 1, "cnn_encoder: l2 %d (0 or 1)", c.l2);
    VSC_REQUIRE(c.max_pixels >= 1 && c.max_pixels < (1ll << 31), "cnn_encoder: max_pixels %lld outside 1 .. 2^31 - 1", (long long)c.max_pixels);
    vsc_cnn_encoder *e = new vsc_cnn_encoder();
    e->cfg = c;
    e->expect("conv1.weight", (size_t)c.stem_width * 147);
    e->expect("conv1.bias", c.stem_width);
    for (int s = 0; s < 4; ++s)
        for (int b = 0; b < c.depths[s]; ++b) {
            const std::string p = block_name(s, b);
            const size_t cin = e->cin_of(s, b), mid = c.widths[s] / 4, wd = c.widths[s];
            e->expect(p + "conv1.weight", mid * cin);
            e->expect(p + "conv1.bias", mid);
            e->expect(p + "conv2.weight", mid * mid * 9);
            e->expect(p + "conv2.bias", mid);
            e->expect(p + "conv3.weight", wd * mid);
            e->expect(p + "conv3.bias", wd);
            if (b == 0) {
                e->expect(p + "downsample.weight", wd * cin);
                e->expect(p + "downsample.bias", wd);
            }
        }
    e->expect("head.weight", (size_t)c.head_out * c.head_in);
    e->expect("head.bias", c.head_out);
    *out = e;
    return VSC_OK;
}

extern "C" void vsc_cnn_encoder_destroy(vsc_cnn_encoder *e) { delete e; }

extern "C" int vsc_cnn_encoder_set_weight(vsc_cnn_encoder *e, const char *name, const float *host, size_t count) {
    VSC_REQUIRE(e && name && host, "cnn_encoder set_weight: null argument");
    return e->set_weight(name, host, count);
}

// [cout, cin, k, k] -> [cout, k, k, cin_pad] (zero padded), rounded to the operand type on the device
static int cnn_upload_conv(vsc_cnn_encoder *e, const std::string &prefix, int cout, int cin, int k, int kpad, CnnConvW *dst) {
    const std::vector<float> &w = e->host_w.at(prefix + "weight");
    const int kdim = k * k * cin;
    std::vector<float> t((size_t)cout * kdim);
    for (int o = 0; o < cout; ++o)
        for (int ci = 0; ci < cin; ++ci)
            for (int rs = 0; rs < k * k; ++rs) t[(size_t)o * kdim + (size_t)rs * cin + ci] = w[((size_t)o * cin + ci) * k * k + rs];
    VSC_TRY(e->upload_bf16(t, prefix + "weight", cout, kdim, kpad, &dst->w));
    return e->upload_f32(prefix + "bias", &dst->b);
}

extern "C" int vsc_cnn_encoder_finalize(vsc_cnn_encoder *e) {
    VSC_REQUIRE(e, "cnn_encoder finalize: null");
    if (e->finalized) return VSC_OK;
    VSC_TRY(e->all_set());
    const vsc_cnn_encoder_config &c = e->cfg;
    VSC_TRY(cnn_upload_conv(e, "conv1.", c.stem_width, 3, 7, VSC_STEM_KPAD, &e->stem));
    for (int s = 0; s < 4; ++s) {
        e->blocks[s].resize(c.depths[s]);
        for (int b = 0; b < c.depths[s]; ++b) {
            const std::string p = block_name(s, b);
            const int cin = e->cin_of(s, b), mid = c.widths[s] / 4, wd = c.widths[s];
            CnnBlockW &B = e->blocks[s][b];
            VSC_TRY(cnn_upload_conv(e, p + "conv1.", mid, cin, 1, cin, &B.c1));
            VSC_TRY(cnn_upload_conv(e, p + "conv2.", mid, mid, 3, 9 * mid, &B.c2));
            VSC_TRY(cnn_upload_conv(e, p + "conv3.", wd, mid, 1, mid, &B.c3));
            if (b == 0) VSC_TRY(cnn_upload_conv(e, p + "downsample.", wd, cin, 1, cin, &B.down));
        }
    }
    VSC_TRY(e->upload_f32("head.weight", &e->head_w));
    VSC_TRY(e->upload_f32("head.bias", &e->head_b));
    // the workspace of one frame of max_pixels with even extents (2 x max_pixels / 2, rounded up to a multiple of 32 rows): what a call
    // of any n frames of even H x W with n H W <= max_pixels needs; odd extents grow it on their first call
    size_t need[vsc_cnn_encoder::NBUF];
    const int64_t hh = (c.max_pixels + 63) / 64 * 32;
    cnn_need(e, 1, (int)(hh < (1ll << 30) ? hh : (1ll << 30)), 2, need);
    need[vsc_cnn_encoder::POOLED] = (size_t)c.widths[3] * 4 * 64;
    VSC_TRY(cnn_grow(e, need));
    e->drop_host();
    return VSC_OK;
}

extern "C" int64_t vsc_cnn_encoder_workspace_bytes(const vsc_cnn_encoder *e) { return e ? e->ws_bytes : 0; }

static int cnn_forward_impl(vsc_cnn_encoder *e, const float *frames, const uint8_t *frames_u8, const float *mean, const float *std, int64_t n,
                            int32_t h, int32_t w, float *desc, void *stream_) {
    typedef vsc_cnn_encoder E;
    VSC_REQUIRE(e, "cnn_encoder forward: null encoder");
    VSC_REQUIRE((frames || frames_u8) && desc, "cnn_encoder forward: null frames or descriptors");
    VSC_REQUIRE(n >= 0, "cnn_encoder forward: n %lld is negative", (long long)n);
    VSC_REQUIRE(h >= 1 && w >= 1, "cnn_encoder forward: H %d, W %d must be >= 1", h, w);
    VSC_REQUIRE((double)n * h * w <= (double)e->cfg.max_pixels, "cnn_encoder forward: n H W = %lld x %d x %d is above the workspace's max_pixels %lld",
                (long long)n, h, w, (long long)e->cfg.max_pixels);
    VSC_TRY(e->forward_ready());
    if (n == 0) return VSC_OK;
    const vsc_cnn_encoder_config &c = e->cfg;
    hipStream_t st = (hipStream_t)stream_;
    size_t need[E::NBUF];
    cnn_need(e, n, h, w, need);
    VSC_TRY(cnn_grow(e, need));
    const CnnShape g = cnn_shape(h, w);
#define PROF(cls) ProfScope _ps(e, (cls), st)
    uint16_t *rows = (uint16_t *)e->buf[E::ROWS], *sm = (uint16_t *)e->buf[E::S], *x = (uint16_t *)e->buf[E::X], *y = (uint16_t *)e->buf[E::Y];
    uint16_t *t1 = (uint16_t *)e->buf[E::T1], *t2 = (uint16_t *)e->buf[E::T2], *d = (uint16_t *)e->buf[E::D];
    float *pooled = (float *)e->buf[E::POOLED];
    { PROF(VSC_CNN_PROF_STEM_ROWS); VSC_TRY(launch_stem_rows(frames_u8, frames, rows, n, h, w, mean, std, st)); }
    { PROF(VSC_CNN_PROF_STEM_CONV); VSC_TRY(launch_conv16(rows, e->stem.w, e->stem.b, nullptr, sm, n, g.h1, g.w1, VSC_STEM_KPAD, c.stem_width, 1, 1, 1, st)); }
    { PROF(VSC_CNN_PROF_MAXPOOL); VSC_TRY(launch_maxpool3x3s2(sm, x, n, g.h1, g.w1, c.stem_width, st)); }
    int hc = g.hs[0], wc = g.ws[0];   // extents of x
    for (int s = 0; s < 4; ++s) {
        PROF(VSC_CNN_PROF_STAGE0 + s);
        const int mid = c.widths[s] / 4, wd = c.widths[s];
        for (int b = 0; b < c.depths[s]; ++b) {
            const CnnBlockW &B = e->blocks[s][b];
            const int cin = e->cin_of(s, b), stride = e->stride_of(s, b);
            const int ho = conv16_out_extent(hc, 3, stride), wo = conv16_out_extent(wc, 3, stride);
            VSC_TRY(launch_conv16(x, B.c1.w, B.c1.b, nullptr, t1, n, hc, wc, cin, mid, 1, 1, 1, st));
            VSC_TRY(launch_conv16(t1, B.c2.w, B.c2.b, nullptr, t2, n, hc, wc, mid, mid, 3, stride, 1, st));
            const uint16_t *idn = x;
            if (b == 0) {
                VSC_TRY(launch_conv16(x, B.down.w, B.down.b, nullptr, d, n, hc, wc, cin, wd, 1, stride, 0, st));
                idn = d;
            }
            VSC_TRY(launch_conv16(t2, B.c3.w, B.c3.b, idn, y, n, ho, wo, mid, wd, 1, 1, 1, st));
            uint16_t *tx = x; x = y; y = tx;
            hc = ho;
            wc = wo;
        }
    }
    {
        PROF(VSC_CNN_PROF_POOL_HEAD);
        VSC_TRY(launch_gem_pool_bf16(x, pooled, n, hc * wc, c.widths[3], c.gem_p, st));
        VSC_TRY(launch_head(pooled, e->head_w, e->head_b, desc, n, c.head_in, c.head_out, c.l2, st));
    }
#undef PROF
    return VSC_OK;
}

extern "C" int vsc_cnn_encoder_forward(void *stream, vsc_cnn_encoder *e, const float *frames_dev, int64_t n, int32_t h, int32_t w, float *desc_dev) {
    VSC_REQUIRE_ALIGNED("cnn_encoder forward", frames_dev, 4);
    return cnn_forward_impl(e, frames_dev, nullptr, nullptr, nullptr, n, h, w, desc_dev, stream);
}

extern "C" int vsc_cnn_encoder_forward_u8(void *stream, vsc_cnn_encoder *e, const uint8_t *frames_u8_dev, int64_t n, int32_t h, int32_t w, const float *mean,
                                          const float *std, float *desc_dev) {
    VSC_REQUIRE(!frames_u8_dev || (mean && std), "cnn_encoder forward_u8: null mean or std");
    return cnn_forward_impl(e, nullptr, frames_u8_dev, mean, std, n, h, w, desc_dev, stream);
}

extern "C" int vsc_cnn_encoder_set_profiling(vsc_cnn_encoder *e, int32_t on) {
    VSC_REQUIRE(e, "cnn_encoder set_profiling: null encoder");
    e->reset(on != 0);
    return VSC_OK;
}

extern "C" int vsc_cnn_encoder_get_profile(vsc_cnn_encoder *e, double *ms_out, int64_t *launches_out) {
    VSC_REQUIRE(e && ms_out && launches_out, "cnn_encoder get_profile: null argument");
    return e->collect(ms_out, launches_out, VSC_CNN_PROF_CLASSES);
}
