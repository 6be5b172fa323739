// vsc_encoder: weights, workspace and the launch sequence of one frame batch through the
// ViT encoder + descriptor head.  Host-side C++; every numeric step is a HIP kernel from
// gemm_bf16.hip / attention.hip / elementwise.hip.
//
// HBM layout for one step of B frames (T tokens, width D, M = B*T):
//   patches bf16 [B*(T-1), Kpad]     x   f32 [M, D]   (residual stream, fp32 throughout)
//   y       bf16 [M, D]  (LN output, then reused for the attention output)
//   qkv     bf16 [M, 3D]             h   bf16 [M, mlp]
//   pooled  f32  [B, D]
// Weights: matrices as bf16 [out, in] (PyTorch Linear layout == the GEMM's W[N,K]),
// biases / LayerNorm / cls / pos / head as f32.
#include <string.h>

#include "model_host.h"

struct LayerW {
    uint16_t *qkv_w, *proj_w, *fc1_w, *fc2_w;
    float *qkv_b, *proj_b, *fc1_b, *fc2_b, *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    // LayerNorm folded into the following GEMM (see fold_ln): W' = gamma o W (bf16), colsum_n = sum_k W'[n,k],
    // bias'_n = b_n + sum_k beta_k W[n,k]
    uint16_t *qkv_wf = nullptr, *fc1_wf = nullptr;
    float *qkv_cs = nullptr, *qkv_bf = nullptr, *fc1_cs = nullptr, *fc1_bf = nullptr;
};

struct vsc_encoder : ModelHost {
    vsc_encoder() : ModelHost("encoder", "") {}
    vsc_encoder_config cfg;
    int tokens = 0, grid = 0, kpatch = 0, kpad = 0, desc_dim = 0;
    std::vector<LayerW> layers;
    uint16_t *patch_w = nullptr;
    float *patch_b = nullptr, *cls = nullptr, *pos = nullptr, *lnpre_g = nullptr, *lnpre_b = nullptr,
          *lnpost_g = nullptr, *lnpost_b = nullptr, *head_w = nullptr, *head_b = nullptr, *hconv_b = nullptr;
    uint16_t *hconv_w = nullptr;  // SSCD head conv weight
    // One workspace per lane.  With two lanes, consecutive max_batch chunks of a forward call run
    // on two internal streams: the HBM-bound kernels of one chunk (LayerNorm, residual write-out)
    // co-run with the MFMA-bound GEMMs of the other instead of leaving the matrix pipes idle.
    struct Workspace {
        uint16_t *patches = nullptr, *y = nullptr, *qkv = nullptr, *h = nullptr, *hconv_out = nullptr;
        float *x = nullptr, *pooled = nullptr;
        float *stats = nullptr, *rowstats = nullptr;  // LayerNorm folding: [D/64][M][2] slice partials, [M][2] (mean, rstd)
        uint16_t *xb = nullptr;                       //                    bf16(x) [M, D]
        // LayerNorm as the tail of the residual GEMMs (gemm_bf16.hip, RESADD_LN): proj's A operand is y, so its tail writes LN2 to a
        // buffer of its own; the counters / claim words of the lane's launches (zeroed here once, zero again behind every launch)
        uint16_t *yln = nullptr;
        unsigned *tail_ws = nullptr;
    } ws[2];
    int lanes = 1;
    int64_t ws_bytes = 0;
};
static_assert(VSC_PROF_CLASSES <= ModelHost::MAX_CLASSES, "profile classes");

namespace {

// round-to-nearest-even f32 -> operand type -> f32, as the device packing / launch_f32_to_bf16 do
inline float bf16_round(float v) { return lp_to_f32(f32_to_lp(v)); }

// LayerNorm folded into the Linear that consumes it:  Linear(LN(x)) = rstd * (x W'^T - mu * colsum) + bias'
// with W' = gamma o W.  The GEMM then reads bf16(x) itself; colsum is taken over the bf16-rounded W' the MFMA
// sees, so (acc - mu * colsum) is exactly sum_k (bf16(x_k) - mu) W'_nk.
int fold_ln(vsc_encoder *e, const std::string &wname, const std::string &bname, const std::string &gname,
            const std::string &betaname, int n, int k, uint16_t **wf, float **cs, float **bf) {
    const std::vector<float> &W = e->host_w.at(wname), &b = e->host_w.at(bname), &g = e->host_w.at(gname),
                             &beta = e->host_w.at(betaname);
    std::vector<float> &Wf = e->host_w[wname + ".folded"];
    std::vector<float> &colsum = e->host_w[wname + ".colsum"], &biasf = e->host_w[bname + ".folded"];
    Wf.resize((size_t)n * k);
    colsum.resize(n);
    biasf.resize(n);
    for (int r = 0; r < n; ++r) {
        double s = 0.0, t = 0.0;
        for (int c = 0; c < k; ++c) {
            const float v = g[c] * W[(size_t)r * k + c];
            Wf[(size_t)r * k + c] = v;
            s += (double)bf16_round(v);
            t += (double)beta[c] * (double)W[(size_t)r * k + c];
        }
        colsum[r] = (float)s;
        biasf[r] = (float)((double)b[r] + t);
    }
    VSC_TRY(e->upload_bf16(wname + ".folded", n, k, k, wf));
    VSC_TRY(e->upload_f32(wname + ".colsum", cs));
    return e->upload_f32(bname + ".folded", bf);
}

}  // namespace

extern "C" int vsc_encoder_create(const vsc_encoder_config *cfg, vsc_encoder **out) {
    VSC_REQUIRE(cfg && out, "encoder_create: null argument");
    const vsc_encoder_config &c = *cfg;
    VSC_REQUIRE(c.image_size > 0 && c.patch_size > 0 && c.image_size % c.patch_size == 0,
                "encoder: image %d / patch %d", c.image_size, c.patch_size);
    VSC_REQUIRE(c.image_size % 4 == 0, "encoder: image size must be a multiple of 4");
    VSC_REQUIRE(c.channels >= 1, "encoder: channels");
    VSC_REQUIRE(c.width % 64 == 0 && c.heads > 0 && c.width == c.heads * 64,
                "encoder: width %d with %d heads -- only head_dim 64 is supported", c.width, c.heads);
    VSC_REQUIRE(c.width <= 2048, "encoder: width %d > 2048", c.width);
    VSC_REQUIRE(c.mlp_dim % 64 == 0 && c.mlp_dim > 0, "encoder: mlp_dim %d", c.mlp_dim);
    VSC_REQUIRE(c.layers >= 1, "encoder: layers");
    VSC_REQUIRE(c.out_dim >= 0 && c.out_dim <= 2048, "encoder: out_dim %d", c.out_dim);
    VSC_REQUIRE(c.act == 0 || c.act == 1, "encoder: act %d", c.act);
    VSC_REQUIRE(c.pool == 0 || c.pool == 1, "encoder: pool %d", c.pool);
    VSC_REQUIRE(c.max_batch >= 1, "encoder: max_batch");
    VSC_REQUIRE(c.head_conv_dim >= 0 && c.head_conv_dim <= 2048 && c.head_conv_dim % 8 == 0,
                "encoder: head_conv_dim %d", c.head_conv_dim);
    VSC_REQUIRE(!c.head_conv_dim || (c.pool == 0 && c.out_dim > 0),
                "encoder: the SSCD head needs GeM pooling and a Linear output");
    int g = c.image_size / c.patch_size;
    int tokens = g * g + 1;
    // up to 320 tokens attention.hip (a whole score row in registers), above that attention_stream.hip (key blocks)
    VSC_REQUIRE(tokens <= VSC_ATTENTION_STREAM_MAX_TOKENS, "encoder: %d tokens > %d (attention kernel limit)", tokens,
                VSC_ATTENTION_STREAM_MAX_TOKENS);

    vsc_encoder *e = new vsc_encoder();
    e->cfg = c;
    e->grid = g;
    e->tokens = tokens;
    e->kpatch = c.channels * c.patch_size * c.patch_size;
    e->kpad = (e->kpatch + 63) / 64 * 64;
    e->desc_dim = c.out_dim ? c.out_dim : c.width;
    const size_t D = c.width, Mlp = c.mlp_dim;
    e->expect("patch.weight", D * e->kpatch);
    if (c.patch_bias) e->expect("patch.bias", D);
    e->expect("cls", D);
    e->expect("pos", (size_t)tokens * D);
    if (c.pre_ln) {
        e->expect("ln_pre.weight", D);
        e->expect("ln_pre.bias", D);
    }
    for (int i = 0; i < c.layers; ++i) {
        const std::string b = "blocks." + std::to_string(i) + ".";
        e->expect(b + "ln1.weight", D);
        e->expect(b + "ln1.bias", D);
        e->expect(b + "ln2.weight", D);
        e->expect(b + "ln2.bias", D);
        e->expect(b + "qkv.weight", 3 * D * D);
        e->expect(b + "qkv.bias", 3 * D);
        e->expect(b + "proj.weight", D * D);
        e->expect(b + "proj.bias", D);
        e->expect(b + "fc1.weight", Mlp * D);
        e->expect(b + "fc1.bias", Mlp);
        e->expect(b + "fc2.weight", D * Mlp);
        e->expect(b + "fc2.bias", D);
    }
    e->expect("ln_post.weight", D);
    e->expect("ln_post.bias", D);
    if (c.head_conv_dim) {
        e->expect("head_conv.weight", (size_t)c.head_conv_dim * D);
        e->expect("head_conv.bias", c.head_conv_dim);
    }
    if (c.out_dim) {
        e->expect("head.weight", (size_t)c.out_dim * (c.head_conv_dim ? c.head_conv_dim : D));
        e->expect("head.bias", c.out_dim);
    }
    *out = e;
    return VSC_OK;
}

extern "C" void vsc_encoder_destroy(vsc_encoder *e) { delete e; }

extern "C" int vsc_encoder_set_weight(vsc_encoder *e, const char *name, const float *host,
                                      size_t count) {
    VSC_REQUIRE(e && name && host, "set_weight: null argument");
    return e->set_weight(name, host, count);
}

extern "C" int vsc_encoder_finalize(vsc_encoder *e) {
    VSC_REQUIRE(e, "finalize: null encoder");
    if (e->finalized) return VSC_OK;
    VSC_TRY(e->all_set());
    const vsc_encoder_config &c = e->cfg;
    const int D = c.width;
    VSC_TRY(e->upload_bf16("patch.weight", D, e->kpatch, e->kpad, &e->patch_w));
    if (c.patch_bias) VSC_TRY(e->upload_f32("patch.bias", &e->patch_b));
    VSC_TRY(e->upload_f32("cls", &e->cls));
    VSC_TRY(e->upload_f32("pos", &e->pos));
    if (c.pre_ln) {
        VSC_TRY(e->upload_f32("ln_pre.weight", &e->lnpre_g));
        VSC_TRY(e->upload_f32("ln_pre.bias", &e->lnpre_b));
    }
    e->layers.resize(c.layers);
    for (int i = 0; i < c.layers; ++i) {
        const std::string b = "blocks." + std::to_string(i) + ".";
        LayerW &L = e->layers[i];
        VSC_TRY(e->upload_f32(b + "ln1.weight", &L.ln1_g));
        VSC_TRY(e->upload_f32(b + "ln1.bias", &L.ln1_b));
        VSC_TRY(e->upload_f32(b + "ln2.weight", &L.ln2_g));
        VSC_TRY(e->upload_f32(b + "ln2.bias", &L.ln2_b));
        VSC_TRY(e->upload_bf16(b + "qkv.weight", 3 * D, D, D, &L.qkv_w));
        VSC_TRY(e->upload_f32(b + "qkv.bias", &L.qkv_b));
        VSC_TRY(e->upload_bf16(b + "proj.weight", D, D, D, &L.proj_w));
        VSC_TRY(e->upload_f32(b + "proj.bias", &L.proj_b));
        VSC_TRY(e->upload_bf16(b + "fc1.weight", c.mlp_dim, D, D, &L.fc1_w));
        VSC_TRY(e->upload_f32(b + "fc1.bias", &L.fc1_b));
        VSC_TRY(e->upload_bf16(b + "fc2.weight", D, c.mlp_dim, c.mlp_dim, &L.fc2_w));
        VSC_TRY(e->upload_f32(b + "fc2.bias", &L.fc2_b));
        if (c.fuse_ln > 0) {
            VSC_TRY(fold_ln(e, b + "fc1.weight", b + "fc1.bias", b + "ln2.weight", b + "ln2.bias", c.mlp_dim, D, &L.fc1_wf,
                            &L.fc1_cs, &L.fc1_bf));
            if (i > 0)  // layer 0 reads x from the patch / cls kernels, which emit no statistics: it keeps its LN1 pass
                VSC_TRY(fold_ln(e, b + "qkv.weight", b + "qkv.bias", b + "ln1.weight", b + "ln1.bias", 3 * D, D, &L.qkv_wf,
                                &L.qkv_cs, &L.qkv_bf));
        }
    }
    VSC_TRY(e->upload_f32("ln_post.weight", &e->lnpost_g));
    VSC_TRY(e->upload_f32("ln_post.bias", &e->lnpost_b));
    if (c.head_conv_dim) {
        VSC_TRY(e->upload_bf16("head_conv.weight", c.head_conv_dim, D, D, &e->hconv_w));
        VSC_TRY(e->upload_f32("head_conv.bias", &e->hconv_b));
    }
    if (c.out_dim) {
        VSC_TRY(e->upload_f32("head.weight", &e->head_w));
        VSC_TRY(e->upload_f32("head.bias", &e->head_b));
    }
    // workspace for max_batch frames
    const size_t B = c.max_batch, M = B * e->tokens;
    const size_t sz_patches = B * (e->tokens - 1) * e->kpad * 2, sz_x = M * D * 4, sz_y = M * D * 2,
                 sz_qkv = M * 3 * D * 2, sz_h = M * (size_t)c.mlp_dim * 2,
                 sz_pool = B * (size_t)(c.head_conv_dim ? c.head_conv_dim : D) * 4;
    VSC_REQUIRE(c.head_conv_dim <= c.mlp_dim, "encoder: head_conv_dim %d > mlp_dim %d", c.head_conv_dim, c.mlp_dim);
    e->lanes = c.lanes == 2 ? 2 : 1;
    // the LayerNorm-tail form of the residual GEMMs (opt-in): its buffers exist when the switch is on HERE; after that it is read per launch
    const bool ln_tail = c.fuse_ln <= 0 && vsc_opt_is(OPT_GEMM_LN_TAIL, '1');
    for (int l = 0; l < e->lanes; ++l) {
        vsc_encoder::Workspace &w = e->ws[l];
        VSC_TRY(e->alloc(sz_patches, (void **)&w.patches));
        VSC_TRY(e->alloc(sz_x, (void **)&w.x));
        VSC_TRY(e->alloc(sz_y, (void **)&w.y));
        VSC_TRY(e->alloc(sz_qkv, (void **)&w.qkv));
        VSC_TRY(e->alloc(sz_h, (void **)&w.h));
        VSC_TRY(e->alloc(sz_pool, (void **)&w.pooled));
        if (c.fuse_ln > 0) {
            VSC_TRY(e->alloc((size_t)(D / 64) * M * 2 * 4, (void **)&w.stats));
            VSC_TRY(e->alloc(M * 2 * 4, (void **)&w.rowstats));
            VSC_TRY(e->alloc(sz_y, (void **)&w.xb));
        }
        if (ln_tail) {
            VSC_TRY(e->alloc(sz_y, (void **)&w.yln));
            VSC_TRY(e->alloc(gemm_ln_tail_ws_bytes((int64_t)M), (void **)&w.tail_ws));
            VSC_CHECK_HIP(hipMemset(w.tail_ws, 0, gemm_ln_tail_ws_bytes((int64_t)M)));
        }
        w.hconv_out = w.h;  // [M, head_conv_dim] bf16 fits in the (idle) MLP buffer: head_conv_dim <= mlp_dim
    }
    if (e->lanes == 2) VSC_TRY(e->make_lanes());
    e->ws_bytes = (int64_t)(sz_patches + sz_x + sz_y + sz_qkv + sz_h + sz_pool + (c.fuse_ln > 0 ? sz_y + ((size_t)(D / 64) + 1) * M * 8 : ln_tail ? sz_y + gemm_ln_tail_ws_bytes((int64_t)M) : 0)) * e->lanes;
    e->drop_host();
    return VSC_OK;
}

extern "C" int64_t vsc_encoder_workspace_bytes(const vsc_encoder *e) { return e ? e->ws_bytes : 0; }

// the chunks of one call; `fork`: alternate them over the two lanes.  Returns at the first failing launch (the caller joins
// the lanes in every case).
static int encoder_run_chunks(vsc_encoder *e, const float *frames, const uint8_t *frames_u8, const float *mean, const float *std,
                              int64_t n, float *desc, float *tokens_out, hipStream_t user, bool fork) {
    const vsc_encoder_config &c = e->cfg;
    const int D = c.width, T = e->tokens;
    const int act_epi = c.act == 0 ? VSC_EPI_GELU_BF16 : VSC_EPI_QGELU_BF16;
    const int64_t frame_elems = (int64_t)c.channels * c.image_size * c.image_size;
    const bool attn_long = T > 320 || vsc_opt_is(OPT_ATTN_LONG, '1');
    int chunk = 0;
    for (int64_t off = 0; off < n; off += c.max_batch, ++chunk) {
        const int lane = fork ? (chunk & 1) : 0;
        hipStream_t st = fork ? e->lane_stream[lane] : user;
        vsc_encoder::Workspace &w = e->ws[lane];
        const int64_t B = (n - off) < c.max_batch ? (n - off) : c.max_batch;
        const int64_t M = B * T, Mp = B * (T - 1);
        {
            ProfScope _ps(e, VSC_PROF_PATCHIFY, st);
            if (frames)
                VSC_TRY(launch_patchify(frames + off * frame_elems, w.patches, B, c.channels, c.image_size, c.patch_size, e->kpad, st));
            else
                VSC_TRY(launch_patchify_u8(frames_u8 + off * frame_elems, w.patches, B, c.channels, c.image_size, c.patch_size,
                                           e->kpad, mean, std, st));
        }
        { ProfScope _ps(e, VSC_PROF_GEMM_PATCH, st); VSC_TRY(launch_gemm_bf16(w.patches, e->patch_w, e->patch_b, e->pos, w.x, Mp, D, e->kpad,
                                 VSC_EPI_PATCH_F32, T, st)); }
        { ProfScope _ps(e, VSC_PROF_MISC, st); VSC_TRY(launch_cls_rows(w.x, e->cls, e->pos, B, T, D, st)); }
        if (c.pre_ln) {
            ProfScope _ps(e, VSC_PROF_LAYERNORM, st);
            VSC_TRY(launch_layernorm(w.x, e->lnpre_g, e->lnpre_b, w.x, M, D, c.ln_eps, 1, st));
        }
        // LayerNorm folding (opt-in): from the first residual GEMM on, bf16(x) and x's row statistics
        // come out of the proj / fc2 write-out (into w.xb / w.stats) and LN2 / the next layer's LN1 are applied inside
        // the fc1 / qkv epilogues -- no LN pass.  Layer 0's LN1 stays (x comes from the patch / cls kernels).
        // Measured on the power-limited MI355X it costs +14 ... +23 us on each of the four GEMMs for the LayerNorm launches it
        // removes: neutral to +1.1 % on two lanes, and it changes bits -- so it stays opt-in.
        //
        // A second opt-in (VSC_GEMM_LN_TAIL=1 from finalize on) runs LN2 / the next layer's LN1 as a TAIL of the proj /
        // fc2 launch wherever the persistent kernel has that form (gemm_resadd_ln_tail_eligible): same arithmetic, same bits, no
        // launch -- and, as measured, no gain either.  y_ready: the previous fc2 launch has already written this layer's LN1
        // output to w.y.
        const bool fold = c.fuse_ln > 0;
        const int act_lnf = c.act == 0 ? VSC_EPI_LNF_GELU_BF16 : VSC_EPI_LNF_QGELU_BF16;
        GemmExtra emit, take;
        emit.xb = w.xb;
        emit.stats = w.stats;
        take.rowstats = w.rowstats;   // scratch: where the GEMM launcher merges the partials when its kernel cannot (launch_v34)
        take.slices = w.stats;
        take.nslices = D / 64;
        take.eps = c.ln_eps;
        const bool tail_proj = !fold && w.yln && gemm_resadd_ln_tail_eligible(M, D, D);
        const bool tail_fc2 = !fold && w.yln && gemm_resadd_ln_tail_eligible(M, D, c.mlp_dim);
        bool y_ready = false;
        for (int l = 0; l < c.layers; ++l) {
            const LayerW &L = e->layers[l];
            if (fold && l > 0) {
                take.colsum = L.qkv_cs;
                ProfScope _ps(e, VSC_PROF_GEMM_QKV, st);
                VSC_TRY(launch_gemm_bf16_ex(w.xb, L.qkv_wf, L.qkv_bf, nullptr, w.qkv, M, 3 * D, D, VSC_EPI_LNF_BF16, 0, take, st));
            } else {
                if (!y_ready) { ProfScope _ps(e, VSC_PROF_LAYERNORM, st); VSC_TRY(launch_layernorm(w.x, L.ln1_g, L.ln1_b, w.y, M, D, c.ln_eps, 0, st)); }
                { ProfScope _ps(e, VSC_PROF_GEMM_QKV, st); VSC_TRY(launch_gemm_bf16(w.y, L.qkv_w, L.qkv_b, nullptr, w.qkv, M, 3 * D, D, VSC_EPI_BF16, 0, st)); }
            }
            {   // the register-row kernel wherever it applies (<= 320 tokens); the streaming kernel above that, or everywhere with VSC_ATTN_LONG=1
                ProfScope _ps(e, VSC_PROF_ATTENTION, st);
                if (attn_long) VSC_TRY(launch_attention_stream_bf16(w.qkv, w.y, (int)B, T, c.heads, st));
                else VSC_TRY(launch_attention_bf16(w.qkv, w.y, (int)B, T, c.heads, st));
            }
            if (fold) {
                { ProfScope _ps(e, VSC_PROF_GEMM_PROJ, st); VSC_TRY(launch_gemm_bf16_ex(w.y, L.proj_w, L.proj_b, w.x, w.x, M, D, D, VSC_EPI_RESADD_STATS_F32, 0, emit, st)); }
                take.colsum = L.fc1_cs;
                { ProfScope _ps(e, VSC_PROF_GEMM_FC1, st); VSC_TRY(launch_gemm_bf16_ex(w.xb, L.fc1_wf, L.fc1_bf, nullptr, w.h, M, c.mlp_dim, D, act_lnf, 0, take, st)); }
                { ProfScope _ps(e, VSC_PROF_GEMM_FC2, st); VSC_TRY(launch_gemm_bf16_ex(w.h, L.fc2_w, L.fc2_b, w.x, w.x, M, D, c.mlp_dim, l + 1 < c.layers ? VSC_EPI_RESADD_STATS_F32 : VSC_EPI_RESADD_F32, 0, emit, st)); }
            } else {
                const uint16_t *ln2 = w.y;
                if (tail_proj) {
                    ProfScope _ps(e, VSC_PROF_GEMM_PROJ, st);
                    VSC_TRY(launch_gemm_resadd_ln_bf16(w.y, L.proj_w, L.proj_b, w.x, L.ln2_g, L.ln2_b, w.yln, M, D, D, c.ln_eps, w.tail_ws, st));
                    ln2 = w.yln;
                } else {
                    { ProfScope _ps(e, VSC_PROF_GEMM_PROJ, st); VSC_TRY(launch_gemm_bf16(w.y, L.proj_w, L.proj_b, w.x, w.x, M, D, D, VSC_EPI_RESADD_F32, 0, st)); }
                    { ProfScope _ps(e, VSC_PROF_LAYERNORM, st); VSC_TRY(launch_layernorm(w.x, L.ln2_g, L.ln2_b, w.y, M, D, c.ln_eps, 0, st)); }
                }
                { ProfScope _ps(e, VSC_PROF_GEMM_FC1, st); VSC_TRY(launch_gemm_bf16(ln2, L.fc1_w, L.fc1_b, nullptr, w.h, M, c.mlp_dim, D, act_epi, 0, st)); }
                y_ready = tail_fc2 && l + 1 < c.layers;
                if (y_ready) {   // the next layer's LN1 rides on this launch (the last layer keeps the plain epilogue: ln_post is the pooling kernel's)
                    const LayerW &N = e->layers[l + 1];
                    ProfScope _ps(e, VSC_PROF_GEMM_FC2, st);
                    VSC_TRY(launch_gemm_resadd_ln_bf16(w.h, L.fc2_w, L.fc2_b, w.x, N.ln1_g, N.ln1_b, w.y, M, D, c.mlp_dim, c.ln_eps, w.tail_ws, st));
                } else {
                    ProfScope _ps(e, VSC_PROF_GEMM_FC2, st);
                    VSC_TRY(launch_gemm_bf16(w.h, L.fc2_w, L.fc2_b, w.x, w.x, M, D, c.mlp_dim, VSC_EPI_RESADD_F32, 0, st));
                }
            }
        }
        if (c.head_conv_dim) {
            // SSCD head: final LN -> bf16 tokens -> Conv1d(D, C, 1) as a GEMM -> GeM over tokens
            ProfScope _ps(e, VSC_PROF_POOL_HEAD, st);
            if (tokens_out)
                VSC_TRY(launch_layernorm(w.x, e->lnpost_g, e->lnpost_b, tokens_out + off * T * D, M, D, c.ln_eps, 1, st));
            VSC_TRY(launch_layernorm(w.x, e->lnpost_g, e->lnpost_b, w.y, M, D, c.ln_eps, 0, st));
            VSC_TRY(launch_gemm_bf16(w.y, e->hconv_w, e->hconv_b, nullptr, w.hconv_out, M, c.head_conv_dim, D,
                                     VSC_EPI_BF16, 0, st));
            VSC_TRY(launch_gem_pool_bf16(w.hconv_out, w.pooled, B, T, c.head_conv_dim, c.gem_p, st));
            VSC_TRY(launch_head(w.pooled, e->head_w, e->head_b, desc + off * e->desc_dim, B, c.head_conv_dim,
                                c.out_dim, c.l2_normalize, st));
        } else {
        { ProfScope _ps(e, VSC_PROF_POOL_HEAD, st); VSC_TRY(launch_ln_pool(w.x, e->lnpost_g, e->lnpost_b, w.pooled,
                               tokens_out ? tokens_out + off * T * D : nullptr, B, T, D, c.ln_eps, c.pool,
                               c.gem_p, st)); }
            { ProfScope _ps(e, VSC_PROF_POOL_HEAD, st); VSC_TRY(launch_head(w.pooled, e->head_w, e->head_b, desc + off * e->desc_dim, B, D, c.out_dim,
                            c.l2_normalize, st)); }
        }
    }
    return VSC_OK;
}

// frames: fp32 [n,C,H,W] already normalised, or (frames == nullptr) frames_u8: uint8 [n,H,W,C] + mean/std
static int encoder_forward_impl(vsc_encoder *e, const float *frames, const uint8_t *frames_u8, const float *mean,
                                const float *std, int64_t n, float *desc, float *tokens_out, void *stream_) {
    VSC_REQUIRE(e && (frames || frames_u8) && desc, "forward: null argument");
    VSC_REQUIRE(n >= 0, "forward: negative frame count");
    VSC_TRY(e->forward_ready());
    hipStream_t user = (hipStream_t)stream_;
    // >= 2 chunks: alternate them over the two lanes.  Not while profiling: the per-launch events are meant to time one kernel
    // at a time (bench.py's kernels{} / roofline loop), so the chunks then run back to back on the caller's stream.
    const bool fork = e->lanes == 2 && n > e->cfg.max_batch && !e->profile;
    if (fork) VSC_TRY(e->fork(user));
    const int rc = encoder_run_chunks(e, frames, frames_u8, mean, std, n, desc, tokens_out, user, fork);
    return fork ? e->join(user, rc) : rc;
}

extern "C" int vsc_encoder_forward_debug(vsc_encoder *e, const float *frames, int64_t n, float *desc,
                                         float *tokens_out, void *stream) {
    VSC_REQUIRE(frames, "forward: null frames");
    VSC_REQUIRE_ALIGNED("forward", frames, 16);       // the patch gather reads eight pixels of a row as two float4
    VSC_REQUIRE_ALIGNED("forward", tokens_out, 16);   // the final LayerNorm stores the hidden state as float4
    return encoder_forward_impl(e, frames, nullptr, nullptr, nullptr, n, desc, tokens_out, stream);
}

extern "C" int vsc_encoder_forward(vsc_encoder *e, const float *frames, int64_t n, float *desc,
                                   void *stream) {
    return vsc_encoder_forward_debug(e, frames, n, desc, nullptr, stream);
}

extern "C" int vsc_encoder_forward_u8(vsc_encoder *e, const uint8_t *frames_u8, int64_t n, const float *mean,
                                      const float *std, float *desc, void *stream) {
    VSC_REQUIRE(frames_u8 && mean && std, "forward_u8: null argument");
    return encoder_forward_impl(e, nullptr, frames_u8, mean, std, n, desc, nullptr, stream);
}

extern "C" int vsc_encoder_set_profiling(vsc_encoder *e, int32_t on) {
    VSC_REQUIRE(e, "set_profiling: null encoder");
    e->reset(on != 0);
    return VSC_OK;
}

extern "C" int vsc_encoder_get_profile(vsc_encoder *e, double *ms_out, int64_t *launches_out) {
    VSC_REQUIRE(e && ms_out && launches_out, "get_profile: null argument");
    return e->collect(ms_out, launches_out, VSC_PROF_CLASSES);
}
