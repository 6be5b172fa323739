// What csrc/score_norm.hip needs beyond tests/hip_emu/common.h (which stays as it is), for tests/test_score_norm_emulated.py only:
// the header's tile constant, the launchers' prototypes (csrc/common.h declares them in the library) and the handle and C entry points that
// csrc/capi.hip puts in front of them, which forward their arguments with the handle's stream.
#pragma once
#include "common.h"
#define VSC_COLUMN_VAR_TILE 64
int launch_column_var(const float *x, int64_t n, int d, int64_t ld, float *var, hipStream_t stream);
int launch_score_norm_rows(const float *x, int64_t n, int d, int64_t ldx, int drop, int normalize, int append, const float *last,
                           float *out, int64_t ldo, hipStream_t stream);
int launch_score_norm_bias(const float *topk, int64_t nq, int64_t ldk, int nk, float neg_beta, const uint8_t *gate, float *bias,
                           hipStream_t stream);
struct vsc_score_norm { hipStream_t stream; };
extern "C" int vsc_score_norm_create(void *stream, vsc_score_norm **out) {
    VSC_REQUIRE(out, "score_norm_create: null pointer");
    *out = new vsc_score_norm{(hipStream_t)stream};
    return VSC_OK;
}
extern "C" void vsc_score_norm_destroy(vsc_score_norm *h) { delete h; }
extern "C" int vsc_column_var_f32(vsc_score_norm *h, const float *x, int64_t n, int32_t d, int64_t ld, float *var) {
    VSC_REQUIRE(h, "column_var: null handle");
    return launch_column_var(x, n, d, ld, var, h->stream);
}
extern "C" int vsc_score_norm_rows_f32(vsc_score_norm *h, const float *x, int64_t n, int32_t d, int64_t ldx, int32_t drop, int32_t normalize,
                                       int32_t append, const float *last, float *out, int64_t ldo) {
    VSC_REQUIRE(h, "score_norm_rows: null handle");
    return launch_score_norm_rows(x, n, d, ldx, drop, normalize, append, last, out, ldo, h->stream);
}
extern "C" int vsc_score_norm_bias_f32(vsc_score_norm *h, const float *topk, int64_t nq, int64_t ldk, int32_t nk, float neg_beta,
                                       const uint8_t *gate, float *bias) {
    VSC_REQUIRE(h, "score_norm_bias: null handle");
    return launch_score_norm_bias(topk, nq, ldk, nk, neg_beta, gate, bias, h->stream);
}
