/* The arithmetic of tests/l2_search_contract.py that needs a true fmaf (TEST INFRASTRUCTURE ONLY).  Built by the contract at test
 * time with the host compiler and -ffp-contract=off: every rounding below is written out. */
#include <math.h>
#include <stdint.h>

/* out[i * nr + j] = the contract's distance of (q_i, r_j): c <- fmaf(t, t, c), t = q_k - r_k, k ascending from c = +0 */
void l2c_dist_matrix(const float *q, int64_t nq, const float *r, int64_t nr, int d, float *out) {
    for (int64_t i = 0; i < nq; ++i)
        for (int64_t j = 0; j < nr; ++j) {
            float c = 0.0f;
            for (int k = 0; k < d; ++k) {
                const float t = q[i * d + k] - r[j * d + k];
                c = fmaf(t, t, c);
            }
            out[i * nr + j] = c;
        }
}

/* out[i] = |x_i|^2 as an ascending fmaf chain (the device sums 64 partial chains: another order, the same bound) */
void l2c_norms(const float *x, int64_t n, int d, float *out) {
    for (int64_t i = 0; i < n; ++i) {
        float c = 0.0f;
        for (int k = 0; k < d; ++k) c = fmaf(x[i * d + k], x[i * d + k], c);
        out[i] = c;
    }
}

/* out[i * nr + j] = the sweep's expanded score <[2q, -1, -|q|^2], [r, |r|^2, 1]> as its ascending fmaf chain of d + 2 terms */
void l2c_expanded_matrix(const float *q, const float *qn, int64_t nq, const float *r, const float *rn, int64_t nr, int d, float *out) {
    for (int64_t i = 0; i < nq; ++i)
        for (int64_t j = 0; j < nr; ++j) {
            float c = 0.0f;
            for (int k = 0; k < d; ++k) c = fmaf(2.0f * q[i * d + k], r[j * d + k], c);
            c = fmaf(-1.0f, rn[j], c);
            c = fmaf(-qn[i], 1.0f, c);
            out[i * nr + j] = c;
        }
}
