// Score normalisation on the device (VSC22-Descriptor-Track-1st/infer/vsc/baseline/score_normalization.py:74-76, 84-88, 95-105,
// 141-150; infer/src/utils.py:2-5).  The contract is stated with vsc_column_var_f32 / vsc_score_norm_rows_f32 /
// vsc_score_norm_bias_f32 in include/vsc_hip.h (executable form: tests/score_norm_contract.py): the descriptors written through
// these kernels are the bytes the numpy path writes, so the order of every rounding below is fixed.
//  (a) cv_kernel: numpy's var(axis=0) of a C-contiguous [n, d] array is, per column, ONE chain over the rows -- a latency problem
//      (one dependent add per row), fed by a bandwidth problem (every row is read twice).  One workgroup per 64 columns: all four
//      waves stage tiles of 64 rows into LDS (two buffers: the loads of tile t + 1 are in flight while tile t is summed), lane c of
//      wave 0 carries column c's chain and reads 16 rows into registers before its 16 dependent adds.  Pass 1 sums, the lane forms
//      the mean, pass 2 sums the centred squares; both in one launch.
//  (b) rows_kernel: one wave per row as l2_normalize_kernel (elementwise.hip), over the logical columns of the narrowed row, into
//      a second buffer.
//  (c) bias_kernel: one thread per row of the [nq, nk] nearest-noise scores, numpy's pairwise row sum for nk <= 128.
// All only enqueue on the caller's stream.  No 16-bit operands: one object for both builds of the library.
#include "common.h"

// contract arithmetic: every difference, product and sum rounded on its own; the one fused operation is written as fmaf
#pragma clang fp contract(off)

namespace {

constexpr int CV_COLS = 64;                   // columns per workgroup = chains per carrying wave
constexpr int CV_TILE = 64;                   // rows per LDS tile (VSC_COLUMN_VAR_TILE): 64 x 64 x 4 bytes = 16 KiB, two of them
constexpr int CV_BLOCK = 256;
constexpr int CV_PER_THREAD = CV_TILE * CV_COLS / CV_BLOCK;
constexpr int CV_BATCH = 16;                  // rows in registers before the dependent adds
constexpr int SN_BLOCK = 256;
constexpr int SN_MAX_NK = 128;                // numpy's pairwise blocksize: beyond it the row sum recurses

static_assert(CV_TILE == VSC_COLUMN_VAR_TILE, "the header states the tile the tests probe");

struct CvArgs {
    const float *x;
    float *var;
    long long n, ld;
    int d;
};

struct RowsArgs {
    const float *x, *last;
    float *out;
    long long n, ldx, ldo;
    int d, drop, normalize, append;
};

struct BiasArgs {
    const float *topk;
    const unsigned char *gate;
    float *bias;
    long long nq, ldk;
    int nk;
    float neg_beta;
};

// rows r0 .. r0 + 63 of the workgroup's 64 columns: thread (w, c) holds rows w, w + 4, ...; nothing outside [0, n) x [0, d) is read
__device__ inline void cv_fetch(const CvArgs &a, long long r0, int c, int w, float (&reg)[CV_PER_THREAD]) {
#pragma unroll
    for (int i = 0; i < CV_PER_THREAD; ++i) {
        const long long r = r0 + w + 4 * i;
        reg[i] = (c < a.d && r < a.n) ? a.x[r * a.ld + c] : 0.f;
    }
}

__device__ inline void cv_stash(float *tile, int col, int w, const float (&reg)[CV_PER_THREAD]) {
#pragma unroll
    for (int i = 0; i < CV_PER_THREAD; ++i) tile[(w + 4 * i) * CV_COLS + col] = reg[i];
}

// One pass over all rows.  Wave 0, lane c: -0.0f + v[0] + v[1] + ... in ascending row order with v = x (CENTRED: fl(fl(x - mean) *
// fl(x - mean))); -0.0f + v is v for every v, so the chain starts from the first row as numpy's does.  Ends behind a barrier: the
// tiles are free again.
template <bool CENTRED>
__device__ inline float cv_pass(const CvArgs &a, float *tiles, float mean) {
    const int tid = threadIdx.x, col = tid & 63, w = tid >> 6;
    const int c = (int)blockIdx.x * CV_COLS + col;
    const long long n_tiles = (a.n + CV_TILE - 1) / CV_TILE;
    float reg[CV_PER_THREAD];
    float acc = -0.0f;
    cv_fetch(a, 0, c, w, reg);
    cv_stash(tiles, col, w, reg);
    __syncthreads();
    for (long long t = 0; t < n_tiles; ++t) {
        const bool more = t + 1 < n_tiles;
        if (more) cv_fetch(a, (t + 1) * CV_TILE, c, w, reg);          // in flight while wave 0 sums tile t
        if (tid < CV_COLS) {
            const float *cur = tiles + (t & 1) * (CV_TILE * CV_COLS);
            const long long left = a.n - t * CV_TILE;
            if (left >= CV_TILE) {
                for (int b = 0; b < CV_TILE; b += CV_BATCH) {
                    float v[CV_BATCH];
#pragma unroll
                    for (int j = 0; j < CV_BATCH; ++j) v[j] = cur[(b + j) * CV_COLS + tid];
                    if (CENTRED) {
#pragma unroll
                        for (int j = 0; j < CV_BATCH; ++j) {
                            const float dl = v[j] - mean;
                            v[j] = dl * dl;
                        }
                    }
#pragma unroll
                    for (int j = 0; j < CV_BATCH; ++j) acc = acc + v[j];
                }
            } else {
                for (int r = 0; r < (int)left; ++r) {
                    float v = cur[r * CV_COLS + tid];
                    if (CENTRED) {
                        const float dl = v - mean;
                        v = dl * dl;
                    }
                    acc = acc + v;
                }
            }
        }
        if (more) cv_stash(tiles + ((t + 1) & 1) * (CV_TILE * CV_COLS), col, w, reg);
        __syncthreads();
    }
    return acc;
}

__global__ __launch_bounds__(CV_BLOCK) void cv_kernel(CvArgs a) {
    __shared__ float tiles[2 * CV_TILE * CV_COLS];
    const float s = cv_pass<false>(a, tiles, 0.f);
    const float mean = (float)((double)s / (double)a.n);
    const float acc = cv_pass<true>(a, tiles, mean);
    const int c = (int)blockIdx.x * CV_COLS + (int)threadIdx.x;
    if (threadIdx.x < CV_COLS && c < a.d) a.var[c] = (float)((double)acc / (double)a.n);
}

__device__ inline float sn_wave_sum(float v) {                       // common.h's wave_sum: the xor butterfly 32 ... 1
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(SN_BLOCK) void rows_kernel(RowsArgs a) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.n) return;
    const float *xr = a.x + row * a.ldx;
    float *o = a.out + row * a.ldo;
    const bool narrowed = a.drop >= 0;
    const int w = a.d - (narrowed ? 1 : 0);                          // logical column c' < w is column c' + (c' >= drop) of x
    float nrm = 0.f;
    if (a.normalize) {
        float ss = 0.f;
        for (int c = lane; c < w; c += 64) {
            const float v = xr[c + (narrowed && c >= a.drop ? 1 : 0)];
            ss = fmaf(v, v, ss);                                     // l2_normalize_kernel's `ss += x * x` is one v_fmac_f32 on gfx950
        }
        nrm = sqrtf(sn_wave_sum(ss));
    }
    for (int c = lane; c < w; c += 64) {
        const float v = xr[c + (narrowed && c >= a.drop ? 1 : 0)];
        o[c] = nrm == 0.f ? v : v / nrm;                             // a row whose squares sum to zero stays as it is
    }
    if (lane == 0 && a.append) o[w] = a.append == 2 ? a.last[row] : 1.0f;
}

__global__ __launch_bounds__(SN_BLOCK) void bias_kernel(BiasArgs a) {
    const long long row = (long long)blockIdx.x * SN_BLOCK + threadIdx.x;
    if (row >= a.nq) return;
    if (a.gate && a.gate[row]) {
        a.bias[row] = -100.0f;
        return;
    }
    const float *s = a.topk + row * a.ldk;
    const int nk = a.nk;
    float res;
    if (nk < 8) {
        res = s[0];
        for (int i = 1; i < nk; ++i) res = res + s[i];
    } else {
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = s[j];
        int i = 8;
        for (; i < nk - nk % 8; i += 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] = r[j] + s[i + j];
        }
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < nk; ++i) res = res + s[i];
    }
    const float mean = (float)((double)res / (double)nk);
    a.bias[row] = a.neg_beta * mean;
}

}  // namespace

int launch_column_var(const float *x, int64_t n, int d, int64_t ld, float *var, hipStream_t stream) {
    VSC_REQUIRE(n >= 1, "column_var: %lld rows (the variance of no rows is refused)", (long long)n);
    VSC_REQUIRE(d >= 1 && ld >= d, "column_var: %d columns with a row stride of %lld", d, (long long)ld);
    VSC_REQUIRE(x && var, "column_var: null pointer");
    CvArgs a;
    a.x = x, a.var = var, a.n = n, a.ld = ld, a.d = d;
    hipLaunchKernelGGL(cv_kernel, dim3((unsigned)((d + CV_COLS - 1) / CV_COLS)), dim3(CV_BLOCK), 0, stream, a);
    VSC_CHECK_LAUNCH();
    return VSC_OK;
}

int launch_score_norm_rows(const float *x, int64_t n, int d, int64_t ldx, int drop, int normalize, int append, const float *last,
                           float *out, int64_t ldo, hipStream_t stream) {
    VSC_REQUIRE(n >= 0 && n < (1ll << 31), "score_norm_rows: %lld rows (in [0, 2^31))", (long long)n);
    VSC_REQUIRE(d >= 1 && drop >= -1 && drop < d, "score_norm_rows: drop %d of %d columns", drop, d);
    VSC_REQUIRE((normalize == 0 || normalize == 1) && append >= 0 && append <= 2, "score_norm_rows: normalize %d, append %d", normalize, append);
    const int wo = d - (drop >= 0 ? 1 : 0) + (append ? 1 : 0);
    VSC_REQUIRE(ldx >= d && ldo >= wo, "score_norm_rows: row strides %lld / %lld below the widths %d / %d", (long long)ldx, (long long)ldo, d, wo);
    if (n == 0) return VSC_OK;
    VSC_REQUIRE(x && out && (last || append != 2), "score_norm_rows: null pointer");
    const uintptr_t x0 = (uintptr_t)x, x1 = x0 + ((uintptr_t)(n - 1) * (uintptr_t)ldx + (uintptr_t)d) * sizeof(float);
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + ((uintptr_t)(n - 1) * (uintptr_t)ldo + (uintptr_t)wo) * sizeof(float);
    VSC_REQUIRE(x1 <= o0 || o1 <= x0, "score_norm_rows: out overlaps x (the kernel is not an in-place shift)");
    RowsArgs a;
    a.x = x, a.last = last, a.out = out, a.n = n, a.ldx = ldx, a.ldo = ldo, a.d = d, a.drop = drop, a.normalize = normalize, a.append = append;
    hipLaunchKernelGGL(rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(SN_BLOCK), 0, stream, a);
    VSC_CHECK_LAUNCH();
    return VSC_OK;
}

int launch_score_norm_bias(const float *topk, int64_t nq, int64_t ldk, int nk, float neg_beta, const uint8_t *gate, float *bias,
                           hipStream_t stream) {
    VSC_REQUIRE(nq >= 0 && nq < (1ll << 31), "score_norm_bias: %lld rows (in [0, 2^31))", (long long)nq);
    VSC_REQUIRE(nk >= 1 && nk <= SN_MAX_NK, "score_norm_bias: nk %d outside [1, %d]", nk, SN_MAX_NK);
    VSC_REQUIRE(ldk >= nk, "score_norm_bias: row stride %lld below nk %d", (long long)ldk, nk);
    if (nq == 0) return VSC_OK;
    VSC_REQUIRE(topk && bias, "score_norm_bias: null pointer");
    BiasArgs a;
    a.topk = topk, a.gate = gate, a.bias = bias, a.nq = nq, a.ldk = ldk, a.nk = nk, a.neg_beta = neg_beta;
    hipLaunchKernelGGL(bias_kernel, dim3((unsigned)((nq + SN_BLOCK - 1) / SN_BLOCK)), dim3(SN_BLOCK), 0, stream, a);
    VSC_CHECK_LAUNCH();
    return VSC_OK;
}

// the handle is the stream every call of it enqueues on
struct vsc_score_norm {
    hipStream_t stream = nullptr;
};

extern "C" int vsc_score_norm_create(void *stream, vsc_score_norm **out) {
    VSC_REQUIRE(out, "score_norm_create: null pointer");
    *out = new vsc_score_norm{(hipStream_t)stream};
    return VSC_OK;
}

extern "C" void vsc_score_norm_destroy(vsc_score_norm *h) { delete h; }

extern "C" int vsc_column_var_f32(vsc_score_norm *h, const float *x_dev, int64_t n, int32_t d, int64_t ld, float *var_dev) {
    VSC_REQUIRE(h, "column_var: null handle");
    return launch_column_var(x_dev, n, d, ld, var_dev, h->stream);
}

extern "C" int vsc_score_norm_rows_f32(vsc_score_norm *h, const float *x_dev, int64_t n, int32_t d, int64_t ldx, int32_t drop, int32_t normalize,
                                       int32_t append, const float *last_dev, float *out_dev, int64_t ldo) {
    VSC_REQUIRE(h, "score_norm_rows: null handle");
    return launch_score_norm_rows(x_dev, n, d, ldx, drop, normalize, append, last_dev, out_dev, ldo, h->stream);
}

extern "C" int vsc_score_norm_bias_f32(vsc_score_norm *h, const float *topk_dev, int64_t nq, int64_t ldk, int32_t nk, float neg_beta,
                                       const uint8_t *gate_dev, float *bias_dev) {
    VSC_REQUIRE(h, "score_norm_bias: null handle");
    return launch_score_norm_bias(topk_dev, nq, ldk, nk, neg_beta, gate_dev, bias_dev, h->stream);
}
