// PCA fit, the n-dependent part (infer/concat_pca_sn.py:42-54, PCA(n_components).fit(train_features)): the raw moments
//     sum[D] = sum_rows x        S2[D, D] = sum_rows x x^T
// of fp32 rows, accumulated in fp64 on the matrix pipe (v_mfma_f64_16x16x4_f64).  The contract is stated with vsc_pca_fit_* in
// include/vsc_hip.h (executable form: tests/pca_contract.py); the D x D eigenproblem is the host's (vsc_hip/pca_fit.py).
//
// X^T X needs no transpose and no packing pass: both MFMA operands are column slabs of the same row-major X.  A K-step is 4 rows,
// lane l holds A[i = l & 15][k = l >> 4] = X[r + (l >> 4)][ci + (l & 15)] and B[k = l >> 4][j = l & 15] = X[r + (l >> 4)][cj + (l & 15)]
// -- the same address pattern for both -- and the f64 C/D map is col = l & 15, row = (l >> 4) + 4 reg (NOT the f32 forms' map).
//
//  (1) pca_s2_kernel: grid = upper-triangular pairs of 128-column tiles x row splits, 4 waves per workgroup, each wave a 64 x 64
//      quarter of the tile pair (4 x 4 MFMA tiles: 16 independent f64 accumulators).  Row slabs of PF_KR rows go through LDS as
//      fp32 (register-staged: the next slab's global loads are in flight while the current one is multiplied) and become fp64 at
//      the fragment read.  Rows past the split's end and columns past D are stored as ZERO (never clamped to the last row: that
//      would add it again).  A 16 x 16 x 4 f64 MFMA keeps the pipe busy far longer than a slab's loads and ds_reads take, so the
//      loads are plain coalesced dwords: any ld >= D, any alignment.  Every (pair, split) writes its 128 x 128 fp64 partial.
//  (2) pca_sum_kernel: column sums in fp64 by column slices x row splits, partials to scratch.
//  (3) pca_fold_kernel: adds the partials of an element IN SPLIT ORDER and folds the total into the handle's running moments
//      (upper triangle of S2 only).  No atomics anywhere: the same calls give the same bits.
//  (4) pca_moments_kernel / pca_cov_kernel mirror the upper triangle on the way out, so the results equal their transposes bit
//      for bit.
#include "common.h"

// the covariance is contract arithmetic: (S2 - n mu mu^T) / (n - 1) with every product and difference rounded on its own
#pragma clang fp contract(off)

namespace {

typedef __attribute__((ext_vector_type(4))) double f64x4_t;

constexpr int PF_T = 128;            // columns per tile
constexpr int PF_KR = 16;            // rows per LDS slab (4 K-steps)
constexpr int PF_LD = PF_T + 16;     // LDS row stride in floats: rows q and q + 1 of a K-step 16 banks apart (ds_read_b32: 32 banks per 32-lane half)
constexpr int PF_BLOCK = 256;
constexpr int PF_PER_THREAD = PF_KR * PF_T / PF_BLOCK;   // staged floats per thread and slab
constexpr int PF_MIN_D = 16, PF_MAX_D = 4096;
constexpr int64_t PF_TILE_ELEMS = (int64_t)PF_T * PF_T;
constexpr int64_t PF_MAX_PARTIAL_TILES = (512ll << 20) / (PF_TILE_ELEMS * 8);   // partials stay under 512 MiB
constexpr int PF_TARGET_BLOCKS = 1024;   // workgroups of (1) asked for (a constant, not the CU count: the split is part of the result's bits)
constexpr int PF_MIN_SPLIT_ROWS = 256;
constexpr int PF_SUM_COLS = 64, PF_SUM_ROWS = 512, PF_SUM_MAX_SPLITS = 256;

// pair index -> (ti, tj), ti <= tj < tiles, pairs numbered row by row
__device__ __host__ inline void pair_tiles(int pair, int tiles, int &ti, int &tj) {
    ti = 0;
    while (pair >= tiles - ti) pair -= tiles - ti, ++ti;
    tj = ti + pair;
}

// one slab of one column tile: rows r .. r + PF_KR of columns c0 .. c0 + 128, zero past r_end / d
__device__ __forceinline__ void slab_load(float (&v)[PF_PER_THREAD], const float *__restrict__ x, int64_t ld, int64_t r, int64_t r_end, int c0, int d,
                                          int tid) {
    const int c = c0 + (tid & (PF_T - 1));
#pragma unroll
    for (int i = 0; i < PF_PER_THREAD; ++i) {
        const int64_t row = r + (tid >> 7) + 2 * i;
        v[i] = (row < r_end && c < d) ? x[row * ld + c] : 0.f;
    }
}
__device__ __forceinline__ void slab_store(const float (&v)[PF_PER_THREAD], float *s, int tid) {
#pragma unroll
    for (int i = 0; i < PF_PER_THREAD; ++i) s[((tid >> 7) + 2 * i) * PF_LD + (tid & (PF_T - 1))] = v[i];
}

__global__ __launch_bounds__(PF_BLOCK) void pca_s2_kernel(const float *__restrict__ x, int64_t n, int64_t ld, int d, int tiles, int64_t rows_per_split,
                                                          double *__restrict__ partial) {
    __shared__ float sa[PF_KR * PF_LD], sb[PF_KR * PF_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;         // the wave's 64 x 64 quarter
    const int l15 = lane & 15, q = lane >> 4;
    int ti, tj;
    pair_tiles(blockIdx.x, tiles, ti, tj);
    const bool diag = ti == tj;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_split;
    const int64_t r1 = r0 + rows_per_split < n ? r0 + rows_per_split : n;
    const float *sbp = diag ? sa : sb;

    f64x4_t acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[m][j] = f64x4_t{0.0, 0.0, 0.0, 0.0};

    float va[PF_PER_THREAD], vb[PF_PER_THREAD];
    slab_load(va, x, ld, r0, r1, ti * PF_T, d, tid);
    if (!diag) slab_load(vb, x, ld, r0, r1, tj * PF_T, d, tid);
    for (int64_t r = r0; r < r1; r += PF_KR) {
        __syncthreads();                       // the previous slab has been read
        slab_store(va, sa, tid);
        if (!diag) slab_store(vb, sb, tid);
        __syncthreads();
        if (r + PF_KR < r1) {
            slab_load(va, x, ld, r + PF_KR, r1, ti * PF_T, d, tid);
            if (!diag) slab_load(vb, x, ld, r + PF_KR, r1, tj * PF_T, d, tid);
        }
#pragma unroll
        for (int kk = 0; kk < PF_KR / 4; ++kk) {
            double a[4], b[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                a[m] = (double)sa[(kk * 4 + q) * PF_LD + wm * 64 + m * 16 + l15];
                b[m] = (double)sbp[(kk * 4 + q) * PF_LD + wn * 64 + m * 16 + l15];
            }
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[m][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[j], acc[m][j], 0, 0, 0);
        }
    }
    // f64 C/D map: col = lane & 15, row = (lane >> 4) + 4 reg
    double *out = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * PF_TILE_ELEMS;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) out[(wm * 64 + m * 16 + q + 4 * g) * PF_T + wn * 64 + j * 16 + l15] = acc[m][j][g];
}

// column sums: 64 columns x 4 row phases per workgroup, the four phases added in order
__global__ __launch_bounds__(PF_BLOCK) void pca_sum_kernel(const float *__restrict__ x, int64_t n, int64_t ld, int d, int64_t rows_per_split,
                                                           double *__restrict__ partial) {
    __shared__ double red[4][PF_SUM_COLS];
    const int tid = threadIdx.x, c = blockIdx.x * PF_SUM_COLS + (tid & (PF_SUM_COLS - 1)), ph = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_split;
    const int64_t r1 = r0 + rows_per_split < n ? r0 + rows_per_split : n;
    double s = 0.0;
    if (c < d)
        for (int64_t r = r0 + ph; r < r1; r += 4) s += (double)x[r * ld + c];
    red[ph][tid & (PF_SUM_COLS - 1)] = s;
    __syncthreads();
    if (ph == 0 && c < d) partial[(int64_t)blockIdx.y * d + c] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// running moments += partials, each element's partials added in split order first
__global__ __launch_bounds__(PF_BLOCK) void pca_fold_kernel(const double *__restrict__ sum_partial, int sum_splits, const double *__restrict__ s2_partial,
                                                            int splits, int pairs, int tiles, int d, double *__restrict__ sum,
                                                            double *__restrict__ s2) {
    const int64_t idx = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (idx < d) {
        double v = 0.0;
        for (int s = 0; s < sum_splits; ++s) v += sum_partial[(int64_t)s * d + idx];
        sum[idx] += v;
    }
    if (idx >= pairs * PF_TILE_ELEMS) return;
    const int pair = (int)(idx / PF_TILE_ELEMS), e = (int)(idx % PF_TILE_ELEMS);
    int ti, tj;
    pair_tiles(pair, tiles, ti, tj);
    const int i = ti * PF_T + e / PF_T, j = tj * PF_T + e % PF_T;
    if (i >= d || j >= d || j < i) return;      // a diagonal tile holds both halves: the upper one is kept
    double v = 0.0;
    for (int s = 0; s < splits; ++s) v += s2_partial[((int64_t)s * pairs + pair) * PF_TILE_ELEMS + e];
    s2[(int64_t)i * d + j] += v;
}

__global__ __launch_bounds__(PF_BLOCK) void pca_moments_kernel(const double *__restrict__ s2, int d, double *__restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (idx >= (int64_t)d * d) return;
    const int i = (int)(idx / d), j = (int)(idx % d);
    out[idx] = i <= j ? s2[idx] : s2[(int64_t)j * d + i];
}

// mean = sum / n;  cov[i][j] = (S2[a][b] - (n mean[a]) mean[b]) / (n - 1) with a = min(i, j), b = max(i, j)
__global__ __launch_bounds__(PF_BLOCK) void pca_cov_kernel(const double *__restrict__ sum, const double *__restrict__ s2, int d, double n,
                                                           double *__restrict__ mean, double *__restrict__ cov) {
    const int64_t idx = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (idx >= (int64_t)d * d) return;
    const int i = (int)(idx / d), j = (int)(idx % d);
    const int a = i <= j ? i : j, b = i <= j ? j : i;
    const double ma = sum[a] / n, mb = sum[b] / n;
    cov[idx] = (s2[(int64_t)a * d + b] - (n * ma) * mb) / (n - 1.0);
    if (i == 0) mean[j] = sum[j] / n;
}

}  // namespace

struct vsc_pca_fit {
    int d = 0, device = 0;
    int64_t n = 0;
    double *sum = nullptr, *s2 = nullptr;      // running moments (S2: upper triangle)
    void *scratch = nullptr;                   // partials of one update: grow-only, freed with the handle
    size_t scratch_bytes = 0;
};

extern "C" int vsc_pca_fit_create(int32_t d, vsc_pca_fit **out) {
    VSC_REQUIRE(out, "pca_fit_create: null pointer");
    *out = nullptr;
    VSC_REQUIRE(d >= PF_MIN_D && d <= PF_MAX_D, "pca_fit_create: %d features unsupported (%d .. %d)", d, PF_MIN_D, PF_MAX_D);
    vsc_pca_fit *f = new vsc_pca_fit;
    f->d = d;
    const size_t bytes = ((size_t)d * d + d) * sizeof(double);
    hipError_t e = hipGetDevice(&f->device);
    if (e == hipSuccess) e = hipMalloc((void **)&f->s2, bytes);
    if (e == hipSuccess) e = hipMemset(f->s2, 0, bytes);
    if (e != hipSuccess) {
        vsc_set_error("pca_fit_create: %zu bytes of moments: %s", bytes, hipGetErrorString(e));
        if (f->s2) (void)hipFree(f->s2);
        delete f;
        return VSC_ERR_HIP;
    }
    f->sum = f->s2 + (size_t)d * d;
    *out = f;
    return VSC_OK;
}

extern "C" void vsc_pca_fit_destroy(vsc_pca_fit *f) {
    if (!f) return;
    if (f->scratch) (void)hipFree(f->scratch);
    if (f->s2) (void)hipFree(f->s2);
    delete f;
}

extern "C" int vsc_pca_fit_update_f32(vsc_pca_fit *f, const float *x_dev, int64_t n, int64_t ld, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    VSC_REQUIRE(f, "pca_fit_update: null handle");
    VSC_REQUIRE(n >= 0, "pca_fit_update: %lld rows", (long long)n);
    if (n == 0) return VSC_OK;
    const int d = f->d;
    VSC_REQUIRE(x_dev, "pca_fit_update: null pointer");
    VSC_REQUIRE(ld >= d, "pca_fit_update: row stride %lld < %d features", (long long)ld, d);
    // the split of the rows depends on (n, d) alone
    const int tiles = (d + PF_T - 1) / PF_T, pairs = tiles * (tiles + 1) / 2;
    int64_t splits = (PF_TARGET_BLOCKS + pairs - 1) / pairs;
    if (splits > PF_MAX_PARTIAL_TILES / pairs) splits = PF_MAX_PARTIAL_TILES / pairs;
    if (splits > (n + PF_MIN_SPLIT_ROWS - 1) / PF_MIN_SPLIT_ROWS) splits = (n + PF_MIN_SPLIT_ROWS - 1) / PF_MIN_SPLIT_ROWS;
    if (splits < 1) splits = 1;
    const int64_t rows_per = ((n + splits - 1) / splits + PF_KR - 1) / PF_KR * PF_KR;
    splits = (n + rows_per - 1) / rows_per;
    int64_t sum_splits = (n + PF_SUM_ROWS - 1) / PF_SUM_ROWS;
    if (sum_splits > PF_SUM_MAX_SPLITS) sum_splits = PF_SUM_MAX_SPLITS;
    const int64_t sum_rows_per = (n + sum_splits - 1) / sum_splits;
    sum_splits = (n + sum_rows_per - 1) / sum_rows_per;

    const size_t sum_bytes = (size_t)sum_splits * d * sizeof(double);
    const size_t need = sum_bytes + (size_t)splits * pairs * PF_TILE_ELEMS * sizeof(double);
    if (need > f->scratch_bytes) {
        if (f->scratch) VSC_CHECK_HIP(hipFree(f->scratch));   // (synchronises the device: earlier updates have finished with it)
        f->scratch = nullptr, f->scratch_bytes = 0;
        hipError_t e = hipMalloc(&f->scratch, need);
        if (e != hipSuccess) {
            vsc_set_error("pca_fit_update: hipMalloc(%zu) failed: %s", need, hipGetErrorString(e));
            return VSC_ERR_NOMEM;
        }
        f->scratch_bytes = need;
    }
    double *sum_partial = (double *)f->scratch, *s2_partial = (double *)((char *)f->scratch + sum_bytes);
    hipLaunchKernelGGL(pca_s2_kernel, dim3((unsigned)pairs, (unsigned)splits), dim3(PF_BLOCK), 0, stream, x_dev, n, ld, d, tiles, rows_per, s2_partial);
    VSC_CHECK_LAUNCH();
    hipLaunchKernelGGL(pca_sum_kernel, dim3((unsigned)((d + PF_SUM_COLS - 1) / PF_SUM_COLS), (unsigned)sum_splits), dim3(PF_BLOCK), 0, stream, x_dev, n,
                       ld, d, sum_rows_per, sum_partial);
    VSC_CHECK_LAUNCH();
    const int64_t elems = pairs * PF_TILE_ELEMS;
    hipLaunchKernelGGL(pca_fold_kernel, dim3((unsigned)((elems + PF_BLOCK - 1) / PF_BLOCK)), dim3(PF_BLOCK), 0, stream, sum_partial, (int)sum_splits,
                       s2_partial, (int)splits, pairs, tiles, d, f->sum, f->s2);
    VSC_CHECK_LAUNCH();
    f->n += n;
    return VSC_OK;
}

extern "C" int vsc_pca_fit_moments_f64(vsc_pca_fit *f, double *sum_dev, double *s2_dev, int64_t *n_out, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    VSC_REQUIRE(f, "pca_fit_moments: null handle");
    if (n_out) *n_out = f->n;
    const int d = f->d;
    if (sum_dev) VSC_CHECK_HIP(hipMemcpyAsync(sum_dev, f->sum, (size_t)d * sizeof(double), hipMemcpyDeviceToDevice, stream));
    if (s2_dev) {
        hipLaunchKernelGGL(pca_moments_kernel, dim3((unsigned)(((int64_t)d * d + PF_BLOCK - 1) / PF_BLOCK)), dim3(PF_BLOCK), 0, stream, f->s2, d, s2_dev);
        VSC_CHECK_LAUNCH();
    }
    return VSC_OK;
}

extern "C" int vsc_pca_fit_covariance_f64(vsc_pca_fit *f, double *mean_dev, double *cov_dev, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    VSC_REQUIRE(f && mean_dev && cov_dev, "pca_fit_covariance: null pointer");
    VSC_REQUIRE(f->n >= 2, "pca_fit_covariance: %lld rows seen, a covariance needs 2", (long long)f->n);
    const int d = f->d;
    hipLaunchKernelGGL(pca_cov_kernel, dim3((unsigned)(((int64_t)d * d + PF_BLOCK - 1) / PF_BLOCK)), dim3(PF_BLOCK), 0, stream, f->sum, f->s2, d, (double)f->n,
                       mean_dev, cov_dev);
    VSC_CHECK_LAUNCH();
    return VSC_OK;
}
