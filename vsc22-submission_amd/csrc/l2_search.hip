// Exact squared-L2 search over a flat float32 bank: certified top-k and range search (replaces
// faiss.IndexFlat(d, METRIC_L2).search / .range_search -- infer/vsc/index.py:76-99, tests/test_index.py).
// Contract: include/vsc_hip.h above vsc_l2_augment_f32; executable form: tests/l2_search_contract.py.
//
// The reported distance of a pair is ONE definition, the ascending chain c <- fmaf(q_j - r_j, q_j - r_j, c), whatever path found
// the pair.  Paths:
//   probe   the inner-product sweep of knn.hip on augmented operands (q' = [2q, -1, -|q|^2], r' = [r, |r|^2, 1]: <q', r'> =
//           -|q - r|^2 up to rounding) selects kk candidates per query; l2_rescore_kernel runs the chain on them, orders the
//           (distance bits, id) keys and certifies the row: D_k < -s'_kk - slack(q), strictly, proves that no row outside the
//           probe can beat or tie the list (slack: DESIGN.md 4.3, "Exact L2 search").
//   direct  rows that are not certified -- and problems too small for a sweep -- take a path that needs no bound:
//           l2_dist_kernel materialises chunks of [rows, nr] chain distances, l2_select_kernel picks the k smallest per row by a
//           radix select on the bits, a stable compaction (lower id first among equals) and a sort of k.
// Range search: the inner-product range sweep at a radius widened by slack (a superset), the chain on the survivors, a count /
// scan / ordered fill into CSR; the direct form materialises chunks instead of sweeping.
// Every output position comes from a scan or a sort: results are a pure function of the inputs.
#include <float.h>
#include <math.h>
#include <string.h>

#include <vector>

#define VSC_TU_BF16 1   // no 16-bit operands here: one object for both builds of the library
#include "common.h"
#include "scan_sort.h"

namespace {

constexpr unsigned long long KEY_NONE = ~0ull;   // no candidate: sorts last
constexpr unsigned BITS_NONE = 0xFFFFFFFFu;      // a NaN or infinite distance: never reported, sorts last
constexpr int QT = 8;                            // queries per workgroup of l2_dist_kernel
constexpr size_t DIRECT_BYTES = 256u << 20;      // cap of one materialised [rows, nr] chunk

__device__ __forceinline__ unsigned dist_bits(float c) { return isfinite(c) ? __float_as_uint(c) : BITS_NONE; }

// the contract's chain of one pair; q may be LDS or global
__device__ __forceinline__ float l2_chain(const float *q, const float *__restrict__ r, int d) {
    float c = 0.f;
    for (int j = 0; j < d; ++j) {
        const float t = __fsub_rn(q[j], r[j]);
        c = __fmaf_rn(t, t, c);
    }
    return c;
}

// ---- augmentation: one wave per row ------------------------------------------------------------------------------------
// bank rows: [r, |r|^2, 1]; query rows: [2q, -1, -|q|^2].  |x|^2 in fp32 (64 lane-strided fmaf partial sums, a shuffle tree);
// norms[row] = |x|^2, and the largest |x|^2 of the rows as uint32 bits in *max_bits (zeroed by the caller; NaN bits compare
// above every number, so one non-finite row makes the maximum non-finite).  A row whose |x|^2 is not finite is written as a
// zero row (bank: [0, FLT_MAX, 1]; query: [0, -1, 0]): the sweep never sees a NaN, and the non-finite norm sends every
// row that depends on it to the direct path.
__global__ __launch_bounds__(256) void l2_augment_kernel(const float *__restrict__ x, int64_t n, int d, int as_query, float *__restrict__ aug,
                                                         float *__restrict__ norms, unsigned *__restrict__ max_bits) {
    const int lane = threadIdx.x & 63;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += (int64_t)gridDim.x * 4) {
        const float *xr = x + row * d;
        float s = 0.f;
        for (int j = lane; j < d; j += 64) s = __fmaf_rn(xr[j], xr[j], s);
        s = wave_sum(s);
        const bool ok = isfinite(s);
        if (aug) {
            float *ar = aug + row * (d + 2);
            for (int j = lane; j < d; j += 64) ar[j] = !ok ? 0.f : (as_query ? 2.f * xr[j] : xr[j]);
            if (lane == 0) {
                ar[d] = as_query ? -1.f : (ok ? s : FLT_MAX);
                ar[d + 1] = as_query ? (ok ? -s : 0.f) : 1.f;
            }
        }
        if (lane == 0) {
            if (norms) norms[row] = s;
            if (max_bits) atomicMax(max_bits, __float_as_uint(s) & 0x7FFFFFFFu);
        }
    }
}

// ---- ascending bitonic sort of P (a power of two <= 1024) keys in LDS by 256 threads ---------------------------------------
__device__ void block_sort_keys(unsigned long long *keys, int P) {
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = threadIdx.x; i < P / 2; i += 256) {
                const int pos = 2 * i - (i & (stride - 1));
                const unsigned long long a = keys[pos], b = keys[pos + stride];
                const bool asc = (pos & size) == 0;
                if ((a > b) == asc) {
                    keys[pos] = b;
                    keys[pos + stride] = a;
                }
            }
        }
    __syncthreads();
}

// first k sorted keys -> one output row; slots without a candidate hold (FLT_MAX, -1)
__device__ void write_row(const unsigned long long *keys, int have, int k, int64_t id_offset, float *__restrict__ out_d,
                          int64_t *__restrict__ out_i) {
    for (int i = threadIdx.x; i < k; i += 256) {
        const unsigned long long key = i < have ? keys[i] : KEY_NONE;
        out_d[i] = key == KEY_NONE ? FLT_MAX : __uint_as_float((unsigned)(key >> 32));
        out_i[i] = key == KEY_NONE ? -1 : (int64_t)(key & 0xFFFFFFFFull) + id_offset;
    }
}

// slack(q) of the certificate and of the widened radius: a bound on |expanded score + chain distance| for every
// bank row, from the computed |q|^2 and the computed largest |r|^2.  Not finite, or (|q| + max|r|)^2 >= 1e38 (a partial sum of
// the sweep could overflow): no bound -> +inf.
__device__ __host__ inline double l2_slack(int d, float qn2, float rmax2) {
    if (!(qn2 >= 0.f && qn2 <= FLT_MAX && rmax2 >= 0.f && rmax2 <= FLT_MAX)) return INFINITY;
    const double s = sqrt((double)qn2) + sqrt((double)rmax2), S = s * s;
    if (!(S < 1.0e38)) return INFINITY;
    const double terms = 3.0 * d + 8.0;
    return terms * 5.9604644775390625e-08 /* 2^-24 */ * S * 1.01 + terms * 1.1754943508222875e-38 /* 2^-126 */;
}

// ---- probe re-score, order, certificate: one workgroup per query row ------------------------------------------------------
// probe_s / probe_i [nq, kk]: the sweep's result on the augmented operands (scores descending, ids without offset, -1 padding).
// rows_list: the wider probe's query rows (its probe and flags are indexed by position in the list), or nullptr: every row.
// LDS: the query row (d floats, dynamic) + 1024 keys.
__global__ __launch_bounds__(256) void l2_rescore_kernel(const float *__restrict__ q, const float *__restrict__ r, int64_t nr, int d, int k, int kk,
                                                         const float *__restrict__ probe_s, const int64_t *__restrict__ probe_i,
                                                         const float *__restrict__ qnorm, const unsigned *__restrict__ rmax_bits,
                                                         int64_t id_offset, const int64_t *__restrict__ rows_list,
                                                         float *__restrict__ out_d, int64_t *__restrict__ out_i, int *__restrict__ certified) {
    extern __shared__ float lds_q[];
    __shared__ unsigned long long keys[1024];
    __shared__ int n_valid;
    const int64_t b = blockIdx.x, row = rows_list ? rows_list[b] : b;   // b: row of the probe and of the flags; row: query / output row
    if (threadIdx.x == 0) n_valid = 0;
    for (int j = threadIdx.x; j < d; j += 256) lds_q[j] = q[row * d + j];
    int P = 1;
    while (P < kk) P <<= 1;
    __syncthreads();
    int valid = 0;
    for (int c = threadIdx.x; c < P; c += 256) {
        unsigned long long key = KEY_NONE;
        if (c < kk) {
            const int64_t id = probe_i[b * kk + c];
            if (id >= 0 && id < nr) {
                ++valid;
                const unsigned b = dist_bits(l2_chain(lds_q, r + id * d, d));
                if (b != BITS_NONE) key = ((unsigned long long)b << 32) | (unsigned long long)id;
            }
        }
        keys[c] = key;
    }
    if (valid) atomicAdd(&n_valid, valid);
    block_sort_keys(keys, P);
    write_row(keys, kk < P ? kk : P, k, id_offset, out_d + row * k, out_i + row * k);
    if (threadIdx.x == 0) {
        bool ok;
        if (kk >= nr) {
            ok = n_valid == nr;          // the probe held the whole bank (and lost no row to a NaN score)
        } else {
            const float s_kk = probe_s[b * kk + kk - 1];
            const double slack = l2_slack(d, qnorm[row], __uint_as_float(*rmax_bits));
            const unsigned long long kth = k <= kk ? keys[k - 1] : KEY_NONE;
            ok = kth != KEY_NONE && isfinite(s_kk) && slack < (double)INFINITY &&
                 (double)__uint_as_float((unsigned)(kth >> 32)) < -(double)s_kk - slack;
        }
        certified[b] = ok ? 1 : 0;
    }
}

// ---- direct path: chain distances of a chunk of query rows against every bank row ------------------------------------------
// grid (bank tiles of 256 rows, groups of QT query rows).  rows_list: the query rows of the chunk (nullptr: row0 + i).  A thread owns
// one bank row and QT accumulators; the bank tile goes through LDS in pieces of 32 columns (coalesced loads, stride 33: no bank
// conflict), j ascending throughout.  out[i * nr + ref] = distance bits (BITS_NONE: not finite).
__global__ __launch_bounds__(256) void l2_dist_kernel(const float *__restrict__ q, const float *__restrict__ r, int64_t nr, int d,
                                                      const int64_t *__restrict__ rows_list, int64_t row0, int64_t rows,
                                                      unsigned *__restrict__ out) {
    __shared__ float lr[256][33];
    __shared__ float lq[QT][32];
    const int tid = threadIdx.x;
    const int64_t ref0 = (int64_t)blockIdx.x * 256, i0 = (int64_t)blockIdx.y * QT;
    float c[QT];
#pragma unroll
    for (int i = 0; i < QT; ++i) c[i] = 0.f;
    int64_t qrow = -1;
    {
        const int64_t i = i0 + (tid >> 5);
        if (i < rows) qrow = rows_list ? rows_list[i] : row0 + i;
    }
    for (int j0 = 0; j0 < d; j0 += 32) {
        const int jn = d - j0 < 32 ? d - j0 : 32;
        __syncthreads();
        const int col = tid & 31;
        for (int i = 0; i < 32; ++i) {
            const int lrow = i * 8 + (tid >> 5);
            const int64_t ref = ref0 + lrow;
            lr[lrow][col] = (ref < nr && col < jn) ? r[ref * d + j0 + col] : 0.f;
        }
        lq[tid >> 5][col] = (qrow >= 0 && col < jn) ? q[qrow * d + j0 + col] : 0.f;
        __syncthreads();
        for (int j = 0; j < jn; ++j) {
            const float rv = lr[tid][j];
#pragma unroll
            for (int i = 0; i < QT; ++i) {
                const float t = __fsub_rn(lq[i][j], rv);
                c[i] = __fmaf_rn(t, t, c[i]);
            }
        }
    }
    const int64_t ref = ref0 + tid;
    if (ref < nr)
#pragma unroll
        for (int i = 0; i < QT; ++i)
            if (i0 + i < rows) out[(i0 + i) * nr + ref] = dist_bits(c[i]);
}

// exclusive rank of this thread's flag among the workgroup's 256 threads, and the workgroup's total (wave ballots + 4 wave sums)
__device__ __forceinline__ int block_rank(bool flag, int *wave_tot, int *total) {
    const unsigned long long b = __ballot(flag);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) wave_tot[w] = __popcll(b);
    __syncthreads();
    int before = __popcll(b & ((1ull << lane) - 1ull));
    int tot = 0;
    for (int i = 0; i < 4; ++i) {
        if (i < w) before += wave_tot[i];
        tot += wave_tot[i];
    }
    *total = tot;
    return before;
}

// ---- direct path: the k smallest of one materialised row -------------------------------------------------------------------
// One workgroup per query row of the chunk.  Radix select (4 passes of 8 bits) of the kth-smallest distance bits T among the finite
// ones, then one ordered pass: every entry below T, and the first entries equal to T in ascending id until k are held, then the
// sort of k.  Integer LDS atomics only accumulate histogram counts; every position comes from a scan.
__global__ __launch_bounds__(256) void l2_select_kernel(const unsigned *__restrict__ dist, int64_t nr, int k, const int64_t *__restrict__ rows_list,
                                                        int64_t row0, int64_t id_offset, float *__restrict__ out_d, int64_t *__restrict__ out_i) {
    __shared__ unsigned long long keys[1024];
    __shared__ int hist[256];
    __shared__ int wave_tot[4];
    __shared__ unsigned sh_prefix;
    __shared__ int sh_remaining, sh_fin;
    const int tid = threadIdx.x;
    const unsigned *du = dist + (int64_t)blockIdx.x * nr;
    const int64_t qrow = rows_list ? rows_list[blockIdx.x] : row0 + blockIdx.x;
    if (tid == 0) sh_fin = 0;
    __syncthreads();
    int fin = 0;
    for (int64_t i = tid; i < nr; i += 256) fin += du[i] != BITS_NONE;
    if (fin) atomicAdd(&sh_fin, fin);
    __syncthreads();
    const int kth = (int64_t)k < (int64_t)sh_fin ? k : sh_fin;   // entries to report
    int P = 1;
    while (P < kth) P <<= 1;
    if (kth > 0) {
        if (tid == 0) { sh_prefix = 0; sh_remaining = kth; }
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            hist[tid] = 0;
            __syncthreads();
            const unsigned prefix = sh_prefix, himask = pass == 0 ? 0u : 0xFFFFFFFFu << (shift + 8);
            for (int64_t i = tid; i < nr; i += 256) {
                const unsigned v = du[i];
                if ((v & himask) == prefix) atomicAdd(&hist[(v >> shift) & 255], 1);
            }
            __syncthreads();
            if (tid == 0) {
                int rem = sh_remaining, dgt = 0;
                while (dgt < 255 && hist[dgt] < rem) rem -= hist[dgt++];
                sh_remaining = rem;
                sh_prefix = prefix | ((unsigned)dgt << shift);
            }
            __syncthreads();
        }
        const unsigned T = sh_prefix;
        const int need_eq = sh_remaining, n_less = kth - need_eq;
        for (int i = tid; i < P; i += 256) keys[i] = KEY_NONE;
        int base_less = 0, base_eq = 0;
        for (int64_t t0 = 0; t0 < nr; t0 += 256) {
            const int64_t i = t0 + tid;
            const unsigned v = i < nr ? du[i] : BITS_NONE;
            const bool less = v < T, eq = v == T;
            int tot_less, tot_eq;
            const int rl = block_rank(less, wave_tot, &tot_less);
            const int re = block_rank(eq, wave_tot, &tot_eq);
            const unsigned long long key = ((unsigned long long)v << 32) | (unsigned long long)i;
            if (less && base_less + rl < n_less) keys[base_less + rl] = key;
            if (eq && base_eq + re < need_eq) keys[n_less + base_eq + re] = key;
            base_less += tot_less;
            base_eq += tot_eq;
        }
        block_sort_keys(keys, P);
    }
    write_row(keys, kth, k, id_offset, out_d + qrow * k, out_i + qrow * k);
}

// dst[i] = src[rows_list[i]], rows of `width` floats: the augmented queries of the wider probe
__global__ __launch_bounds__(256) void l2_gather_rows_kernel(const float *__restrict__ src, const int64_t *__restrict__ rows_list, int width,
                                                             float *__restrict__ dst) {
    const float *s = src + rows_list[blockIdx.x] * width;
    float *o = dst + (int64_t)blockIdx.x * width;
    for (int j = threadIdx.x; j < width; j += 256) o[j] = s[j];
}

__global__ __launch_bounds__(256) void l2_fill_empty_kernel(int64_t n, float *__restrict__ out_d, int64_t *__restrict__ out_i) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        out_d[i] = FLT_MAX;
        out_i[i] = -1;
    }
}

// ---- range search ----------------------------------------------------------------------------------------------------------
// A segment per query row: entries [seg0, seg1) of `dist` (distance bits) with ids ids[i], or -- ids == nullptr -- the materialised
// row: entry i of segment s is bank row i - s * nr.

// chain distances of the sweep's survivors, in place of their expanded scores
__global__ __launch_bounds__(256) void l2_range_rescore_kernel(const float *__restrict__ q, const float *__restrict__ r, int64_t nr, int d,
                                                               const int64_t *__restrict__ seg_lims, const int64_t *__restrict__ ids,
                                                               unsigned *__restrict__ dist) {
    extern __shared__ float lds_q[];
    const int64_t row = blockIdx.x;
    const int64_t a = seg_lims[row], b = seg_lims[row + 1];
    if (a == b) return;
    for (int j = threadIdx.x; j < d; j += 256) lds_q[j] = q[row * d + j];
    __syncthreads();
    for (int64_t i = a + threadIdx.x; i < b; i += 256) {
        const int64_t id = ids[i];
        dist[i] = id >= 0 && id < nr ? dist_bits(l2_chain(lds_q, r + id * d, d)) : BITS_NONE;
    }
}

__device__ __forceinline__ bool range_hit(unsigned bits, float radius) { return bits != BITS_NONE && __uint_as_float(bits) < radius; }

__global__ __launch_bounds__(256) void l2_range_count_kernel(const unsigned *__restrict__ dist, const int64_t *__restrict__ seg_lims, int64_t nr,
                                                             float radius, long long *__restrict__ counts) {
    __shared__ long long sh;
    const int64_t s = blockIdx.x;
    const int64_t a = seg_lims ? seg_lims[s] : s * nr, b = seg_lims ? seg_lims[s + 1] : (s + 1) * nr;
    if (threadIdx.x == 0) sh = 0;
    __syncthreads();
    long long n = 0;
    for (int64_t i = a + threadIdx.x; i < b; i += 256) n += range_hit(dist[i], radius);
    if (n) atomicAdd((unsigned long long *)&sh, (unsigned long long)n);
    __syncthreads();
    if (threadIdx.x == 0) counts[s] = sh;
}

// lims[0] = 0, lims[i + 1] = counts[0] + .. + counts[i]: one workgroup of 1024 threads walks the rows in tiles
__global__ __launch_bounds__(1024) void l2_range_scan_kernel(const long long *__restrict__ counts, int64_t n, int64_t *__restrict__ lims) {
    __shared__ long long buf[1024];
    __shared__ long long carry;
    const int tid = threadIdx.x;
    if (tid == 0) {
        carry = 0;
        lims[0] = 0;
    }
    __syncthreads();
    for (int64_t t0 = 0; t0 < n; t0 += 1024) {
        const int64_t i = t0 + tid;
        long long v = i < n ? counts[i] : 0;
        buf[tid] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const long long add = tid >= o ? buf[tid - o] : 0;
            __syncthreads();
            buf[tid] += add;
            __syncthreads();
        }
        if (i < n) lims[i + 1] = carry + buf[tid];
        __syncthreads();
        if (tid == 0) carry += buf[1023];
        __syncthreads();
    }
}

// hits of segment s -> CSR row lims_row0 + s, in the segment's order (ascending id)
__global__ __launch_bounds__(256) void l2_range_fill_kernel(const unsigned *__restrict__ dist, const int64_t *__restrict__ seg_lims,
                                                            const int64_t *__restrict__ ids, int64_t nr, float radius, const int64_t *__restrict__ lims,
                                                            int64_t id_offset, float *__restrict__ out_d, int64_t *__restrict__ out_i) {
    __shared__ int wave_tot[4];
    const int64_t s = blockIdx.x;
    const int64_t a = seg_lims ? seg_lims[s] : s * nr, b = seg_lims ? seg_lims[s + 1] : (s + 1) * nr;
    int64_t base = lims[s];
    if (lims[s + 1] == base) return;
    for (int64_t t0 = a; t0 < b; t0 += 256) {
        const int64_t i = t0 + threadIdx.x;
        const unsigned v = i < b ? dist[i] : BITS_NONE;
        const bool hit = range_hit(v, radius);
        int tot;
        const int rank = block_rank(hit, wave_tot, &tot);
        if (hit) {
            out_d[base + rank] = __uint_as_float(v);
            out_i[base + rank] = (ids ? ids[i] : i - a) + id_offset;
        }
        base += tot;
    }
}

inline unsigned blocks_of(int64_t items, int per) {
    const int64_t b = (items + per - 1) / per;
    return (unsigned)(b < 1 ? 1 : b);
}

int augment(const float *x, int64_t n, int d, int as_query, float *aug, float *norms, unsigned *max_bits, hipStream_t stream) {
    if (max_bits) VSC_CHECK_HIP(hipMemsetAsync(max_bits, 0, 4, stream));
    if (n <= 0) return VSC_OK;
    const int64_t blocks = (n + 3) / 4;
    hipLaunchKernelGGL(l2_augment_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, stream, x, n, d, as_query, aug, norms,
                       max_bits);
    VSC_CHECK_LAUNCH();
    return VSC_OK;
}

// rows of one materialised chunk: DIRECT_BYTES of distances, at least QT rows, at most 65 535 row groups (gridDim.y)
inline int64_t chunk_rows(int64_t nr) {
    int64_t rows = (int64_t)(DIRECT_BYTES / 4) / nr;
    if (rows < QT) rows = QT;
    if (rows > 65535ll * QT) rows = 65535ll * QT;
    return rows;
}

int launch_dist(const float *q, const float *r, int64_t nr, int d, const int64_t *rows_list, int64_t row0, int64_t rows, unsigned *dist,
                hipStream_t stream) {
    hipLaunchKernelGGL(l2_dist_kernel, dim3(blocks_of(nr, 256), blocks_of(rows, QT)), dim3(256), 0, stream, q, r, nr, d, rows_list, row0, rows, dist);
    VSC_CHECK_LAUNCH();
    return VSC_OK;
}

// top-k of `n` query rows (rows_list, or nullptr: all of 0 .. n - 1) on the direct path
int knn_direct(const float *q, const float *r, int64_t nr, int d, int k, int64_t id_offset, const int64_t *rows_list, int64_t n, float *out_d,
               int64_t *out_i, hipStream_t stream) {
    const int64_t step = chunk_rows(nr);
    unsigned *dist;
    VSC_TRY(search_scratch_get(SCRATCH_L2_DIST, (size_t)(n < step ? n : step) * nr * 4, &dist));
    for (int64_t lo = 0; lo < n; lo += step) {
        const int64_t rows = n - lo < step ? n - lo : step;
        VSC_TRY(launch_dist(q, r, nr, d, rows_list ? rows_list + lo : nullptr, lo, rows, dist, stream));
        hipLaunchKernelGGL(l2_select_kernel, dim3((unsigned)rows), dim3(256), 0, stream, (const unsigned *)dist, nr, k,
                           rows_list ? rows_list + lo : nullptr, lo, id_offset, out_d, out_i);
        VSC_CHECK_LAUNCH();
    }
    return VSC_OK;
}

enum { L2_AUTO = 0, L2_PROBE = 1, L2_DIRECT = 2 };
int forced_path() {
    const char *e = vsc_opt(OPT_L2_PATH);
    return e && e[0] == 'p' ? L2_PROBE : (e && e[0] == 'd' ? L2_DIRECT : L2_AUTO);
}

int64_t g_last_path[3] = {0, 0, 0};   // rows of the last vsc_knn_l2_f32 call: certified at the first probe, at the wider probe, direct

}  // namespace

extern "C" int vsc_l2_augment_f32(void *stream_, const float *x_dev, int64_t n, int32_t d, int32_t as_query, float *aug_dev, float *norms_dev,
                                  float *max_norm_dev) {
    VSC_REQUIRE(n >= 0 && (n == 0 || x_dev), "l2_augment: null pointer");
    VSC_REQUIRE(d >= 1 && d <= 4094, "l2_augment: dimension %d unsupported (1 .. 4094: the augmented row has d + 2 <= 4096 columns)", d);
    VSC_REQUIRE(aug_dev || norms_dev || max_norm_dev, "l2_augment: no output");
    if (max_norm_dev) VSC_REQUIRE_ALIGNED("l2_augment", max_norm_dev, 4);
    return augment(x_dev, n, d, as_query != 0, aug_dev, norms_dev, (unsigned *)max_norm_dev, (hipStream_t)stream_);
}

extern "C" int vsc_knn_l2_last_path(int64_t rows_out[3]) {
    VSC_REQUIRE(rows_out, "knn_l2_last_path: null pointer");
    for (int i = 0; i < 3; ++i) rows_out[i] = g_last_path[i];
    return VSC_OK;
}

// the bank's augmented rows and largest norm: the caller's (vsc_l2_augment_f32, once per bank), or made here for this call
static int bank_operands(const float *r_dev, int64_t nr, int d, const float *r_aug_dev, const float *r_max_norm_dev, const float **aug,
                         const unsigned **max_bits, hipStream_t stream) {
    if (r_aug_dev) {
        *aug = r_aug_dev;
        *max_bits = (const unsigned *)r_max_norm_dev;
        return VSC_OK;
    }
    float *a;
    unsigned *m;
    VSC_TRY(search_scratch_get(SCRATCH_L2_RAUG, (size_t)nr * (d + 2) * 4, &a));
    VSC_TRY(search_scratch_get(SCRATCH_L2_RMAX, 16, &m));
    VSC_TRY(augment(r_dev, nr, d, 0, a, nullptr, m, stream));
    *aug = a;
    *max_bits = m;
    return VSC_OK;
}

extern "C" int vsc_knn_l2_f32(void *stream_, const float *q_dev, int64_t nq, const float *r_dev, int64_t nr, int32_t d, int32_t k,
                              int64_t ref_id_offset, const float *r_aug_dev, const float *r_max_norm_dev, float *out_dist_dev,
                              int64_t *out_ids_dev) {
    hipStream_t stream = (hipStream_t)stream_;
    VSC_REQUIRE(nq >= 0 && nr >= 0, "knn_l2: negative row count (nq=%lld nr=%lld)", (long long)nq, (long long)nr);
    VSC_REQUIRE(d >= 1 && d <= 4096, "knn_l2: dimension %d unsupported (1 .. 4096)", d);
    VSC_REQUIRE(k >= 1 && k <= 1024, "knn_l2: k=%d out of range [1,1024]", k);
    VSC_REQUIRE(nr < (1ll << 32) - 1, "knn_l2: more than 2^32-2 references in one call");
    VSC_REQUIRE((r_aug_dev == nullptr) == (r_max_norm_dev == nullptr), "knn_l2: r_aug_dev and r_max_norm_dev come together");
    const int forced = forced_path();
    VSC_REQUIRE(!(forced == L2_PROBE && d > 4094), "knn_l2: VSC_L2_PATH=probe needs d <= 4094 (d + 2 <= 4096), not %d", d);
    VSC_REQUIRE(!(r_aug_dev && d > 4094), "knn_l2: augmented rows exist up to d = 4094, not %d", d);
    if (r_aug_dev && d + 2 < 32 && ((d + 2) & 3) == 0) VSC_REQUIRE_ALIGNED("knn_l2", r_aug_dev, 16);   // as vsc_knn_ip_f32 reads its bank
    if (nq == 0) return VSC_OK;
    VSC_REQUIRE(q_dev && out_dist_dev && out_ids_dev && (r_dev || nr == 0), "knn_l2: null pointer");
    g_last_path[0] = g_last_path[1] = g_last_path[2] = 0;
    if (nr == 0) {
        hipLaunchKernelGGL(l2_fill_empty_kernel, dim3(blocks_of(nq * k, 256)), dim3(256), 0, stream, nq * k, out_dist_dev, out_ids_dev);
        VSC_CHECK_LAUNCH();
        return VSC_OK;
    }
    int64_t kk = k + 8 > 2 * k ? k + 8 : 2 * k;
    if (kk > 1024) kk = 1024;
    // a bank that one probe would hold whole is too small for a sweep: the direct path at once
    const bool probe = forced == L2_PROBE || (forced == L2_AUTO && d <= 4094 && nr > kk);
    if (!probe) {
        g_last_path[2] = nq;
        return knn_direct(q_dev, r_dev, nr, d, k, ref_id_offset, nullptr, nq, out_dist_dev, out_ids_dev, stream);
    }
    if (kk > nr) kk = nr;
    float *q_aug, *q_norm;
    int64_t *rows_dev;
    int *flags;
    const float *r_aug;
    const unsigned *r_max;
    VSC_TRY(search_scratch_get(SCRATCH_L2_QAUG, (size_t)nq * (d + 2) * 4, &q_aug));
    VSC_TRY(search_scratch_get(SCRATCH_L2_QNORM, (size_t)nq * 4, &q_norm));
    VSC_TRY(search_scratch_get(SCRATCH_L2_FLAGS, (size_t)nq * 4, &flags));
    VSC_TRY(search_scratch_get(SCRATCH_L2_ROWS, (size_t)nq * 8, &rows_dev));
    VSC_TRY(bank_operands(r_dev, nr, d, r_aug_dev, r_max_norm_dev, &r_aug, &r_max, stream));
    VSC_TRY(augment(q_dev, nq, d, 1, q_aug, q_norm, nullptr, stream));
    // the rows a probe of `ranks` ranks cannot certify: sweep, re-score (their lists are written either way), read the flags
    std::vector<int64_t> todo;
    auto probe_pass = [&](const float *qa, int64_t n, int64_t ranks, const int64_t *rows_list) -> int {
        float *probe_s;
        int64_t *probe_i;
        VSC_TRY(search_scratch_get(SCRATCH_L2_PROBE_S, (size_t)n * ranks * 4, &probe_s));
        VSC_TRY(search_scratch_get(SCRATCH_L2_PROBE_I, (size_t)n * ranks * 8, &probe_i));
        VSC_TRY(search_knn_ip(qa, n, r_aug, nr, d + 2, (int)ranks, probe_s, probe_i, stream));
        hipLaunchKernelGGL(l2_rescore_kernel, dim3((unsigned)n), dim3(256), (size_t)d * 4, stream, q_dev, r_dev, nr, d, k, (int)ranks,
                           (const float *)probe_s, (const int64_t *)probe_i, (const float *)q_norm, r_max, ref_id_offset, rows_list, out_dist_dev,
                           out_ids_dev, flags);
        VSC_CHECK_LAUNCH();
        std::vector<int> host_flags((size_t)n);
        VSC_CHECK_HIP(hipMemcpyAsync(host_flags.data(), flags, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
        VSC_CHECK_HIP(hipStreamSynchronize(stream));
        std::vector<int64_t> left;
        for (int64_t i = 0; i < n; ++i)
            if (!host_flags[(size_t)i]) left.push_back(rows_list ? todo[(size_t)i] : i);
        todo.swap(left);
        if (!todo.empty()) {
            VSC_CHECK_HIP(hipMemcpyAsync(rows_dev, todo.data(), todo.size() * 8, hipMemcpyHostToDevice, stream));
            VSC_CHECK_HIP(hipStreamSynchronize(stream));   // `todo` is pageable host memory: the copy is done before it changes
        }
        return VSC_OK;
    };
    VSC_TRY(probe_pass(q_aug, nq, kk, nullptr));
    g_last_path[0] = nq - (int64_t)todo.size();
    // one wider probe for what is left: four times the ranks, at least 256 -- unless that is the whole bank, which the direct path
    // answers at the same cost without a bound
    int64_t wide = 4 * kk < 256 ? 256 : 4 * kk;
    if (wide > 1024) wide = 1024;
    if (!todo.empty() && wide > kk && wide < nr && !vsc_opt_is(OPT_L2_WIDE, '0')) {
        const int64_t n = (int64_t)todo.size();
        float *q_aug2;
        VSC_TRY(search_scratch_get(SCRATCH_L2_QAUG2, (size_t)n * (d + 2) * 4, &q_aug2));
        hipLaunchKernelGGL(l2_gather_rows_kernel, dim3((unsigned)n), dim3(256), 0, stream, (const float *)q_aug, (const int64_t *)rows_dev, d + 2,
                           q_aug2);
        VSC_CHECK_LAUNCH();
        VSC_TRY(probe_pass(q_aug2, n, wide, rows_dev));
        g_last_path[1] = n - (int64_t)todo.size();
    }
    g_last_path[2] = (int64_t)todo.size();
    if (todo.empty()) return VSC_OK;
    return knn_direct(q_dev, r_dev, nr, d, k, ref_id_offset, rows_dev, (int64_t)todo.size(), out_dist_dev, out_ids_dev, stream);
}

// counts -> lims -> total (one synchronisation); -> whether the fill may run
static int range_total(const long long *counts, int64_t nq, int64_t *lims_dev, int64_t capacity, int64_t *total_out, bool *fill,
                       hipStream_t stream) {
    hipLaunchKernelGGL(l2_range_scan_kernel, dim3(1), dim3(1024), 0, stream, counts, nq, lims_dev);
    VSC_CHECK_LAUNCH();
    int64_t total = 0;
    VSC_CHECK_HIP(hipMemcpyAsync(&total, lims_dev + nq, 8, hipMemcpyDeviceToHost, stream));
    VSC_CHECK_HIP(hipStreamSynchronize(stream));
    *total_out = total;
    *fill = total > 0 && total <= capacity;
    return VSC_OK;
}

extern "C" int vsc_range_search_l2_f32(void *stream_, const float *q_dev, int64_t nq, const float *r_dev, int64_t nr, int32_t d, float radius,
                                       int64_t ref_id_offset, const float *r_aug_dev, const float *r_max_norm_dev, int64_t *lims_dev,
                                       float *out_dist_dev, int64_t *out_ids_dev, int64_t capacity, int64_t *total_out) {
    hipStream_t stream = (hipStream_t)stream_;
    VSC_REQUIRE(nq >= 0 && nr >= 0, "range_search_l2: negative row count (nq=%lld nr=%lld)", (long long)nq, (long long)nr);
    VSC_REQUIRE(lims_dev && total_out, "range_search_l2: null pointer");
    VSC_REQUIRE(d >= 1 && d <= 4096, "range_search_l2: dimension %d unsupported (1 .. 4096)", d);
    VSC_REQUIRE(nr < (1ll << 32) - 1, "range_search_l2: more than 2^32-2 references in one call");
    VSC_REQUIRE(capacity >= 0 && (capacity == 0 || (out_dist_dev && out_ids_dev)), "range_search_l2: capacity %lld without output buffers",
                (long long)capacity);
    VSC_REQUIRE((r_aug_dev == nullptr) == (r_max_norm_dev == nullptr), "range_search_l2: r_aug_dev and r_max_norm_dev come together");
    const int forced = forced_path();
    VSC_REQUIRE(!(forced == L2_PROBE && d > 4094), "range_search_l2: VSC_L2_PATH=probe needs d <= 4094 (d + 2 <= 4096), not %d", d);
    VSC_REQUIRE(!(r_aug_dev && d > 4094), "range_search_l2: augmented rows exist up to d = 4094, not %d", d);
    if (r_aug_dev && d + 2 < 32 && ((d + 2) & 3) == 0) VSC_REQUIRE_ALIGNED("range_search_l2", r_aug_dev, 16);
    *total_out = 0;
    if (nq == 0 || nr == 0 || !(radius > 0.f)) {   // distances are >= 0: nothing is below a radius <= 0 (or NaN)
        VSC_CHECK_HIP(hipMemsetAsync(lims_dev, 0, (size_t)(nq + 1) * 8, stream));
        return VSC_OK;
    }
    VSC_REQUIRE(q_dev && r_dev, "range_search_l2: null pointer");
    long long *counts;
    VSC_TRY(search_scratch_get(SCRATCH_L2_COUNTS, (size_t)nq * 8, &counts));
    bool fill = false;
    if (forced != L2_DIRECT && d <= 4094) {
        // the sweep's radius: widened by the largest slack of the call (one read of the two norm maxima)
        float *q_aug;
        unsigned *q_max;
        const float *r_aug;
        const unsigned *r_max;
        VSC_TRY(search_scratch_get(SCRATCH_L2_QAUG, (size_t)nq * (d + 2) * 4, &q_aug));
        VSC_TRY(search_scratch_get(SCRATCH_L2_QNORM, 16, &q_max));
        VSC_TRY(bank_operands(r_dev, nr, d, r_aug_dev, r_max_norm_dev, &r_aug, &r_max, stream));
        VSC_TRY(augment(q_dev, nq, d, 1, q_aug, nullptr, q_max, stream));
        unsigned maxima[2] = {0, 0};
        VSC_CHECK_HIP(hipMemcpyAsync(&maxima[0], q_max, 4, hipMemcpyDeviceToHost, stream));
        VSC_CHECK_HIP(hipMemcpyAsync(&maxima[1], r_max, 4, hipMemcpyDeviceToHost, stream));
        VSC_CHECK_HIP(hipStreamSynchronize(stream));
        float qm, rm;
        memcpy(&qm, &maxima[0], 4);
        memcpy(&rm, &maxima[1], 4);
        const double wide = (double)radius + l2_slack(d, qm, rm);
        if (wide < 1.0e38) {
            const float sweep_radius = -nextafterf((float)wide, INFINITY);   // (float) rounds to nearest: one step up covers it
            int64_t *s_lims, *s_ids;
            float *s_scores;
            int64_t cap = 1 << 20, total_s = 0;
            VSC_TRY(search_scratch_get(SCRATCH_L2_SLIMS, (size_t)(nq + 1) * 8, &s_lims));
            for (int attempt = 0; attempt < 2; ++attempt) {
                VSC_TRY(search_scratch_get(SCRATCH_L2_PROBE_S, (size_t)cap * 4, &s_scores));
                VSC_TRY(search_scratch_get(SCRATCH_L2_PROBE_I, (size_t)cap * 8, &s_ids));
                VSC_TRY(search_range_ip(q_aug, nq, r_aug, nr, d + 2, sweep_radius, s_lims, s_scores, s_ids, cap, &total_s, stream));
                if (total_s <= cap) break;
                VSC_REQUIRE(attempt == 0, "range_search_l2: the sweep's count changed between two calls");
                cap = total_s;
            }
            if (total_s == 0) {
                VSC_CHECK_HIP(hipMemsetAsync(lims_dev, 0, (size_t)(nq + 1) * 8, stream));
                return VSC_OK;
            }
            unsigned *s_dist = (unsigned *)s_scores;
            hipLaunchKernelGGL(l2_range_rescore_kernel, dim3((unsigned)nq), dim3(256), (size_t)d * 4, stream, q_dev, r_dev, nr, d,
                               (const int64_t *)s_lims, (const int64_t *)s_ids, s_dist);
            VSC_CHECK_LAUNCH();
            hipLaunchKernelGGL(l2_range_count_kernel, dim3((unsigned)nq), dim3(256), 0, stream, (const unsigned *)s_dist, (const int64_t *)s_lims, nr,
                               radius, counts);
            VSC_CHECK_LAUNCH();
            VSC_TRY(range_total(counts, nq, lims_dev, capacity, total_out, &fill, stream));
            if (fill) {
                hipLaunchKernelGGL(l2_range_fill_kernel, dim3((unsigned)nq), dim3(256), 0, stream, (const unsigned *)s_dist, (const int64_t *)s_lims,
                                   (const int64_t *)s_ids, nr, radius, (const int64_t *)lims_dev, ref_id_offset, out_dist_dev, out_ids_dev);
                VSC_CHECK_LAUNCH();
            }
            return VSC_OK;
        }
    }
    // direct: materialised chunks, counted, then -- if the hits fit -- materialised again and filled
    const int64_t step = chunk_rows(nr);
    unsigned *dist;
    VSC_TRY(search_scratch_get(SCRATCH_L2_DIST, (size_t)(nq < step ? nq : step) * nr * 4, &dist));
    for (int pass = 0; pass < 2; ++pass) {
        for (int64_t lo = 0; lo < nq; lo += step) {
            const int64_t rows = nq - lo < step ? nq - lo : step;
            VSC_TRY(launch_dist(q_dev, r_dev, nr, d, nullptr, lo, rows, dist, stream));
            if (pass == 0)
                hipLaunchKernelGGL(l2_range_count_kernel, dim3((unsigned)rows), dim3(256), 0, stream, (const unsigned *)dist,
                                   (const int64_t *)nullptr, nr, radius, counts + lo);
            else
                hipLaunchKernelGGL(l2_range_fill_kernel, dim3((unsigned)rows), dim3(256), 0, stream, (const unsigned *)dist,
                                   (const int64_t *)nullptr, (const int64_t *)nullptr, nr, radius, (const int64_t *)(lims_dev + lo), ref_id_offset,
                                   out_dist_dev, out_ids_dev);
            VSC_CHECK_LAUNCH();
        }
        if (pass == 0) {
            VSC_TRY(range_total(counts, nq, lims_dev, capacity, total_out, &fill, stream));
            if (!fill) break;
        }
    }
    return VSC_OK;
}
