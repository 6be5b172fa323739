// Descriptor-track micro-AP on the device (VSC22-Descriptor-Track-1st/infer/vsc/metrics.py:423-494: average_precision and, through
// drivendata_average_precision, sklearn's average_precision_score).  The contracts are stated with vsc_uap_rank_f64 /
// vsc_uap_curve_f64 in include/vsc_hip.h (executable form: tests/uap_contract.py).  Pairs travel as 64-bit keys that the host
// interned; everything else the reference does with sorted(), sets, a merge and cumsum is here:
//  vsc_uap_rank_f64
//   (a) stable ascending LSD radix sort (8-bit digits) of the order-preserving 64-bit image of -score with the input position as
//       payload: the order of sorted(reverse=True) and argsort(-s, kind="mergesort").  The sort is scan_sort.h's, on 64-bit keys.
//   (b) the same sort, keys only and only the passes below key_bits, of the prediction keys and of the ground-truth keys, each
//       followed by a count of adjacent equal keys: the duplicates the reference detects with sets.
//   (c) one binary search per ranked prediction in the sorted ground truth: `correct`.
//  vsc_uap_curve_f64
//   (d) per tile of 2048 rows the numbers of correct rows and of tie-group ends, one exclusive scan over the tiles, and a second
//       sweep that turns the in-tile scans into cum_i and the group index: precision / recall / score at the correct rows, the
//       term precision_i * correct_i of every row, and (tps, last row) of every tie group.
//   (e) the tie groups' terms (R_j - R_{j-1}) P_j, written REVERSED, as sklearn holds its curve.
//   (f) two sums in np.sum's order.  numpy's reduction hands its inner loop at most 8192 elements at a time (its buffer size) and
//       adds the chunks' sums one after the other, starting from 0.0; inside a chunk the sum is pairwise: a node longer than 128
//       splits at n2 = n / 2, n2 -= n2 % 8, anything else is a leaf summed with eight interleaved accumulators.  A node's children
//       differ from half its length by less than 8, so the leaves sit at (nearly) one depth D <= 8, and the tree embeds into the
//       complete binary tree of depth D: one workgroup per chunk, thread i walks from the root along the bits of i, finds the leaf
//       it ends in, and -- if i is the least index that ends there -- sums it into slot i of LDS; a node of depth d at slot
//       p << (D - d) shares the slot of its left child, so combining a level is slot = slot + (slot + half) for the nodes that
//       exist and are no leaves (leaf depth of the slot > d).  One thread then adds the chunks in order.  The group count exists
//       only on the device: every workgroup derives its chunk, D and the walks from the length it reads there.
// Integer atomics only count (histogram bins and the four status counters); every output position is a scan result and every
// floating-point sum has a fixed association, so the outputs are a pure function of the inputs.  Both entries take a handle made
// on the caller's stream (as the segment-metric and score-normalisation entries do) and only enqueue on it.  Divisions are IEEE fp64
// divisions of exactly representable integers; nothing is contracted.  No 16-bit operands: one object for both builds of the library.
#include "common.h"
#include "scan_sort.h"

// contract arithmetic: every product, difference and sum rounded on its own
#pragma clang fp contract(off)

namespace {

constexpr int UAP_THREADS = 256;
constexpr int UAP_ITEMS = 8;                      // consecutive rows of one thread in the tile passes: (tile, thread, item) is row order
constexpr int UAP_TILE = VSC_UAP_TILE;
static_assert(UAP_TILE == UAP_THREADS * UAP_ITEMS, "tile = threads x items");
constexpr int UAP_SCAN_THREADS = 512;
constexpr int UAP_PW_LEAF = 128;                  // numpy's PW_BLOCKSIZE
constexpr int UAP_PW_CHUNK = 8192;                // numpy's reduction hands its inner loop at most this many elements (its buffer size)
constexpr int UAP_PW_LOCAL = 8;                   // a chunk's tree has at most this many levels below the root (2^8 = UAP_THREADS slots)
constexpr int UAP_NO_LEAF = 255;

struct UapCounters {
    unsigned nonfinite, dup_pred, dup_gt, n_pos;
};

__device__ inline uint64_t f64_bits(double x) {
    uint64_t u;
    memcpy(&u, &x, sizeof u);
    return u;
}

// ---- (a) the sort key: ascending key <=> descending score; -0.0 and +0.0 share a key -------------------------------------------
struct UapBuildArgs {
    const double *scores;
    int64_t n;
    uint64_t *keys;
    unsigned *nonfinite;
    int grid;
};

__global__ __launch_bounds__(UAP_THREADS) void uap_build_kernel(UapBuildArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * UAP_THREADS + threadIdx.x; i < a.n; i += (int64_t)a.grid * UAP_THREADS) {
        uint64_t u = f64_bits(a.scores[i]);
        if (((u >> 52) & 0x7FFu) == 0x7FFu) atomicAdd(a.nonfinite, 1u);
        u ^= 0x8000000000000000ull;                                  // -score
        if (u == 0x8000000000000000ull) u = 0ull;
        a.keys[i] = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    }
}

// ---- (b) adjacent equal keys of a sorted list ---------------------------------------------------------------------------------------
struct UapDupArgs {
    const uint64_t *keys;
    int64_t n;
    unsigned *count;
    int grid;
};

__global__ __launch_bounds__(UAP_THREADS) void uap_dup_kernel(UapDupArgs a) {
    const int lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * UAP_THREADS; base < a.n; base += (int64_t)a.grid * UAP_THREADS) {
        const int64_t i = base + threadIdx.x;
        const bool dup = i >= 1 && i < a.n && a.keys[i] == a.keys[i - 1];
        const unsigned long long b = __ballot(dup);
        if (lane == 0 && b) atomicAdd(a.count, (unsigned)__popcll(b));
    }
}

// ---- (c) the join -------------------------------------------------------------------------------------------------------------------
struct UapJoinArgs {
    const double *scores;
    const uint64_t *pred_keys, *gt_sorted;
    const int64_t *perm_sorted;
    int64_t n, g;
    int64_t *perm;
    double *ranked;
    uint8_t *correct;
    unsigned *n_pos;
    int grid;
};

__global__ __launch_bounds__(UAP_THREADS) void uap_join_kernel(UapJoinArgs a) {
    const int lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * UAP_THREADS; base < a.n; base += (int64_t)a.grid * UAP_THREADS) {
        const int64_t i = base + threadIdx.x;
        bool hit = false;
        if (i < a.n) {
            const int64_t p = a.perm_sorted[i];
            const uint64_t key = a.pred_keys[p];
            int64_t lo = 0, hi = a.g;
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if (a.gt_sorted[mid] < key) lo = mid + 1;
                else hi = mid;
            }
            hit = lo < a.g && a.gt_sorted[lo] == key;
            a.perm[i] = p;
            a.ranked[i] = a.scores[p];
            a.correct[i] = hit ? 1 : 0;
        }
        const unsigned long long b = __ballot(hit);
        if (lane == 0 && b) atomicAdd(a.n_pos, (unsigned)__popcll(b));
    }
}

struct UapStatusArgs {
    const UapCounters *cnt;
    int64_t *status;
};

__global__ void uap_status_kernel(UapStatusArgs a) {
    if (threadIdx.x != 0) return;
    a.status[0] = a.cnt->nonfinite;
    a.status[1] = a.cnt->dup_pred;
    a.status[2] = a.cnt->dup_gt;
    a.status[3] = a.cnt->n_pos;
}

// ---- (d) the curve --------------------------------------------------------------------------------------------------------------------
struct UapCurveArgs {
    const double *s;           // ranked scores
    const uint8_t *correct;
    int64_t n, n_gt, nb;
    unsigned *blk;             // [nb] correct rows per tile, [nb] group ends per tile, then the two totals {n_pos, n_groups}
    double *curve;             // [3][n]
    double *terms_p;           // [n]: precision_i * correct_i
    unsigned *gtps, *glast;    // [n] each, the first n_groups written: cum and row at the end of every tie group
};

// per-thread counts of one tile packed as (correct << 16 | group ends): a tile holds 2048 rows, neither field can carry
__device__ inline unsigned uap_curve_flags(const UapCurveArgs &a, int64_t p0, unsigned *packed) {
    unsigned bits = 0, pk = 0;
#pragma unroll
    for (int j = 0; j < UAP_ITEMS; ++j) {
        const int64_t i = p0 + j;
        if (i < a.n) {
            if (a.correct[i]) {
                bits |= 1u << (2 * j);
                pk += 0x10000u;
            }
            if (i == a.n - 1 || a.s[i] != a.s[i + 1]) {
                bits |= 2u << (2 * j);
                pk += 1u;
            }
        }
    }
    *packed = pk;
    return bits;
}

__global__ __launch_bounds__(UAP_THREADS) void uap_curve_count_kernel(UapCurveArgs a) {
    __shared__ unsigned wsum[UAP_THREADS / 64];
    unsigned packed, tot;
    uap_curve_flags(a, (int64_t)blockIdx.x * UAP_TILE + (int64_t)threadIdx.x * UAP_ITEMS, &packed);
    block_scan_excl<UAP_THREADS>(packed, wsum, &tot);
    if (threadIdx.x == 0) {
        a.blk[blockIdx.x] = tot >> 16;
        a.blk[a.nb + blockIdx.x] = tot & 0xFFFFu;
    }
}

__global__ __launch_bounds__(UAP_THREADS) void uap_curve_rows_kernel(UapCurveArgs a) {
    __shared__ unsigned wsum[UAP_THREADS / 64];
    const int64_t p0 = (int64_t)blockIdx.x * UAP_TILE + (int64_t)threadIdx.x * UAP_ITEMS;
    unsigned packed, tot;
    const unsigned bits = uap_curve_flags(a, p0, &packed);
    const unsigned ex = block_scan_excl<UAP_THREADS>(packed, wsum, &tot);
    unsigned cum = a.blk[blockIdx.x] + (ex >> 16);              // correct rows before this one
    unsigned grp = a.blk[a.nb + blockIdx.x] + (ex & 0xFFFFu);   // tie groups that ended before this one
    const double n_gt = (double)a.n_gt;
#pragma unroll
    for (int j = 0; j < UAP_ITEMS; ++j) {
        const int64_t i = p0 + j;
        if (i >= a.n) break;
        double term = 0.0;
        if ((bits >> (2 * j)) & 1u) {
            ++cum;
            const int64_t pos = (int64_t)cum - 1;
            term = (double)cum / (double)(i + 1);
            a.curve[pos] = term;
            a.curve[a.n + pos] = (double)cum / n_gt;
            a.curve[2 * a.n + pos] = a.s[i];
        }
        a.terms_p[i] = term;
        if ((bits >> (2 * j)) & 2u) {
            a.gtps[grp] = cum;
            a.glast[grp] = (unsigned)i;
            ++grp;
        }
    }
}

// ---- (e) the tie groups' terms, last group first ----------------------------------------------------------------------------------------
struct UapTermArgs {
    const unsigned *gtps, *glast;
    const unsigned *totals;    // {n_pos, n_groups}
    double *terms_a;           // [n], the first n_groups written
    int64_t *counts;
    int grid;
};

__global__ __launch_bounds__(UAP_THREADS) void uap_terms_kernel(UapTermArgs a) {
    const unsigned n_pos = a.totals[0];
    const int64_t groups = a.totals[1];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.counts[0] = n_pos;
        a.counts[1] = groups;
    }
    const double last = (double)n_pos;
    for (int64_t j = (int64_t)blockIdx.x * UAP_THREADS + threadIdx.x; j < groups; j += (int64_t)a.grid * UAP_THREADS) {
        const double tps = (double)a.gtps[j];
        const double r = n_pos ? tps / last : 0.0;
        const double r_prev = (n_pos && j) ? (double)a.gtps[j - 1] / last : 0.0;
        const double p = tps / (double)((int64_t)a.glast[j] + 1);
        a.terms_a[groups - 1 - j] = (r - r_prev) * p;
    }
}

// ---- (f) numpy's pairwise sum -----------------------------------------------------------------------------------------------------------
// a depth no leaf lies below: a child is at most (len + 1) / 2 + 7 long
__device__ __host__ constexpr int uap_pw_depth(int64_t len) {
    int d = 0;
    while (len > UAP_PW_LEAF) {
        len = (len + 1) / 2 + 7;
        ++d;
    }
    return d;
}

static_assert(uap_pw_depth(UAP_PW_CHUNK) <= UAP_PW_LOCAL, "a chunk's tree fits the workgroup (the depth bound grows with the length)");
inline int64_t uap_pw_chunks(int64_t len) { return len <= 0 ? 1 : (len + UAP_PW_CHUNK - 1) / UAP_PW_CHUNK; }

__device__ inline double uap_pw_leaf_sum(const double *a, int64_t n) {
    if (n < 8) {
        double res = 0.0;
        for (int64_t i = 0; i < n; ++i) res += a[i];
        return res;
    }
    double r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = a[k];
    int64_t i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] += a[i + k];
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}

struct UapPwArgs {
    const double *a;
    const unsigned *len_dev;   // the length, on the device; null: len_host
    int64_t len_host;
    double *chunks;            // one value per chunk of UAP_PW_CHUNK terms
    double *out;
};

__device__ inline int64_t uap_pw_len(const UapPwArgs &a) { return a.len_dev ? (int64_t)*a.len_dev : a.len_host; }

// one workgroup per chunk; the grid is sized for the host's bound of the length
__global__ __launch_bounds__(UAP_THREADS) void uap_pw_chunk_kernel(UapPwArgs a) {
    __shared__ double v[UAP_THREADS];
    __shared__ unsigned char ld[UAP_THREADS];
    const int64_t total = uap_pw_len(a);
    const int64_t begin = (int64_t)blockIdx.x * UAP_PW_CHUNK;
    if (begin >= total) return;
    const int64_t len = total - begin < UAP_PW_CHUNK ? total - begin : UAP_PW_CHUNK;
    const int D = uap_pw_depth(len);               // <= UAP_PW_LOCAL: the slots of a chunk's tree fit the workgroup
    const int tid = threadIdx.x;
    double val = 0.0;
    int depth = UAP_NO_LEAF;
    if (tid < (1 << D)) {
        int64_t off = begin, l = len;
        int d = 0;
        while (l > UAP_PW_LEAF) {
            int64_t n2 = l / 2;
            n2 -= n2 % 8;
            if ((tid >> (D - 1 - d)) & 1) {
                off += n2;
                l -= n2;
            } else {
                l = n2;
            }
            ++d;
        }
        depth = d;
        if ((tid & ((1 << (D - d)) - 1)) == 0) val = uap_pw_leaf_sum(a.a + off, l);
    }
    v[tid] = val;
    ld[tid] = (unsigned char)depth;
    __syncthreads();
    for (int d = D - 1; d >= 0; --d) {
        const int stride = 1 << (D - d);
        if ((tid & (stride - 1)) == 0 && ld[tid] != UAP_NO_LEAF && (int)ld[tid] > d) v[tid] = v[tid] + v[tid + (stride >> 1)];
        __syncthreads();
    }
    if (tid == 0) a.chunks[blockIdx.x] = v[0];
}

// the chunks one after the other, starting from the identity 0.0 as numpy's reduction does
__global__ void uap_pw_total_kernel(UapPwArgs a) {
    if (threadIdx.x != 0) return;
    const int64_t total = uap_pw_len(a);
    double res = 0.0;
    for (int64_t c = 0; c * UAP_PW_CHUNK < total; ++c) res += a.chunks[c];
    *a.out = res;
}

int uap_pairwise(const double *terms, const unsigned *len_dev, int64_t len_bound, double *chunks, double *out, hipStream_t stream) {
    UapPwArgs a = {terms, len_dev, len_bound, chunks, out};
    hipLaunchKernelGGL(uap_pw_chunk_kernel, dim3((unsigned)uap_pw_chunks(len_bound)), dim3(UAP_THREADS), 0, stream, a);
    VSC_CHECK_LAUNCH();
    hipLaunchKernelGGL(uap_pw_total_kernel, dim3(1), dim3(64), 0, stream, a);
    VSC_CHECK_LAUNCH();
    return VSC_OK;
}

// the shared sort as this file uses it: the length on the host, positions (or nothing) as the payload
constexpr auto uap_sort = radix_sort<UAP_SCAN_THREADS, uint64_t, int64_t>;

}  // namespace

// the handle: the stream every call enqueues on; it owns no device memory (the scratch is the search's)
struct vsc_uap {
    hipStream_t stream;
};

extern "C" int vsc_uap_create(void *stream, vsc_uap **out) {
    VSC_REQUIRE(out, "uap_create: null pointer");
    *out = new vsc_uap{(hipStream_t)stream};
    return VSC_OK;
}

extern "C" void vsc_uap_destroy(vsc_uap *h) { delete h; }

extern "C" int vsc_uap_rank_f64(vsc_uap *h, const double *scores_dev, const uint64_t *pred_keys_dev, int64_t n, const uint64_t *gt_keys_dev,
                                int64_t g, int32_t key_bits, int64_t *perm_dev, double *scores_ranked_dev, uint8_t *correct_dev,
                                int64_t *status_dev) {
    VSC_REQUIRE(h, "uap_rank: null handle");
    hipStream_t stream = h->stream;
    VSC_REQUIRE(n >= 0 && n < (1ll << 31), "uap_rank: n = %lld outside [0, 2^31)", (long long)n);
    VSC_REQUIRE(g >= 0 && g < (1ll << 31), "uap_rank: g = %lld outside [0, 2^31)", (long long)g);
    VSC_REQUIRE(key_bits >= 1 && key_bits <= 64, "uap_rank: key_bits = %d outside [1, 64]", key_bits);
    if (n == 0) return VSC_OK;
    VSC_REQUIRE(scores_dev && pred_keys_dev && perm_dev && scores_ranked_dev && correct_dev && status_dev, "uap_rank: null pointer");
    VSC_REQUIRE(gt_keys_dev || g == 0, "uap_rank: null ground truth with g = %lld", (long long)g);
    const int64_t stride = n > g ? n : g;
    UapCounters *cnt;
    uint64_t *keys;
    int64_t *pay;
    VSC_TRY(search_scratch_get(SCRATCH_UAP_STATE, sizeof(UapCounters), &cnt));
    VSC_TRY(search_scratch_get(SCRATCH_UAP_KEYS, (size_t)stride * 2 * 8, &keys));
    VSC_TRY(search_scratch_get(SCRATCH_UAP_PAY, (size_t)n * 3 * 8, &pay));
    unsigned *hist;
    const int64_t tiles = sort_tiles(n) > sort_tiles(g) ? sort_tiles(n) : sort_tiles(g);
    VSC_TRY(search_scratch_get(SCRATCH_UAP_HIST, (size_t)tiles * 256 * 4, &hist));
    uint64_t *score_keys = (uint64_t *)(pay + 2 * n);               // the sort's input; its two key buffers are `keys`
    VSC_CHECK_HIP(hipMemsetAsync(cnt, 0, sizeof(UapCounters), stream));
    const int sweep = grid_for(n, UAP_THREADS, 2048);
    UapBuildArgs b = {scores_dev, n, score_keys, &cnt->nonfinite, sweep};
    hipLaunchKernelGGL(uap_build_kernel, dim3(sweep), dim3(UAP_THREADS), 0, stream, b);
    VSC_CHECK_LAUNCH();
    const uint64_t *sorted;
    const int64_t *perm_sorted;
    VSC_TRY(uap_sort(score_keys, nullptr, nullptr, n, 64, keys, pay, n, hist, stream, &sorted, &perm_sorted));
    VSC_TRY(uap_sort(pred_keys_dev, nullptr, nullptr, n, key_bits, keys, nullptr, stride, hist, stream, &sorted, nullptr));
    UapDupArgs dp = {sorted, n, &cnt->dup_pred, sweep};
    hipLaunchKernelGGL(uap_dup_kernel, dim3(sweep), dim3(UAP_THREADS), 0, stream, dp);
    VSC_CHECK_LAUNCH();
    sorted = nullptr;
    if (g) {
        VSC_TRY(uap_sort(gt_keys_dev, nullptr, nullptr, g, key_bits, keys, nullptr, stride, hist, stream, &sorted, nullptr));
        const int gsweep = grid_for(g, UAP_THREADS, 2048);
        UapDupArgs dg = {sorted, g, &cnt->dup_gt, gsweep};
        hipLaunchKernelGGL(uap_dup_kernel, dim3(gsweep), dim3(UAP_THREADS), 0, stream, dg);
        VSC_CHECK_LAUNCH();
    }
    UapJoinArgs j = {scores_dev, pred_keys_dev, sorted, perm_sorted, n, g, perm_dev, scores_ranked_dev, correct_dev, &cnt->n_pos, sweep};
    hipLaunchKernelGGL(uap_join_kernel, dim3(sweep), dim3(UAP_THREADS), 0, stream, j);
    VSC_CHECK_LAUNCH();
    UapStatusArgs s = {cnt, status_dev};
    hipLaunchKernelGGL(uap_status_kernel, dim3(1), dim3(64), 0, stream, s);
    VSC_CHECK_LAUNCH();
    return VSC_OK;
}

extern "C" int vsc_uap_curve_f64(vsc_uap *h, const double *scores_ranked_dev, const uint8_t *correct_dev, int64_t n, int64_t n_gt,
                                 double *sums_dev, int64_t *counts_dev, double *curve_dev) {
    VSC_REQUIRE(h, "uap_curve: null handle");
    hipStream_t stream = h->stream;
    VSC_REQUIRE(n >= 0 && n < (1ll << 31), "uap_curve: n = %lld outside [0, 2^31)", (long long)n);
    VSC_REQUIRE(n_gt >= 1, "uap_curve: n_gt = %lld", (long long)n_gt);
    if (n == 0) return VSC_OK;
    VSC_REQUIRE(scores_ranked_dev && correct_dev && sums_dev && counts_dev && curve_dev, "uap_curve: null pointer");
    const int64_t nb = (n + UAP_TILE - 1) / UAP_TILE;
    const int64_t chunks_n = uap_pw_chunks(n);
    unsigned *blk, *groups;
    double *terms, *slots;
    VSC_TRY(search_scratch_get(SCRATCH_UAP_HIST, (size_t)(2 * nb + 2) * 4, &blk));
    VSC_TRY(search_scratch_get(SCRATCH_UAP_PAY, (size_t)n * 2 * 4, &groups));
    VSC_TRY(search_scratch_get(SCRATCH_UAP_KEYS, (size_t)n * 2 * 8, &terms));
    VSC_TRY(search_scratch_get(SCRATCH_UAP_TREE, (size_t)chunks_n * 8, &slots));
    UapCurveArgs c = {scores_ranked_dev, correct_dev, n, n_gt, nb, blk, curve_dev, terms + n, groups, groups + n};
    hipLaunchKernelGGL(uap_curve_count_kernel, dim3((unsigned)nb), dim3(UAP_THREADS), 0, stream, c);
    VSC_CHECK_LAUNCH();
    VSC_TRY(scan_runs<UAP_SCAN_THREADS>(blk, nb, 2, blk + 2 * nb, stream));
    hipLaunchKernelGGL(uap_curve_rows_kernel, dim3((unsigned)nb), dim3(UAP_THREADS), 0, stream, c);
    VSC_CHECK_LAUNCH();
    const int sweep = grid_for(n, UAP_THREADS, 2048);
    UapTermArgs t = {groups, groups + n, blk + 2 * nb, terms, counts_dev, sweep};
    hipLaunchKernelGGL(uap_terms_kernel, dim3(sweep), dim3(UAP_THREADS), 0, stream, t);
    VSC_CHECK_LAUNCH();
    VSC_TRY(uap_pairwise(terms, blk + 2 * nb + 1, n, slots, sums_dev, stream));
    VSC_TRY(uap_pairwise(terms + n, nullptr, n, slots, sums_dev + 1, stream));
    return VSC_OK;
}
