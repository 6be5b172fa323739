// Global top-k of frame pairs and their grouping into video pairs (infer/vsc/index.py:145-165, infer/vsc/candidates.py:24-40):
// what the host did with a stable sort, a cut and np.unique over the search's probe, as exact and deterministic device passes.
// Contracts: vsc_global_topk_f32 / vsc_pair_first_hits in include/vsc_hip.h (executable form: tests/global_topk_contract.py).
//
// vsc_global_topk_f32, n entries, `want` asked for, m = min(want, valid) selected:
//  (A) select   4 x (digit histogram of the order-preserving 32-bit score key over the entries that match the key bits decided so
//               far; one thread picks the digit that holds the want-th key)            4 x (12 n bytes read), 4 KiB of counters
//               -> threshold key T and the number of entries equal to T that still fit.
//  (B) compact  per 2048-entry tile: (above T, equal to T) counts; exclusive scan over the tiles; scatter (~key, position) of
//               every entry above T and of the first `fit` entries equal to T, in input order   2 x 12 n read, 8 m written
//  (C) order    stable LSD radix sort of the m survivors by ~key (scan_sort.h), m read on the device 4 x (12 m read, 8 m written)
//  (D) gather   rows / ids / scores through the position payload                                      4 m read, 20 m written
// Integer atomics only count (LDS and global histogram bins); every output position is a scan result, so the output is a pure
// function of the input.  Nothing synchronises the host: the count stays on the device.
//
// vsc_pair_first_hits: an open-addressing table keyed by the 64-bit video-pair key holds the atomicMin of the positions that
// carry it -- which slot a key settles in depends on arrival order, the minimum does not --, a flag pass marks the entries that
// ARE their pair's minimum, and the same tile count / scan / scatter writes the first `limit` flagged positions in ascending order.
// Every kernel takes one argument struct, its grid in it where it strides by the grid: the form the host emulation launches.
#include "common.h"
#include "scan_sort.h"

namespace {

constexpr int GT_THREADS = 256;
constexpr int GT_ITEMS = 8;                       // consecutive entries of one thread in the tile passes: (tile, thread, item) is input order
constexpr int GT_TILE = VSC_GLOBAL_TOPK_TILE;
static_assert(GT_TILE == GT_THREADS * GT_ITEMS, "tile = threads x items");
constexpr int GT_SCAN_THREADS = 1024;
constexpr unsigned GT_ALL = 0xFFFFFFFFu;          // "every entry equal to the threshold fits" (counts stay below 2^31)

struct GtState {
    unsigned hist[4][256];   // (A): digit histogram of every pass
    unsigned prefix;         // key bits decided so far; after pass 3 the threshold key T
    unsigned remaining;      // entries still to take among the keys matching `prefix`; after pass 3: entries equal to T that fit
    unsigned take_all;       // valid <= want: everything valid is selected (T = 0, remaining = GT_ALL)
    unsigned count;          // m
};

// larger score <=> larger key; -0.0 and +0.0 share a key.  NaN is outside the contract (it would order by its bit pattern).
__device__ inline unsigned score_key(float s) {
    unsigned u = __float_as_uint(s);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ---- (A) radix select ----------------------------------------------------------------------------------------------------------
struct GtSelectArgs {
    const float *scores;
    const int64_t *ids;
    int64_t n;
    int pass;
    unsigned want;
    GtState *st;
    int64_t *out_count;
    int grid;
};

__global__ __launch_bounds__(GT_THREADS) void gt_select_hist_kernel(GtSelectArgs a) {
    __shared__ unsigned h[256];
    if (a.st->take_all) return;
    const int tid = threadIdx.x;
    h[tid] = 0u;
    __syncthreads();
    const int shift = 24 - 8 * a.pass;
    const unsigned himask = a.pass == 0 ? 0u : 0xFFFFFFFFu << (shift + 8);
    const unsigned prefix = a.st->prefix & himask;
    for (int64_t p = (int64_t)blockIdx.x * GT_THREADS + tid; p < a.n; p += (int64_t)a.grid * GT_THREADS) {
        if (a.ids[p] < 0) continue;
        const unsigned k = score_key(a.scores[p]);
        if ((k & himask) == prefix) atomicAdd(&h[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (h[tid]) atomicAdd(&a.st->hist[a.pass][tid], h[tid]);
}

__global__ void gt_select_pick_kernel(GtSelectArgs a) {
    GtState *st = a.st;
    if (threadIdx.x != 0 || st->take_all) return;
    unsigned rem = st->remaining;
    if (a.pass == 0) {
        unsigned valid = 0;
        for (int b = 0; b < 256; ++b) valid += st->hist[0][b];
        if (valid <= a.want) {
            st->take_all = 1u;
            st->prefix = 0u;
            st->remaining = GT_ALL;
            st->count = valid;
            *a.out_count = (int64_t)valid;
            return;
        }
        st->count = a.want;
        *a.out_count = (int64_t)a.want;
        rem = a.want;
    }
    // the highest digit whose bin, together with the bins above it, reaches `rem`: more than `rem` entries match the prefix, so one does
    unsigned above = 0;
    int b = 255;
    for (; b > 0; --b) {
        const unsigned c = st->hist[a.pass][b];
        if (above + c >= rem) break;
        above += c;
    }
    st->prefix |= (unsigned)b << (24 - 8 * a.pass);
    st->remaining = rem - above;
}

// ---- (B) stable compaction -----------------------------------------------------------------------------------------------------
struct GtCompactArgs {
    const float *scores;
    const int64_t *ids;
    int64_t n;
    const GtState *st;
    unsigned *blk;             // [nb] entries above T per tile, [nb] entries equal to T per tile
    int64_t nb;
    unsigned *keys, *pay;
};

// per-thread counts of one tile packed as (above << 16 | equal): a tile holds 2048 entries, neither field can carry into the other
__global__ __launch_bounds__(GT_THREADS) void gt_compact_count_kernel(GtCompactArgs a) {
    __shared__ unsigned wsum[GT_THREADS / 64];
    const unsigned thr = a.st->prefix;
    const int64_t p0 = (int64_t)blockIdx.x * GT_TILE + (int64_t)threadIdx.x * GT_ITEMS;
    unsigned packed = 0;
#pragma unroll
    for (int j = 0; j < GT_ITEMS; ++j) {
        const int64_t p = p0 + j;
        if (p < a.n && a.ids[p] >= 0) {
            const unsigned k = score_key(a.scores[p]);
            packed += k > thr ? 0x10000u : (k == thr ? 1u : 0u);
        }
    }
    unsigned tot;
    block_scan_excl<GT_THREADS>(packed, wsum, &tot);
    if (threadIdx.x == 0) {
        a.blk[blockIdx.x] = tot >> 16;
        a.blk[a.nb + blockIdx.x] = tot & 0xFFFFu;
    }
}

__global__ __launch_bounds__(GT_THREADS) void gt_compact_scatter_kernel(GtCompactArgs a) {
    __shared__ unsigned wsum[GT_THREADS / 64];
    const unsigned thr = a.st->prefix, fit = a.st->remaining;
    const int64_t p0 = (int64_t)blockIdx.x * GT_TILE + (int64_t)threadIdx.x * GT_ITEMS;
    unsigned key[GT_ITEMS];
    unsigned kind = 0;          // 2 bits per item: 0 not selected, 1 equal to T, 2 above T
    unsigned packed = 0;
#pragma unroll
    for (int j = 0; j < GT_ITEMS; ++j) {
        const int64_t p = p0 + j;
        key[j] = 0u;
        if (p < a.n && a.ids[p] >= 0) {
            const unsigned k = score_key(a.scores[p]);
            key[j] = k;
            if (k > thr) {
                kind |= 2u << (2 * j);
                packed += 0x10000u;
            } else if (k == thr) {
                kind |= 1u << (2 * j);
                packed += 1u;
            }
        }
    }
    unsigned tot;
    const unsigned ex = block_scan_excl<GT_THREADS>(packed, wsum, &tot);
    unsigned above = a.blk[blockIdx.x] + (ex >> 16);            // entries above T before this one, in input order
    unsigned equal = a.blk[a.nb + blockIdx.x] + (ex & 0xFFFFu);  // entries equal to T before this one
#pragma unroll
    for (int j = 0; j < GT_ITEMS; ++j) {
        const unsigned kd = (kind >> (2 * j)) & 3u;
        if (kd == 2u) {
            const unsigned o = above + (equal < fit ? equal : fit);
            a.keys[o] = ~key[j];
            a.pay[o] = (unsigned)(p0 + j);
            ++above;
        } else if (kd == 1u) {
            if (equal < fit) {
                const unsigned o = above + equal;
                a.keys[o] = ~key[j];
                a.pay[o] = (unsigned)(p0 + j);
            }
            ++equal;
        }
    }
}

// ---- (D) ---------------------------------------------------------------------------------------------------------------------
struct GtGatherArgs {
    const float *scores;
    const int64_t *rows, *ids;
    int32_t row_stride;
    const unsigned *pay;
    const GtState *st;
    int64_t *out_rows, *out_ids;
    float *out_scores;
    int grid;
};

__global__ __launch_bounds__(GT_THREADS) void gt_gather_kernel(GtGatherArgs a) {
    const int64_t m = a.st->count;
    for (int64_t i = (int64_t)blockIdx.x * GT_THREADS + threadIdx.x; i < m; i += (int64_t)a.grid * GT_THREADS) {
        const int64_t p = a.pay[i];
        a.out_rows[i] = a.rows ? a.rows[p] : p / a.row_stride;
        a.out_ids[i] = a.ids[p];
        a.out_scores[i] = a.scores[p];
    }
}

// ---- vsc_pair_first_hits --------------------------------------------------------------------------------------------------------
constexpr unsigned long long PFH_EMPTY = ~0ull;

struct PfhArgs {
    const int64_t *rows, *ids;
    int64_t n;
    const int32_t *qv, *rv;
    int32_t nrv;
    unsigned long long *tkeys;
    unsigned *tpos;
    uint64_t mask;
    uint8_t *flags;
    unsigned *blk;             // [nb] flagged entries per tile, then their sum
    int64_t nb, limit;
    int64_t *out_pos, *out_count;
    int grid;                  // of the insert pass
};

__device__ inline uint64_t pfh_mix(uint64_t x) {   // splitmix64's finaliser
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// the pair key of entry p, or PFH_EMPTY for an entry that is no hit (a negative row or id: the search's padding)
__device__ inline unsigned long long pfh_key(const PfhArgs &a, int64_t p) {
    const int64_t row = a.rows[p], id = a.ids[p];
    if (row < 0 || id < 0) return PFH_EMPTY;
    return (unsigned long long)a.qv[row] * (unsigned long long)a.nrv + (unsigned long long)a.rv[id];
}

// the table holds at most n keys in >= 2 n slots: a probe sequence always ends at the key or at an empty slot
__global__ __launch_bounds__(GT_THREADS) void pfh_insert_kernel(PfhArgs a) {
    for (int64_t p = (int64_t)blockIdx.x * GT_THREADS + threadIdx.x; p < a.n; p += (int64_t)a.grid * GT_THREADS) {
        const unsigned long long key = pfh_key(a, p);
        if (key == PFH_EMPTY) continue;
        uint64_t h = pfh_mix(key) & a.mask;
        for (uint64_t step = 0; step <= a.mask; ++step) {
            const unsigned long long prev = atomicCAS(&a.tkeys[h], PFH_EMPTY, key);
            if (prev == PFH_EMPTY || prev == key) {
                atomicMin(&a.tpos[h], (unsigned)p);
                break;
            }
            h = (h + 1) & a.mask;
        }
    }
}

__global__ __launch_bounds__(GT_THREADS) void pfh_flag_count_kernel(PfhArgs a) {
    __shared__ unsigned wsum[GT_THREADS / 64];
    const int64_t p0 = (int64_t)blockIdx.x * GT_TILE + (int64_t)threadIdx.x * GT_ITEMS;
    unsigned mine = 0;
    for (int j = 0; j < GT_ITEMS; ++j) {
        const int64_t p = p0 + j;
        if (p >= a.n) break;
        const unsigned long long key = pfh_key(a, p);
        unsigned first = 0;
        if (key != PFH_EMPTY) {
            uint64_t h = pfh_mix(key) & a.mask;
            for (uint64_t step = 0; step <= a.mask; ++step) {
                const unsigned long long at = a.tkeys[h];
                if (at == key) {
                    first = a.tpos[h] == (unsigned)p ? 1u : 0u;
                    break;
                }
                if (at == PFH_EMPTY) break;     // (cannot happen after the insert pass: every key is in the table)
                h = (h + 1) & a.mask;
            }
        }
        a.flags[p] = (uint8_t)first;
        mine += first;
    }
    unsigned tot;
    block_scan_excl<GT_THREADS>(mine, wsum, &tot);
    if (threadIdx.x == 0) a.blk[blockIdx.x] = tot;
}

// blk: exclusive scan of the tiles' counts, blk[nb] their sum
__global__ __launch_bounds__(GT_THREADS) void pfh_scatter_kernel(PfhArgs a) {
    __shared__ unsigned wsum[GT_THREADS / 64];
    const int64_t p0 = (int64_t)blockIdx.x * GT_TILE + (int64_t)threadIdx.x * GT_ITEMS;
    unsigned bits = 0, mine = 0;
#pragma unroll
    for (int j = 0; j < GT_ITEMS; ++j)
        if (p0 + j < a.n && a.flags[p0 + j]) {
            bits |= 1u << j;
            ++mine;
        }
    unsigned tot;
    int64_t o = (int64_t)a.blk[blockIdx.x] + block_scan_excl<GT_THREADS>(mine, wsum, &tot);
#pragma unroll
    for (int j = 0; j < GT_ITEMS; ++j)
        if ((bits >> j) & 1u) {
            if (o < a.limit) a.out_pos[o] = p0 + j;
            ++o;
        }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t total = a.blk[a.nb];
        *a.out_count = total < a.limit ? total : a.limit;
    }
}

}  // namespace

extern "C" int vsc_global_topk_f32(const float *scores_dev, const int64_t *rows_dev, const int64_t *ids_dev, int64_t n,
                                   int32_t row_stride, int64_t want, int64_t *out_rows_dev, int64_t *out_ids_dev,
                                   float *out_scores_dev, int64_t *out_count_dev, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    VSC_REQUIRE(out_count_dev, "global_topk: null count pointer");
    VSC_REQUIRE(n >= 0 && n < (1ll << 31), "global_topk: n = %lld outside [0, 2^31)", (long long)n);
    VSC_REQUIRE(want >= 0, "global_topk: want = %lld", (long long)want);
    if (n == 0 || want == 0) {
        VSC_CHECK_HIP(hipMemsetAsync(out_count_dev, 0, sizeof(int64_t), stream));
        return VSC_OK;
    }
    VSC_REQUIRE(scores_dev && ids_dev && out_rows_dev && out_ids_dev && out_scores_dev, "global_topk: null pointer");
    VSC_REQUIRE(rows_dev || row_stride >= 1, "global_topk: row_stride = %d without a row array", row_stride);
    const int64_t mb = want < n ? want : n;                       // upper bound of m: sizes the buffers and grids of (C) and (D)
    const int64_t nb = (n + GT_TILE - 1) / GT_TILE;
    GtState *st;
    unsigned *blk, *keys, *pay, *hist;
    VSC_TRY(search_scratch_get(SCRATCH_GTK_STATE, sizeof(GtState), &st));
    VSC_TRY(search_scratch_get(SCRATCH_GTK_BLOCKS, (size_t)nb * 2 * 4, &blk));
    VSC_TRY(search_scratch_get(SCRATCH_GTK_KEYS, (size_t)mb * 2 * 4, &keys));
    VSC_TRY(search_scratch_get(SCRATCH_GTK_PAY, (size_t)mb * 2 * 4, &pay));
    VSC_TRY(search_scratch_get(SCRATCH_GTK_HIST, (size_t)sort_tiles(mb) * 256 * 4, &hist));
    VSC_CHECK_HIP(hipMemsetAsync(st, 0, sizeof(GtState), stream));
    GtSelectArgs sel = {scores_dev, ids_dev, n, 0, (unsigned)mb, st, out_count_dev, grid_for(n, GT_THREADS, 1024)};
    for (sel.pass = 0; sel.pass < 4; ++sel.pass) {
        hipLaunchKernelGGL(gt_select_hist_kernel, dim3(sel.grid), dim3(GT_THREADS), 0, stream, sel);
        VSC_CHECK_LAUNCH();
        hipLaunchKernelGGL(gt_select_pick_kernel, dim3(1), dim3(64), 0, stream, sel);
        VSC_CHECK_LAUNCH();
    }
    GtCompactArgs c = {scores_dev, ids_dev, n, st, blk, nb, keys, pay};
    hipLaunchKernelGGL(gt_compact_count_kernel, dim3((unsigned)nb), dim3(GT_THREADS), 0, stream, c);
    VSC_CHECK_LAUNCH();
    VSC_TRY(scan_runs<GT_SCAN_THREADS>(blk, nb, 2, nullptr, stream));
    hipLaunchKernelGGL(gt_compact_scatter_kernel, dim3((unsigned)nb), dim3(GT_THREADS), 0, stream, c);
    VSC_CHECK_LAUNCH();
    const unsigned *sorted, *order;                               // 4 passes: both end in the buffers they started from
    VSC_TRY(radix_sort<GT_SCAN_THREADS>((const unsigned *)keys, (const unsigned *)pay, &st->count, mb, 32, keys, pay, mb, hist, stream,
                                        &sorted, &order));
    GtGatherArgs g = {scores_dev, rows_dev, ids_dev, row_stride, order, st, out_rows_dev, out_ids_dev, out_scores_dev,
                      grid_for(mb, GT_THREADS, 2048)};
    hipLaunchKernelGGL(gt_gather_kernel, dim3(g.grid), dim3(GT_THREADS), 0, stream, g);
    VSC_CHECK_LAUNCH();
    return VSC_OK;
}

extern "C" int vsc_pair_first_hits(const int64_t *rows_dev, const int64_t *ids_dev, int64_t n, const int32_t *q_video_dev,
                                   const int32_t *r_video_dev, int32_t n_r_videos, int64_t limit, int64_t *out_pos_dev,
                                   int64_t *out_count_dev, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    VSC_REQUIRE(out_count_dev, "pair_first_hits: null count pointer");
    VSC_REQUIRE(n >= 0 && n < (1ll << 31), "pair_first_hits: n = %lld outside [0, 2^31)", (long long)n);
    if (limit < 0 || limit > n) limit = n;
    if (n == 0 || limit == 0) {
        VSC_CHECK_HIP(hipMemsetAsync(out_count_dev, 0, sizeof(int64_t), stream));
        return VSC_OK;
    }
    VSC_REQUIRE(rows_dev && ids_dev && q_video_dev && r_video_dev && out_pos_dev, "pair_first_hits: null pointer");
    VSC_REQUIRE(n_r_videos >= 1, "pair_first_hits: n_r_videos = %d", n_r_videos);
    uint64_t slots = 64;
    while (slots < 2 * (uint64_t)n) slots <<= 1;
    const int64_t nb = (n + GT_TILE - 1) / GT_TILE;
    unsigned long long *tkeys;
    unsigned *tpos, *blk;
    uint8_t *flags;
    VSC_TRY(search_scratch_get(SCRATCH_PFH_KEYS, (size_t)slots * 8, &tkeys));
    VSC_TRY(search_scratch_get(SCRATCH_PFH_POS, (size_t)slots * 4, &tpos));
    VSC_TRY(search_scratch_get(SCRATCH_PFH_FLAGS, (size_t)n, &flags));
    VSC_TRY(search_scratch_get(SCRATCH_PFH_BLOCKS, (size_t)(nb + 1) * 4, &blk));
    VSC_CHECK_HIP(hipMemsetAsync(tkeys, 0xFF, (size_t)slots * 8, stream));
    VSC_CHECK_HIP(hipMemsetAsync(tpos, 0xFF, (size_t)slots * 4, stream));
    PfhArgs a = {rows_dev, ids_dev, n, q_video_dev, r_video_dev, n_r_videos, tkeys, tpos, slots - 1, flags, blk, nb, limit, out_pos_dev,
                 out_count_dev, grid_for(n, GT_THREADS, 2048)};
    hipLaunchKernelGGL(pfh_insert_kernel, dim3(a.grid), dim3(GT_THREADS), 0, stream, a);
    VSC_CHECK_LAUNCH();
    hipLaunchKernelGGL(pfh_flag_count_kernel, dim3((unsigned)nb), dim3(GT_THREADS), 0, stream, a);
    VSC_CHECK_LAUNCH();
    VSC_TRY(scan_runs<GT_SCAN_THREADS>(blk, nb, 1, blk + nb, stream));
    hipLaunchKernelGGL(pfh_scatter_kernel, dim3((unsigned)nb), dim3(GT_THREADS), 0, stream, a);
    VSC_CHECK_LAUNCH();
    return VSC_OK;
}
