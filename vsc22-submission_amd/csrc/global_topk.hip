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
//  (C) order    stable LSD radix sort of the m survivors by ~key, 8-bit digits: per-tile digit histograms, one exclusive scan
//               over [digit][tile], stable in-tile ranking by wave ballots                     4 x (12 m read, 8 m written)
//  (D) gather   rows / ids / scores through the position payload                                      4 m read, 20 m written
// Integer atomics only count (LDS and global histogram bins); every output position is a scan result, so the output is a pure
// function of the input.  Nothing synchronises the host: the count stays on the device.
//
// vsc_pair_first_hits: an open-addressing table keyed by the 64-bit video-pair key holds the atomicMin of the positions that
// carry it -- which slot a key settles in depends on arrival order, the minimum does not --, a flag pass marks the entries that
// ARE their pair's minimum, and the same tile count / scan / scatter writes the first `limit` flagged positions in ascending order.
#include "common.h"

namespace {

constexpr int GT_THREADS = 256;
constexpr int GT_ITEMS = 8;                       // consecutive entries of one thread in the tile passes: (tile, thread, item) is input order
constexpr int GT_TILE = VSC_GLOBAL_TOPK_TILE;
static_assert(GT_TILE == GT_THREADS * GT_ITEMS, "tile = threads x items");
constexpr int GT_SCAN_THREADS = 1024;
constexpr int GT_MAX_SORT_TILES = 4096;           // the sort's tile grows beyond this many tiles: the [256][tiles] scan stays <= 1M counters
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

__device__ inline unsigned wave_scan_incl(unsigned v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// exclusive prefix of v over the workgroup's threads, *total = the sum; wsum: NT / 64 words of LDS (reusable across calls:
// the leading barrier orders a call behind the reads of the one before)
template <int NT>
__device__ inline unsigned block_scan_excl(unsigned v, unsigned *wsum, unsigned *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned inc = wave_scan_incl(v);
    __syncthreads();
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        const unsigned s = wsum[w];
        if (w < wave) base += s;
        tot += s;
    }
    *total = tot;
    return base + inc - v;
}

// exclusive scan in place of gridDim.x segments of `len` counters each, one workgroup per segment; totals (or null): [segments]
__global__ __launch_bounds__(GT_SCAN_THREADS) void gt_scan_kernel(unsigned *data, int64_t len, unsigned *totals) {
    __shared__ unsigned wsum[GT_SCAN_THREADS / 64];
    unsigned *d = data + (int64_t)blockIdx.x * len;
    unsigned carry = 0;
    for (int64_t base = 0; base < len; base += GT_SCAN_THREADS) {
        const int64_t i = base + threadIdx.x;
        const unsigned v = i < len ? d[i] : 0u;
        unsigned tot;
        const unsigned ex = block_scan_excl<GT_SCAN_THREADS>(v, wsum, &tot);
        if (i < len) d[i] = carry + ex;
        carry += tot;
    }
    if (totals && threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// ---- (A) radix select ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GT_THREADS) void gt_select_hist_kernel(const float *scores, const int64_t *ids, int64_t n, int pass,
                                                                    GtState *st) {
    __shared__ unsigned h[256];
    if (st->take_all) return;
    const int tid = threadIdx.x;
    h[tid] = 0u;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const unsigned himask = pass == 0 ? 0u : 0xFFFFFFFFu << (shift + 8);
    const unsigned prefix = st->prefix & himask;
    for (int64_t p = (int64_t)blockIdx.x * GT_THREADS + tid; p < n; p += (int64_t)gridDim.x * GT_THREADS) {
        if (ids[p] < 0) continue;
        const unsigned k = score_key(scores[p]);
        if ((k & himask) == prefix) atomicAdd(&h[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (h[tid]) atomicAdd(&st->hist[pass][tid], h[tid]);
}

__global__ void gt_select_pick_kernel(GtState *st, int pass, unsigned want, int64_t *out_count) {
    if (threadIdx.x != 0 || st->take_all) return;
    unsigned rem = st->remaining;
    if (pass == 0) {
        unsigned valid = 0;
        for (int b = 0; b < 256; ++b) valid += st->hist[0][b];
        if (valid <= want) {
            st->take_all = 1u;
            st->prefix = 0u;
            st->remaining = GT_ALL;
            st->count = valid;
            *out_count = (int64_t)valid;
            return;
        }
        st->count = want;
        *out_count = (int64_t)want;
        rem = want;
    }
    // the highest digit whose bin, together with the bins above it, reaches `rem`: more than `rem` entries match the prefix, so one does
    unsigned above = 0;
    int b = 255;
    for (; b > 0; --b) {
        const unsigned c = st->hist[pass][b];
        if (above + c >= rem) break;
        above += c;
    }
    st->prefix |= (unsigned)b << (24 - 8 * pass);
    st->remaining = rem - above;
}

// ---- (B) stable compaction -----------------------------------------------------------------------------------------------------
// per-thread counts of one tile packed as (above << 16 | equal): a tile holds 2048 entries, neither field can carry into the other
__global__ __launch_bounds__(GT_THREADS) void gt_compact_count_kernel(const float *scores, const int64_t *ids, int64_t n,
                                                                      const GtState *st, unsigned *blk, int64_t nb) {
    __shared__ unsigned wsum[GT_THREADS / 64];
    const unsigned thr = st->prefix;
    const int64_t p0 = (int64_t)blockIdx.x * GT_TILE + (int64_t)threadIdx.x * GT_ITEMS;
    unsigned packed = 0;
#pragma unroll
    for (int j = 0; j < GT_ITEMS; ++j) {
        const int64_t p = p0 + j;
        if (p < n && ids[p] >= 0) {
            const unsigned k = score_key(scores[p]);
            packed += k > thr ? 0x10000u : (k == thr ? 1u : 0u);
        }
    }
    unsigned tot;
    block_scan_excl<GT_THREADS>(packed, wsum, &tot);
    if (threadIdx.x == 0) {
        blk[blockIdx.x] = tot >> 16;
        blk[nb + blockIdx.x] = tot & 0xFFFFu;
    }
}

__global__ __launch_bounds__(GT_THREADS) void gt_compact_scatter_kernel(const float *scores, const int64_t *ids, int64_t n,
                                                                        const GtState *st, const unsigned *blk, int64_t nb,
                                                                        unsigned *keys, unsigned *pay) {
    __shared__ unsigned wsum[GT_THREADS / 64];
    const unsigned thr = st->prefix, fit = st->remaining;
    const int64_t p0 = (int64_t)blockIdx.x * GT_TILE + (int64_t)threadIdx.x * GT_ITEMS;
    unsigned key[GT_ITEMS];
    unsigned kind = 0;          // 2 bits per item: 0 not selected, 1 equal to T, 2 above T
    unsigned packed = 0;
#pragma unroll
    for (int j = 0; j < GT_ITEMS; ++j) {
        const int64_t p = p0 + j;
        key[j] = 0u;
        if (p < n && ids[p] >= 0) {
            const unsigned k = score_key(scores[p]);
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
    unsigned above = blk[blockIdx.x] + (ex >> 16);          // entries above T before this one, in input order
    unsigned equal = blk[nb + blockIdx.x] + (ex & 0xFFFFu);  // entries equal to T before this one
#pragma unroll
    for (int j = 0; j < GT_ITEMS; ++j) {
        const unsigned kd = (kind >> (2 * j)) & 3u;
        if (kd == 2u) {
            const unsigned o = above + (equal < fit ? equal : fit);
            keys[o] = ~key[j];
            pay[o] = (unsigned)(p0 + j);
            ++above;
        } else if (kd == 1u) {
            if (equal < fit) {
                const unsigned o = above + equal;
                keys[o] = ~key[j];
                pay[o] = (unsigned)(p0 + j);
            }
            ++equal;
        }
    }
}

// ---- (C) stable LSD radix sort of the survivors, ascending ~key = descending score -----------------------------------------------
__global__ __launch_bounds__(GT_THREADS) void gt_sort_hist_kernel(const unsigned *keys, const GtState *st, int shift, int64_t tile,
                                                                  unsigned *hist, int64_t nbs) {
    __shared__ unsigned h[256];
    const int tid = threadIdx.x;
    h[tid] = 0u;
    __syncthreads();
    const int64_t m = st->count;
    const int64_t lo = (int64_t)blockIdx.x * tile;
    const int64_t hi = lo + tile < m ? lo + tile : m;
    for (int64_t i = lo + tid; i < hi; i += GT_THREADS) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);
    __syncthreads();
    hist[(int64_t)tid * nbs + blockIdx.x] = h[tid];
}

// hist: after the scan, the first output slot of (digit, tile).  Inside a tile an element's slot is that base + the elements of
// its digit in earlier rounds of 256 (running) + those in lower waves of its round (wcount) + those in lower lanes of its wave.
__global__ __launch_bounds__(GT_THREADS) void gt_sort_scatter_kernel(const unsigned *keys_in, const unsigned *pay_in,
                                                                     unsigned *keys_out, unsigned *pay_out, const GtState *st,
                                                                     int shift, int64_t tile, const unsigned *hist, int64_t nbs) {
    constexpr int WAVES = GT_THREADS / 64;
    __shared__ unsigned running[256];
    __shared__ unsigned wcount[WAVES][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    running[tid] = hist[(int64_t)tid * nbs + blockIdx.x];
#pragma unroll
    for (int w = 0; w < WAVES; ++w) wcount[w][tid] = 0u;
    __syncthreads();
    const int64_t m = st->count;
    const int64_t lo = (int64_t)blockIdx.x * tile;
    const int64_t hi = lo + tile < m ? lo + tile : m;
    for (int64_t r = lo; r < hi; r += GT_THREADS) {
        const int64_t i = r + tid;
        const bool active = i < hi;
        const unsigned k = active ? keys_in[i] : 0u;
        const unsigned v = active ? pay_in[i] : 0u;
        const unsigned d = (k >> shift) & 255u;
        unsigned long long peers = __ballot(active);      // lanes of this wave that hold the same digit
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool set = (d >> bit) & 1u;
            const unsigned long long bal = __ballot(set);
            peers &= set ? bal : ~bal;
        }
        const unsigned below = (unsigned)__popcll(peers & ((1ull << lane) - 1ull));
        if (active && below == 0u) wcount[wave][d] = (unsigned)__popcll(peers);
        __syncthreads();
        if (active) {
            unsigned o = running[d] + below;
            for (int w = 0; w < wave; ++w) o += wcount[w][d];
            keys_out[o] = k;
            pay_out[o] = v;
        }
        __syncthreads();
        unsigned add = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            add += wcount[w][tid];
            wcount[w][tid] = 0u;
        }
        running[tid] += add;
        __syncthreads();
    }
}

// ---- (D) ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GT_THREADS) void gt_gather_kernel(const float *scores, const int64_t *rows, const int64_t *ids,
                                                               int32_t row_stride, const unsigned *pay, const GtState *st,
                                                               int64_t *out_rows, int64_t *out_ids, float *out_scores) {
    const int64_t m = st->count;
    for (int64_t i = (int64_t)blockIdx.x * GT_THREADS + threadIdx.x; i < m; i += (int64_t)gridDim.x * GT_THREADS) {
        const int64_t p = pay[i];
        out_rows[i] = rows ? rows[p] : p / row_stride;
        out_ids[i] = ids[p];
        out_scores[i] = scores[p];
    }
}

// ---- vsc_pair_first_hits --------------------------------------------------------------------------------------------------------
constexpr unsigned long long PFH_EMPTY = ~0ull;

__device__ inline uint64_t pfh_mix(uint64_t x) {   // splitmix64's finaliser
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// the pair key of entry p, or PFH_EMPTY for an entry that is no hit (a negative row or id: the search's padding)
__device__ inline unsigned long long pfh_key(const int64_t *rows, const int64_t *ids, int64_t p, const int32_t *qv, const int32_t *rv,
                                             int32_t nrv) {
    const int64_t row = rows[p], id = ids[p];
    if (row < 0 || id < 0) return PFH_EMPTY;
    return (unsigned long long)qv[row] * (unsigned long long)nrv + (unsigned long long)rv[id];
}

// the table holds at most n keys in >= 2 n slots: a probe sequence always ends at the key or at an empty slot
__global__ __launch_bounds__(GT_THREADS) void pfh_insert_kernel(const int64_t *rows, const int64_t *ids, int64_t n, const int32_t *qv,
                                                                const int32_t *rv, int32_t nrv, unsigned long long *tkeys,
                                                                unsigned *tpos, uint64_t mask) {
    for (int64_t p = (int64_t)blockIdx.x * GT_THREADS + threadIdx.x; p < n; p += (int64_t)gridDim.x * GT_THREADS) {
        const unsigned long long key = pfh_key(rows, ids, p, qv, rv, nrv);
        if (key == PFH_EMPTY) continue;
        uint64_t h = pfh_mix(key) & mask;
        for (uint64_t step = 0; step <= mask; ++step) {
            const unsigned long long prev = atomicCAS(&tkeys[h], PFH_EMPTY, key);
            if (prev == PFH_EMPTY || prev == key) {
                atomicMin(&tpos[h], (unsigned)p);
                break;
            }
            h = (h + 1) & mask;
        }
    }
}

__global__ __launch_bounds__(GT_THREADS) void pfh_flag_count_kernel(const int64_t *rows, const int64_t *ids, int64_t n, const int32_t *qv,
                                                                    const int32_t *rv, int32_t nrv, const unsigned long long *tkeys,
                                                                    const unsigned *tpos, uint64_t mask, uint8_t *flags, unsigned *blk) {
    __shared__ unsigned wsum[GT_THREADS / 64];
    const int64_t p0 = (int64_t)blockIdx.x * GT_TILE + (int64_t)threadIdx.x * GT_ITEMS;
    unsigned mine = 0;
    for (int j = 0; j < GT_ITEMS; ++j) {
        const int64_t p = p0 + j;
        if (p >= n) break;
        const unsigned long long key = pfh_key(rows, ids, p, qv, rv, nrv);
        unsigned first = 0;
        if (key != PFH_EMPTY) {
            uint64_t h = pfh_mix(key) & mask;
            for (uint64_t step = 0; step <= mask; ++step) {
                const unsigned long long at = tkeys[h];
                if (at == key) {
                    first = tpos[h] == (unsigned)p ? 1u : 0u;
                    break;
                }
                if (at == PFH_EMPTY) break;     // (cannot happen after the insert pass: every key is in the table)
                h = (h + 1) & mask;
            }
        }
        flags[p] = (uint8_t)first;
        mine += first;
    }
    unsigned tot;
    block_scan_excl<GT_THREADS>(mine, wsum, &tot);
    if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}

// blk: exclusive scan of the tiles' counts, blk[nb] their sum
__global__ __launch_bounds__(GT_THREADS) void pfh_scatter_kernel(const uint8_t *flags, int64_t n, const unsigned *blk, int64_t nb,
                                                                 int64_t limit, int64_t *out_pos, int64_t *out_count) {
    __shared__ unsigned wsum[GT_THREADS / 64];
    const int64_t p0 = (int64_t)blockIdx.x * GT_TILE + (int64_t)threadIdx.x * GT_ITEMS;
    unsigned bits = 0, mine = 0;
#pragma unroll
    for (int j = 0; j < GT_ITEMS; ++j)
        if (p0 + j < n && flags[p0 + j]) {
            bits |= 1u << j;
            ++mine;
        }
    unsigned tot;
    int64_t o = (int64_t)blk[blockIdx.x] + block_scan_excl<GT_THREADS>(mine, wsum, &tot);
#pragma unroll
    for (int j = 0; j < GT_ITEMS; ++j)
        if ((bits >> j) & 1u) {
            if (o < limit) out_pos[o] = p0 + j;
            ++o;
        }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t total = blk[nb];
        *out_count = total < limit ? total : limit;
    }
}

inline int grid_for(int64_t items, int per_block, int cap) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

template <class T>
int gt_scratch(int slot, size_t bytes, T **out) {
    void *p = nullptr;
    VSC_TRY(search_scratch_get(slot, bytes, &p));
    *out = (T *)p;
    return VSC_OK;
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
    int64_t tile = GT_TILE;
    if ((mb + tile - 1) / tile > GT_MAX_SORT_TILES)
        tile = ((mb + GT_MAX_SORT_TILES - 1) / GT_MAX_SORT_TILES + GT_THREADS - 1) / GT_THREADS * GT_THREADS;
    const int64_t nbs = (mb + tile - 1) / tile;
    GtState *st;
    unsigned *blk, *keys, *pay, *hist;
    VSC_TRY(gt_scratch(SCRATCH_GTK_STATE, sizeof(GtState), &st));
    VSC_TRY(gt_scratch(SCRATCH_GTK_BLOCKS, (size_t)nb * 2 * 4, &blk));
    VSC_TRY(gt_scratch(SCRATCH_GTK_KEYS, (size_t)mb * 2 * 4, &keys));
    VSC_TRY(gt_scratch(SCRATCH_GTK_PAY, (size_t)mb * 2 * 4, &pay));
    VSC_TRY(gt_scratch(SCRATCH_GTK_HIST, (size_t)nbs * 256 * 4, &hist));
    VSC_CHECK_HIP(hipMemsetAsync(st, 0, sizeof(GtState), stream));
    const int sweep_grid = grid_for(n, GT_THREADS, 1024);
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(gt_select_hist_kernel, dim3(sweep_grid), dim3(GT_THREADS), 0, stream, scores_dev, ids_dev, n, pass, st);
        VSC_CHECK_LAUNCH();
        hipLaunchKernelGGL(gt_select_pick_kernel, dim3(1), dim3(64), 0, stream, st, pass, (unsigned)mb, out_count_dev);
        VSC_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(gt_compact_count_kernel, dim3((unsigned)nb), dim3(GT_THREADS), 0, stream, scores_dev, ids_dev, n,
                       (const GtState *)st, blk, nb);
    VSC_CHECK_LAUNCH();
    hipLaunchKernelGGL(gt_scan_kernel, dim3(2), dim3(GT_SCAN_THREADS), 0, stream, blk, nb, (unsigned *)nullptr);
    VSC_CHECK_LAUNCH();
    hipLaunchKernelGGL(gt_compact_scatter_kernel, dim3((unsigned)nb), dim3(GT_THREADS), 0, stream, scores_dev, ids_dev, n,
                       (const GtState *)st, (const unsigned *)blk, nb, keys, pay);
    VSC_CHECK_LAUNCH();
    unsigned *k_in = keys, *k_out = keys + mb, *p_in = pay, *p_out = pay + mb;
    for (int shift = 0; shift < 32; shift += 8) {
        hipLaunchKernelGGL(gt_sort_hist_kernel, dim3((unsigned)nbs), dim3(GT_THREADS), 0, stream, (const unsigned *)k_in,
                           (const GtState *)st, shift, tile, hist, nbs);
        VSC_CHECK_LAUNCH();
        hipLaunchKernelGGL(gt_scan_kernel, dim3(1), dim3(GT_SCAN_THREADS), 0, stream, hist, nbs * 256, (unsigned *)nullptr);
        VSC_CHECK_LAUNCH();
        hipLaunchKernelGGL(gt_sort_scatter_kernel, dim3((unsigned)nbs), dim3(GT_THREADS), 0, stream, (const unsigned *)k_in,
                           (const unsigned *)p_in, k_out, p_out, (const GtState *)st, shift, tile, (const unsigned *)hist, nbs);
        VSC_CHECK_LAUNCH();
        unsigned *t = k_in; k_in = k_out; k_out = t;
        t = p_in; p_in = p_out; p_out = t;
    }
    hipLaunchKernelGGL(gt_gather_kernel, dim3(grid_for(mb, GT_THREADS, 2048)), dim3(GT_THREADS), 0, stream, scores_dev, rows_dev,
                       ids_dev, row_stride, (const unsigned *)p_in, (const GtState *)st, out_rows_dev, out_ids_dev, out_scores_dev);
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
    VSC_TRY(gt_scratch(SCRATCH_PFH_KEYS, (size_t)slots * 8, &tkeys));
    VSC_TRY(gt_scratch(SCRATCH_PFH_POS, (size_t)slots * 4, &tpos));
    VSC_TRY(gt_scratch(SCRATCH_PFH_FLAGS, (size_t)n, &flags));
    VSC_TRY(gt_scratch(SCRATCH_PFH_BLOCKS, (size_t)(nb + 1) * 4, &blk));
    VSC_CHECK_HIP(hipMemsetAsync(tkeys, 0xFF, (size_t)slots * 8, stream));
    VSC_CHECK_HIP(hipMemsetAsync(tpos, 0xFF, (size_t)slots * 4, stream));
    hipLaunchKernelGGL(pfh_insert_kernel, dim3(grid_for(n, GT_THREADS, 2048)), dim3(GT_THREADS), 0, stream, rows_dev, ids_dev, n,
                       q_video_dev, r_video_dev, n_r_videos, tkeys, tpos, slots - 1);
    VSC_CHECK_LAUNCH();
    hipLaunchKernelGGL(pfh_flag_count_kernel, dim3((unsigned)nb), dim3(GT_THREADS), 0, stream, rows_dev, ids_dev, n, q_video_dev,
                       r_video_dev, n_r_videos, (const unsigned long long *)tkeys, (const unsigned *)tpos, slots - 1, flags, blk);
    VSC_CHECK_LAUNCH();
    hipLaunchKernelGGL(gt_scan_kernel, dim3(1), dim3(GT_SCAN_THREADS), 0, stream, blk, nb, blk + nb);
    VSC_CHECK_LAUNCH();
    hipLaunchKernelGGL(pfh_scatter_kernel, dim3((unsigned)nb), dim3(GT_THREADS), 0, stream, (const uint8_t *)flags, n,
                       (const unsigned *)blk, nb, limit, out_pos_dev, out_count_dev);
    VSC_CHECK_LAUNCH();
    return VSC_OK;
}
