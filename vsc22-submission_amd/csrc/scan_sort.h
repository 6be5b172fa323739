// Prefix scans and the stable LSD radix sort of the device stages that order or compact (global_topk.hip, uap.hip), and the two
// host helpers every such stage repeats (grid_for, the typed search_scratch_get).  This header includes nothing: a .hip file
// includes it AFTER "common.h".  A quoted include of common.h from here would search csrc/ first -- the including file's own
// directory comes before the -I path -- and so hand the host emulation (tests/hip_emu, which is first only on the -I path) the
// device's common.h.  Kernels take one argument struct and no gridDim: the form the emulation launches.
//
// The sort, one 8-bit digit per pass: per-tile digit histograms, one exclusive scan over [digit][tile], stable in-tile ranking by
// wave ballots.  Integer atomics only count (LDS bins); every output position is a scan result.

namespace {

constexpr int SORT_THREADS = 256;
constexpr int SORT_TILE = 2048;
#ifndef VSC_SORT_MAX_TILES
#define VSC_SORT_MAX_TILES 4096                   // the sort's tile grows beyond this many tiles: the [256][tiles] scan stays <= 1M counters
#endif
static_assert(VSC_GLOBAL_TOPK_TILE == SORT_THREADS * 8 && VSC_UAP_TILE == SORT_THREADS * 8, "the public tiles are 256 threads x 8 items");
static_assert(SORT_TILE % SORT_THREADS == 0, "a tile is whole rounds of the workgroup");

__device__ inline unsigned wave_scan_incl(unsigned v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// exclusive prefix of v over the workgroup's threads, *total = the sum; wsum: NT / 64 words of LDS (reusable across calls: the
// leading barrier orders a call behind the reads of the one before)
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

// exclusive scan in place of `grid` runs of `len` counters each, one workgroup of NT threads per run; totals (or null): [grid]
struct ScanRunsArgs {
    unsigned *data;
    int64_t len;
    unsigned *totals;
};

template <int NT>
__global__ __launch_bounds__(NT) void scan_runs_kernel(ScanRunsArgs a) {
    __shared__ unsigned wsum[NT / 64];
    unsigned *d = a.data + (int64_t)blockIdx.x * a.len;
    unsigned carry = 0;
    for (int64_t base = 0; base < a.len; base += NT) {
        const int64_t i = base + threadIdx.x;
        const unsigned v = i < a.len ? d[i] : 0u;
        unsigned tot;
        const unsigned ex = block_scan_excl<NT>(v, wsum, &tot);
        if (i < a.len) d[i] = carry + ex;
        carry += tot;
    }
    if (a.totals && threadIdx.x == 0) a.totals[blockIdx.x] = carry;
}

template <int NT>
int scan_runs(unsigned *data, int64_t len, int grid, unsigned *totals, hipStream_t stream) {
    ScanRunsArgs a = {data, len, totals};
    hipLaunchKernelGGL(scan_runs_kernel<NT>, dim3(grid), dim3(NT), 0, stream, a);
    VSC_CHECK_LAUNCH();
    return VSC_OK;
}

// ---- stable LSD radix sort, one 8-bit digit per pass; K: an unsigned key type, P: the payload type ------------------------------
template <class K, class P>
struct SortArgs {
    const K *keys_in;
    const P *pay_in;           // null: the payload of entry i is i (the first pass of a sort that carries positions)
    K *keys_out;
    P *pay_out;                // null: keys only
    const unsigned *m_dev;     // the number of entries, on the device; null: m_host.  The grid is sized for the host's bound
    int64_t m_host, tile, nbs;
    unsigned *hist;            // [256][nbs]
    int shift;
};

template <class K, class P>
__device__ inline int64_t sort_len(const SortArgs<K, P> &a) { return a.m_dev ? (int64_t)*a.m_dev : a.m_host; }

template <class K, class P>
__global__ __launch_bounds__(SORT_THREADS) void sort_hist_kernel(SortArgs<K, P> a) {
    __shared__ unsigned h[256];
    const int tid = threadIdx.x;
    h[tid] = 0u;
    __syncthreads();
    const int64_t m = sort_len(a);
    const int64_t lo = (int64_t)blockIdx.x * a.tile;
    const int64_t hi = lo + a.tile < m ? lo + a.tile : m;
    for (int64_t i = lo + tid; i < hi; i += SORT_THREADS) atomicAdd(&h[(unsigned)(a.keys_in[i] >> a.shift) & 255u], 1u);
    __syncthreads();
    a.hist[(int64_t)tid * a.nbs + blockIdx.x] = h[tid];
}

// hist: after the scan, the first output slot of (digit, tile).  Inside a tile an element's slot is that base + the elements of
// its digit in earlier rounds of 256 (running) + those in lower waves of its round (wcount) + those in lower lanes of its wave.
template <class K, class P>
__global__ __launch_bounds__(SORT_THREADS) void sort_scatter_kernel(SortArgs<K, P> a) {
    constexpr int WAVES = SORT_THREADS / 64;
    __shared__ unsigned running[256];
    __shared__ unsigned wcount[WAVES][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    running[tid] = a.hist[(int64_t)tid * a.nbs + blockIdx.x];
#pragma unroll
    for (int w = 0; w < WAVES; ++w) wcount[w][tid] = 0u;
    __syncthreads();
    const int64_t m = sort_len(a);
    const int64_t lo = (int64_t)blockIdx.x * a.tile;
    const int64_t hi = lo + a.tile < m ? lo + a.tile : m;
    for (int64_t r = lo; r < hi; r += SORT_THREADS) {
        const int64_t i = r + tid;
        const bool active = i < hi;
        const K k = active ? a.keys_in[i] : (K)0;
        const P v = active ? (a.pay_in ? a.pay_in[i] : (P)i) : (P)0;
        const unsigned d = (unsigned)(k >> a.shift) & 255u;
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
            a.keys_out[o] = k;
            if (a.pay_out) a.pay_out[o] = v;
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

// the tile of a sort of (at most) m entries, and how many of them that makes
inline int64_t sort_tile(int64_t m) {
    int64_t tile = SORT_TILE;
    if ((m + tile - 1) / tile > VSC_SORT_MAX_TILES)
        tile = ((m + VSC_SORT_MAX_TILES - 1) / VSC_SORT_MAX_TILES + SORT_THREADS - 1) / SORT_THREADS * SORT_THREADS;
    return tile;
}
inline int64_t sort_tiles(int64_t m) { return (m + sort_tile(m) - 1) / sort_tile(m); }

// Sorts by the low `bits` bits of the keys, passes shift = 0, 8, .. < bits, the scan with SCAN_NT threads.  The entries number
// *m_dev, at most m (m_dev null: exactly m); m sizes the grids.  src_keys / src_pay (null: entry i carries i) feed the first
// pass and are only read unless they are `keys` / `pay` themselves.  keys: two buffers of `stride` keys; pay (or null: keys only):
// two buffers of `stride` payloads; hist: sort_tiles(m) x 256 counters.  A pass writes the buffer it does not read; the last
// pass's output is returned in *keys_sorted / *pay_sorted (or null).
template <int SCAN_NT, class K, class P>
int radix_sort(const K *src_keys, const P *src_pay, const unsigned *m_dev, int64_t m, int bits, K *keys, P *pay, int64_t stride,
               unsigned *hist, hipStream_t stream, const K **keys_sorted, const P **pay_sorted) {
    const int64_t nbs = sort_tiles(m);
    SortArgs<K, P> a;
    a.keys_in = src_keys;
    a.pay_in = src_pay;
    a.m_dev = m_dev;
    a.m_host = m;
    a.tile = sort_tile(m);
    a.nbs = nbs;
    a.hist = hist;
    for (int shift = 0; shift < bits; shift += 8) {
        a.keys_out = a.keys_in == keys ? keys + stride : keys;
        a.pay_out = !pay ? nullptr : (a.pay_in == pay ? pay + stride : pay);
        a.shift = shift;
        hipLaunchKernelGGL((sort_hist_kernel<K, P>), dim3((unsigned)nbs), dim3(SORT_THREADS), 0, stream, a);
        VSC_CHECK_LAUNCH();
        VSC_TRY(scan_runs<SCAN_NT>(hist, nbs * 256, 1, nullptr, stream));
        hipLaunchKernelGGL((sort_scatter_kernel<K, P>), dim3((unsigned)nbs), dim3(SORT_THREADS), 0, stream, a);
        VSC_CHECK_LAUNCH();
        a.keys_in = a.keys_out;
        a.pay_in = a.pay_out;
    }
    *keys_sorted = a.keys_in;
    if (pay_sorted) *pay_sorted = a.pay_in;
    return VSC_OK;
}

inline int grid_for(int64_t items, int per_block, int cap) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace

// the search's grow-only scratch (common.h), typed
template <class T>
int search_scratch_get(int slot, size_t bytes, T **out) {
    void *p = nullptr;
    VSC_TRY(search_scratch_get(slot, bytes, &p));
    *out = (T *)p;
    return VSC_OK;
}
