// Matching-track localisation (VSC22-Matching-Track-1st/infer/src/utils.py:76-117): threshold, 8-connected components and one
// RANSAC line fit per component group of every (probability map, threshold) item, batched: one workgroup per item, the items of
// a launch independent.  The contract is stated with vsc_match_segments_f32 in include/vsc_hip.h (executable form:
// tests/seg_contract.py).
//
// Per item, in one workgroup of MS_BLOCK threads; pixel p = x * w + y belongs to thread p % MS_BLOCK, so a wave always holds
// 64 consecutive pixels and raster order is (chunk, lane) order:
//  (A) labels: a uint16 per pixel in LDS (224^2 * 2 B = 98 KiB), initialised to the pixel's own index; sweeps of "minimum over
//      the 8 neighbours, then two pointer jumps" until a whole sweep changes nothing.  Every thread writes only its own pixels and
//      labels only decrease, so stale reads cost a sweep at most; the fixed point is the component's first pixel in raster order.
//      view_prep.hip's union-find (Canny hysteresis) is not shared: it links int32 labels in global memory with atomicMin, and
//      neither 32-bit labels (196 KiB) nor a 16-bit atomicMin exist in LDS; the sweep needs no atomics at all.
//  (B) sizes: a root's own cell is redundant once a bitmap marks the roots, so it becomes the component's counter: the other
//      pixels add 1 to it (one wave-aggregated 32-bit LDS add per distinct label of a wave; 50 176 < 2^16: no carry into the
//      neighbouring cell).  Roots of more than 10 pixels are ranked in raster order by ballots and prefix sums; then every cell
//      holds the rank of its large component, LOOSE or BG.
//  (C) per group (large component g + all loose pixels): per-chunk member counts + exclusive scan (point index -> pixel by a
//      binary search and a ballot), the distinct query frames, then the sequential trial loop: thread 0 draws the 2-subset from
//      an MT19937 in LDS (numpy's RandomState(2023) stream: permutation's head below 200 points, tracking selection from there),
//      and each trial is one pass of the whole workgroup over the map: integer inlier test, k / sum y / sum y^2 / A by wave and
//      workgroup reductions, R^2 and the dynamic stop in float64 scalars.
//  (D) the final weighted least squares, the near-point statistics and the score: float64 reductions in a fixed order (two
//      runs give the same bytes).
#include <vector>

#include "common.h"

// R^2, the dx = 0 constant and the score are contract arithmetic: every product and sum is rounded on its own
#pragma clang fp contract(off)

namespace {

constexpr int MS_BLOCK = 512;
constexpr int MS_WAVES = MS_BLOCK / 64;
constexpr int MS_MAX_SIDE = 224;
constexpr int MS_MAX_THR = 8;
constexpr int MS_MIN_COMPONENT = 10;
constexpr int MS_MAX_TRIALS = 200;
constexpr int MS_PERM_BELOW = 200;            // 2 / n > 0.01: sample_without_replacement takes a permutation's head
constexpr unsigned MS_BG = 0xFFFFu, MS_LOOSE = 0xFFFEu, MS_NO_GROUP = 0xFFFDu;
constexpr int MT_N = 624, MT_M = 397;

struct MtState { uint32_t v[MT_N]; };
constexpr MtState mt_seeded(uint32_t seed) {   // init_genrand: numpy's RandomState(seed) for an integer seed
    MtState s{};
    for (int i = 0; i < MT_N; ++i) {
        s.v[i] = seed;
        seed = 1812433253u * (seed ^ (seed >> 30)) + (uint32_t)i + 1u;
    }
    return s;
}
__constant__ MtState ms_seed_2023 = mt_seeded(2023u);

struct MsItem {
    long long off;
    int h, w;
};

struct MsArgs {
    const float *maps;
    const MsItem *items;
    float thr[MS_MAX_THR];
    double ratio[MS_MAX_THR];
    int n_thr, max_seg;
    int32_t *seg;
    double *score;
    int32_t *counts;
};

// one word of the generator, in place (equivalent to regenerating all 624 words at once)
__device__ inline uint32_t mt_next(uint32_t *mt, int &pos) {
    const int i = pos, i1 = i + 1 == MT_N ? 0 : i + 1, im = i + MT_M >= MT_N ? i + MT_M - MT_N : i + MT_M;
    const uint32_t y = (mt[i] & 0x80000000u) | (mt[i1] & 0x7fffffffu);
    uint32_t v = mt[im] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    mt[i] = v;
    pos = i1;
    v ^= v >> 11;
    v ^= (v << 7) & 0x9d2c5680u;
    v ^= (v << 15) & 0xefc60000u;
    v ^= v >> 18;
    return v;
}

// uniform integer in [0, max], max >= 1: numpy's masked rejection (random_interval / buffered_bounded_masked_uint32)
__device__ inline uint32_t mt_bounded(uint32_t *mt, int &pos, uint32_t max) {
    uint32_t mask = max;
    mask |= mask >> 1, mask |= mask >> 2, mask |= mask >> 4, mask |= mask >> 8, mask |= mask >> 16;
    uint32_t v;
    do v = mt_next(mt, pos) & mask;
    while (v > max);
    return v;
}

struct OpSumLL { __device__ long long operator()(long long a, long long b) const { return a + b; } };
struct OpMinLL { __device__ long long operator()(long long a, long long b) const { return a < b ? a : b; } };
struct OpMaxLL { __device__ long long operator()(long long a, long long b) const { return a > b ? a : b; } };
struct OpSumD { __device__ double operator()(double a, double b) const { return a + b; } };
struct OpMaxD { __device__ double operator()(double a, double b) const { return a > b ? a : b; } };

// workgroup reduction in a fixed order: xor-butterfly inside each wave, then waves 0 .. MS_WAVES-1 in sequence; every thread gets
// the result.  `red` holds MS_WAVES values of 8 bytes.
template <class T, class Op>
__device__ inline T block_reduce(T v, Op op, void *red_raw) {
    T *red = (T *)red_raw;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = red[0];
#pragma unroll
    for (int i = 1; i < MS_WAVES; ++i) r = op(r, red[i]);
    __syncthreads();
    return r;
}

// the same for N values under one operation: one exchange and one pair of barriers for all of them.  `red` holds MS_WAVES * N values.
template <int N, class T, class Op>
__device__ inline void block_reduce_n(T (&v)[N], Op op, void *red_raw) {
    T *red = (T *)red_raw;
#pragma unroll
    for (int j = 0; j < N; ++j) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[j] = op(v[j], __shfl_xor(v[j], o, 64));
        if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * N + j] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) {
        T r = red[j];
#pragma unroll
        for (int i = 1; i < MS_WAVES; ++i) r = op(r, red[i * N + j]);
        v[j] = r;
    }
    __syncthreads();
}

// pixel walk of one thread: p = tid, tid + MS_BLOCK, ... with (x, y) kept without a division per pixel
struct Walk {
    int p, x, y, sx, sy, w;
    __device__ Walk(int tid, int w_) : p(tid), x(tid / w_), y(tid % w_), sx(MS_BLOCK / w_), sy(MS_BLOCK % w_), w(w_) {}
    __device__ void step() {
        p += MS_BLOCK, x += sx, y += sy;
        if (y >= w) y -= w, ++x;
    }
};

struct Model {          // a trial's line: through (x1, y1) with direction (dx, dy), or y = c when dx == 0
    int x1, y1, dx, dy;
    double c;
    __device__ bool inlier(int x, int y) const {
        if (dx != 0) {
            const int r = (y - y1) * dx - dy * (x - x1);
            return (r < 0 ? -r : r) <= 2 * (dx < 0 ? -dx : dx);
        }
        return fabs((double)y - c) <= 2.0;
    }
};

__global__ __launch_bounds__(MS_BLOCK) void match_segments_kernel(MsArgs a) {
    extern __shared__ __align__(16) unsigned char ms_smem[];
    __shared__ uint32_t mt[MT_N];
    __shared__ int perm[MS_PERM_BELOW];
    __shared__ int rowflag[MS_MAX_SIDE], colflag[MS_MAX_SIDE];
    __shared__ long long red[MS_WAVES * 4];
    __shared__ int s_wave_cnt[MS_WAVES];
    __shared__ int s_idx[2], s_pt[2];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const int ti = blockIdx.x % a.n_thr;
    const MsItem it = a.items[blockIdx.x / a.n_thr];
    const int h = it.h, w = it.w, npx = h * w;
    int32_t *seg_out = a.seg + (size_t)blockIdx.x * a.max_seg * 4;
    double *score_out = a.score + (size_t)blockIdx.x * a.max_seg;
    if (npx == 0) {
        if (tid == 0) a.counts[blockIdx.x] = 0;
        return;
    }
    const int nchunk = (npx + 63) >> 6, npad = nchunk << 6;
    uint16_t *lab = (uint16_t *)ms_smem;                       // [npad]
    uint32_t *lab32 = (uint32_t *)ms_smem;
    uint32_t *isroot = (uint32_t *)(ms_smem + (size_t)npad * 2);   // [nchunk][2]: ballot of "is the first pixel of its component"
    uint32_t *prefix = isroot + 2 * nchunk;                    // [nchunk + 1]: members before each chunk
    const float *P = a.maps + it.off;
    const float thr = a.thr[ti];
    const double std_ratio = a.ratio[ti];

    // ---- (A) mask and labels -----------------------------------------------------------------------------------------
    for (int p = tid; p < npad; p += MS_BLOCK) lab[p] = p < npx && P[p] > thr ? (uint16_t)p : (uint16_t)MS_BG;
    __syncthreads();
    // The reads of other threads' cells below are unsynchronised on purpose: a cell is written by its owner only and only ever
    // decreases, so a stale value is a valid older label.  The barrier inside __syncthreads_or is what publishes a sweep's writes
    // to the next sweep; the loop ends only after a sweep in which nobody wrote, i.e. one that read a consistent state.
    for (;;) {
        int changed = 0;
        for (Walk k(tid, w); k.p < npx; k.step()) {
            const unsigned v = lab[k.p];
            if (v == MS_BG) continue;
            unsigned m = v;
            const bool left = k.y > 0, right = k.y + 1 < w;
            if (k.x > 0) {
                const uint16_t *up = lab + k.p - w;
                if (left) m = min(m, (unsigned)up[-1]);
                m = min(m, (unsigned)up[0]);
                if (right) m = min(m, (unsigned)up[1]);
            }
            if (left) m = min(m, (unsigned)lab[k.p - 1]);
            if (right) m = min(m, (unsigned)lab[k.p + 1]);
            if (k.x + 1 < h) {
                const uint16_t *dn = lab + k.p + w;
                if (left) m = min(m, (unsigned)dn[-1]);
                m = min(m, (unsigned)dn[0]);
                if (right) m = min(m, (unsigned)dn[1]);
            }
            m = min(m, (unsigned)lab[m]);         // a label is always a pixel of the same component (never BG)
            m = min(m, (unsigned)lab[m]);
            if (m < v) lab[k.p] = (uint16_t)m, changed = 1;
        }
        if (!__syncthreads_or(changed)) break;
    }

    // ---- (B) component sizes, large components ranked in raster order --------------------------------------------------
    for (int p = tid; p < npad; p += MS_BLOCK) {
        const bool root = lab[p] == p;            // BG and the padding never equal an index
        const unsigned long long bal = __ballot(root);
        if (lane == 0) isroot[2 * (p >> 6)] = (uint32_t)bal, isroot[2 * (p >> 6) + 1] = (uint32_t)(bal >> 32);
        if (root) lab[p] = 0;                     // from here on: pixels of the component beside the root
    }
    __syncthreads();
    for (int p = tid; p < npad; p += MS_BLOCK) {
        const unsigned v = lab[p];
        const bool root = (isroot[2 * (p >> 6) + (lane >> 5)] >> (lane & 31)) & 1u;
        const bool other = v != MS_BG && !root;
        unsigned long long rem = __ballot(other);
        while (rem) {
            const int leader = __ffsll((long long)rem) - 1;
            const unsigned l = __shfl(v, leader, 64);
            const unsigned long long same = __ballot(other && v == l);
            if (lane == leader) atomicAdd(lab32 + (l >> 1), (uint32_t)__popcll(same) << (16 * (l & 1u)));
            rem &= ~same;
        }
    }
    __syncthreads();
    int n_large = 0;
    for (int base = 0; base < npad; base += MS_BLOCK) {   // same trip count for every wave: the loop holds barriers
        const int p = base + tid;
        const bool root = p < npad && ((isroot[2 * (p >> 6) + (lane >> 5)] >> (lane & 31)) & 1u);
        const bool large = root && (int)lab[p] + 1 > MS_MIN_COMPONENT;
        const unsigned long long bal = __ballot(large);
        if (lane == 0) s_wave_cnt[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int i = 0; i < MS_WAVES; ++i) {
            const int c = s_wave_cnt[i];
            before += i < wave ? c : 0;
            total += c;
        }
        if (root) lab[p] = large ? (uint16_t)(n_large + before + __popcll(bal & lt_mask)) : (uint16_t)MS_LOOSE;
        n_large += total;
        __syncthreads();
    }
    for (int p = tid; p < npad; p += MS_BLOCK) {   // the other pixels take their root's value (roots are written above only)
        const unsigned v = lab[p];
        const bool root = (isroot[2 * (p >> 6) + (lane >> 5)] >> (lane & 31)) & 1u;
        if (v != MS_BG && !root) lab[p] = lab[v];
    }
    __syncthreads();

    // ---- (C) one RANSAC fit per group --------------------------------------------------------------------------------------
    int n_seg = 0;
    const int n_groups = n_large ? n_large : 1;
    for (int g = 0; g < n_groups; ++g) {
        const unsigned target = n_large ? (unsigned)g : MS_NO_GROUP;
        auto member = [&](unsigned v) { return v == MS_LOOSE || v == target; };
        if (tid < MS_MAX_SIDE) rowflag[tid] = 0;
        __syncthreads();
        {
            Walk k(tid, w);
            for (; k.p < npad; k.step()) {
                const bool mem = member(lab[k.p]);
                const unsigned long long bal = __ballot(mem);
                if (lane == 0) prefix[k.p >> 6] = __popcll(bal);
                if (mem) rowflag[k.x] = 1;
            }
        }
        __syncthreads();
        if (wave == 0) {                          // exclusive scan of the chunk counts: a run of chunks per lane
            const int per = (nchunk + 63) >> 6, lo = lane * per, hi = min(nchunk, lo + per);
            int sum = 0;
            for (int c = lo; c < hi; ++c) sum += prefix[c];
            int incl = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(incl, o, 64);
                if (lane >= o) incl += t;
            }
            int run = incl - sum;
            for (int c = lo; c < hi; ++c) {
                const int t = prefix[c];
                prefix[c] = run;
                run += t;
            }
            if (lane == 63) prefix[nchunk] = incl;
        }
        const long long n_rows = block_reduce<long long>(tid < h ? rowflag[tid] : 0, OpSumLL(), red);   // syncs: prefix[] is complete
        const int n = (int)prefix[nchunk];
        if (n_rows <= 3) continue;

        for (int i = tid; i < MT_N; i += MS_BLOCK) mt[i] = ms_seed_2023.v[i];
        int mt_pos = 0;                           // thread 0's
        int best_k = 1, trials = 0, max_trials = MS_MAX_TRIALS;
        double best_r2 = -INFINITY;
        bool have = false;
        Model best = {0, 0, 0, 0, 0.0};
        __syncthreads();
        while (trials < max_trials) {
            ++trials;
            if (n < MS_PERM_BELOW) {
                if (tid < n) perm[tid] = tid;
                __syncthreads();
            }
            if (tid == 0) {
                int i1, i2;
                if (n < MS_PERM_BELOW) {          // rs.permutation(n)[:2]: the whole shuffle decides the head
                    for (int i = n - 1; i >= 1; --i) {
                        const int j = (int)mt_bounded(mt, mt_pos, (uint32_t)i);
                        const int t = perm[i];
                        perm[i] = perm[j], perm[j] = t;
                    }
                    i1 = perm[0], i2 = perm[1];
                } else {                          // tracking selection: redraw while the index is taken
                    i1 = (int)mt_bounded(mt, mt_pos, (uint32_t)(n - 1));
                    do i2 = (int)mt_bounded(mt, mt_pos, (uint32_t)(n - 1));
                    while (i2 == i1);
                }
                s_idx[0] = i1, s_idx[1] = i2;
            }
            __syncthreads();
            if (wave < 2) {                       // point index -> pixel
                const int i = s_idx[wave];
                int lo = 0, hi = nchunk;
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if ((int)prefix[mid] <= i) lo = mid;
                    else hi = mid;
                }
                const int p = (lo << 6) + lane;
                const bool mem = member(lab[p]);
                const unsigned long long bal = __ballot(mem);
                if (mem && __popcll(bal & lt_mask) == i - (int)prefix[lo]) s_pt[wave] = p;
            }
            __syncthreads();
            const int p1 = s_pt[0], p2 = s_pt[1];
            Model m;
            m.x1 = p1 / w, m.y1 = p1 % w;
            const int x2 = p2 / w, y2 = p2 % w;
            m.dx = x2 - m.x1, m.dy = y2 - m.y1, m.c = (double)m.y1;
            if (m.dx == 0 && m.dy != 0) {
                const float q1 = P[p1], q2 = P[p2];
                const float f1 = q1 * q1, f2 = q2 * q2;          // np.square of an fp32 map stays fp32
                const double w1 = (double)f1, w2 = (double)f2;
                m.c = (w1 * (double)m.y1 + w2 * (double)y2) / (w1 + w2);
            }
            long long k = 0, sy = 0, syy = 0, aa = 0;
            for (Walk t(tid, w); t.p < npx; t.step()) {
                if (!member(lab[t.p])) continue;
                if (m.dx != 0) {
                    const int r = (t.y - m.y1) * m.dx - m.dy * (t.x - m.x1);
                    if ((r < 0 ? -r : r) > 2 * (m.dx < 0 ? -m.dx : m.dx)) continue;
                    aa += (long long)r * r;
                } else if (!(fabs((double)t.y - m.c) <= 2.0)) {
                    continue;
                }
                ++k, sy += t.y, syy += t.y * t.y;
            }
            long long sums[4] = {k, sy, syy, aa};
            block_reduce_n(sums, OpSumLL(), red);
            k = sums[0], sy = sums[1], syy = sums[2], aa = sums[3];
            if (k < best_k) continue;
            const long long b = k * syy - sy * sy;
            double r2;
            if (m.dx != 0) {
                if (b == 0) r2 = aa == 0 ? 1.0 : 0.0;
                else r2 = 1.0 - ((double)aa * (double)k) / ((double)((long long)m.dx * m.dx) * (double)b);
            } else {
                const double res = ((double)syy - (2.0 * m.c) * (double)sy) + ((double)k * m.c) * m.c;
                if (b == 0) r2 = res == 0.0 ? 1.0 : 0.0;
                else r2 = 1.0 - (res * (double)k) / (double)b;
            }
            if (k == best_k && r2 < best_r2) continue;
            best_k = (int)k, best_r2 = r2, best = m, have = true;
            const double ratio = (double)k / (double)n;
            const double denom = fmax(2.220446049250313e-16, 1.0 - ratio * ratio);
            if (denom != 1.0) {
                const double t = fabs(ceil(log(1.0 - 0.99) / log(denom)));
                if (t < (double)max_trials) max_trials = (int)t;
            }
        }
        if (!have) continue;

        // ---- (D) final model over the best inliers, near points, score ---------------------------------------------------
        double sw = 0.0, swx = 0.0, swy = 0.0;
        for (Walk t(tid, w); t.p < npx; t.step()) {
            if (!member(lab[t.p]) || !best.inlier(t.x, t.y)) continue;
            const float q = P[t.p];
            const float f = q * q;
            const double wi = (double)f;
            sw += wi, swx += wi * (double)t.x, swy += wi * (double)t.y;
        }
        double wsum[3] = {sw, swx, swy};
        block_reduce_n(wsum, OpSumD(), red);
        sw = wsum[0], swx = wsum[1], swy = wsum[2];
        const double xm = swx / sw, ym = swy / sw;
        double sxx = 0.0, sxy = 0.0;
        for (Walk t(tid, w); t.p < npx; t.step()) {
            if (!member(lab[t.p]) || !best.inlier(t.x, t.y)) continue;
            const float q = P[t.p];
            const float f = q * q;
            const double wx = (double)f * ((double)t.x - xm);
            sxx += wx * ((double)t.x - xm), sxy += wx * ((double)t.y - ym);
        }
        double csum[2] = {sxx, sxy};
        block_reduce_n(csum, OpSumD(), red);
        sxx = csum[0], sxy = csum[1];
        const double slope = sxx > 0.0 ? sxy / sxx : 0.0;
        const double icpt = ym - slope * xm;
        if (!(slope > 0.0)) continue;
        if (tid < MS_MAX_SIDE) rowflag[tid] = 0, colflag[tid] = 0;
        __syncthreads();
        long long cnt = 0, first = npx, last = -1;
        double top = -INFINITY, sum = 0.0;
        for (Walk t(tid, w); t.p < npx; t.step()) {
            if (!member(lab[t.p])) continue;
            if (!(fabs((double)t.y - (slope * (double)t.x + icpt)) < 1.0)) continue;
            const double q = (double)P[t.p];
            ++cnt, sum += q;
            top = q > top ? q : top;
            first = t.p < first ? t.p : first, last = t.p > last ? t.p : last;
            rowflag[t.x] = 1, colflag[t.y] = 1;
        }
        first = block_reduce(first, OpMinLL(), red);
        last = block_reduce(last, OpMaxLL(), red);
        top = block_reduce(top, OpMaxD(), red);
        sum = block_reduce(sum, OpSumD(), red);
        long long flags[3] = {cnt, tid < h ? rowflag[tid] : 0, tid < w ? colflag[tid] : 0};
        block_reduce_n(flags, OpSumLL(), red);
        cnt = flags[0];
        const long long near_x = flags[1], near_y = flags[2];
        if (!(cnt > 5 && near_x > 3 && near_y > 3)) continue;
        const double mean = sum / (double)cnt;
        double var = 0.0;
        for (Walk t(tid, w); t.p < npx; t.step()) {
            if (!member(lab[t.p])) continue;
            if (!(fabs((double)t.y - (slope * (double)t.x + icpt)) < 1.0)) continue;
            const double d = (double)P[t.p] - mean;
            var += d * d;
        }
        var = block_reduce(var, OpSumD(), red);
        const double sd = sqrt(var / (double)cnt);
        const double s = fmax(1.0 / slope, slope);
        if (tid == 0 && n_seg < a.max_seg) {
            int32_t *o = seg_out + 4 * n_seg;
            o[0] = (int)first / w, o[1] = (int)first % w, o[2] = (int)last / w, o[3] = (int)last % w;
            score_out[n_seg] = (top - sd * std_ratio) - fabs(s - 1.0) / 10.0;
        }
        ++n_seg;
    }
    if (tid == 0) a.counts[blockIdx.x] = n_seg;     // uncapped: the caller sees an overflow
}

}  // namespace

int launch_match_segments(const float *maps_dev, int64_t maps_len, const int64_t *items_host, int64_t n_items, const float *thresholds,
                          const double *std_ratios, int n_thr, int max_segments, int32_t *segments_dev, double *scores_dev,
                          int32_t *counts_dev, hipStream_t stream) {
    VSC_REQUIRE(n_items >= 0 && n_thr >= 1 && n_thr <= MS_MAX_THR && n_items * n_thr < (1ll << 31), "match_segments: %lld items x %d thresholds (1 .. %d)",
                (long long)n_items, n_thr, MS_MAX_THR);
    VSC_REQUIRE(max_segments >= 0, "match_segments: max_segments %d < 0", max_segments);
    if (n_items == 0) return VSC_OK;
    VSC_REQUIRE(items_host && thresholds && std_ratios && counts_dev && (max_segments == 0 || (segments_dev && scores_dev)),
                "match_segments: null pointer");
    static thread_local std::vector<MsItem> table;
    table.resize((size_t)n_items);
    int max_px = 0;
    for (int64_t i = 0; i < n_items; ++i) {
        const int64_t off = items_host[3 * i], h = items_host[3 * i + 1], w = items_host[3 * i + 2];
        VSC_REQUIRE(h >= 0 && h <= MS_MAX_SIDE && w >= 0 && w <= MS_MAX_SIDE, "match_segments: item %lld is %lld x %lld (limit %d x %d)",
                    (long long)i, (long long)h, (long long)w, MS_MAX_SIDE, MS_MAX_SIDE);
        VSC_REQUIRE(off >= 0 && off + h * w <= maps_len && (h * w == 0 || maps_dev), "match_segments: item %lld = (%lld, %lld, %lld) outside the %lld map values",
                    (long long)i, (long long)off, (long long)h, (long long)w, (long long)maps_len);
        table[i] = MsItem{off, (int)h, (int)w};
        max_px = h * w > max_px ? (int)(h * w) : max_px;
    }
    MsArgs a;
    for (int t = 0; t < n_thr; ++t) a.thr[t] = thresholds[t], a.ratio[t] = std_ratios[t];
    void *tt;
    VSC_TRY(search_scratch_get(SCRATCH_MS_TABLE, (size_t)n_items * sizeof(MsItem), &tt));
    VSC_CHECK_HIP(hipMemcpyAsync(tt, table.data(), table.size() * sizeof(MsItem), hipMemcpyHostToDevice, stream));
    VSC_CHECK_HIP(hipStreamSynchronize(stream));  // `table` is reused by the next call
    const int nchunk = (max_px + 63) / 64;
    const int lds = nchunk * 64 * 2 + nchunk * 8 + (nchunk + 1) * 4;   // labels, root bitmap, chunk prefix (<= 109 768 B)
    VSC_TRY(vsc_allow_dynamic_lds(match_segments_kernel, lds));
    a.maps = maps_dev, a.items = (const MsItem *)tt;
    a.n_thr = n_thr, a.max_seg = max_segments;
    a.seg = segments_dev, a.score = scores_dev, a.counts = counts_dev;
    hipLaunchKernelGGL(match_segments_kernel, dim3((unsigned)(n_items * n_thr)), dim3(MS_BLOCK), (size_t)lds, stream, a);
    VSC_CHECK_LAUNCH();
    return VSC_OK;
}

extern "C" int vsc_match_segments_f32(const float *maps_dev, int64_t maps_len, const int64_t *items_host, int64_t n_items,
                                      const float *thresholds, const double *std_ratios, int32_t n_thr, int32_t max_segments,
                                      int32_t *out_segments_dev, double *out_scores_dev, int32_t *out_counts_dev, void *stream) {
    return launch_match_segments(maps_dev, maps_len, items_host, n_items, thresholds, std_ratios, n_thr, max_segments, out_segments_dev,
                                 out_scores_dev, out_counts_dev, (hipStream_t)stream);
}
