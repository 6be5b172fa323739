// Matching-track segment AP on the device (VSC22-Matching-Track-1st/infer/vsc/metrics.py:120-383: Intervals, VideoPair.add_prediction
// and the accumulation loop of match_metric).  The contract is stated with vsc_segment_metric_deltas_f64 / _scan_f64 in
// include/vsc_hip.h (executable form: tests/segment_metric_contract.py).  The reference rebuilds and re-sorts every interval list
// of a video pair on every prediction; here the work is split where the metric allows it:
//  (a) sm_delta_kernel, one wave (one 64-thread workgroup) per video pair.  Per axis the wave keeps three MERGED SETS as sorted
//      arrays of disjoint components in the handle's scratch: U (the predictions so far), G (the considered ground truths) and W
//      (both together).  All three only ever grow, so a new interval is one sorted insert: the lanes count the components that end
//      before it and those that start at or before its end (ballots over chunks of 64), the components in between fuse with it, and
//      the list is copied into its second buffer with the tail shifted.  Components, their order and their bounds involve no
//      rounding.  The lengths do: len = ((0.0 + (e0 - s0)) + (e1 - s1)) + ... is summed left to right -- the lanes compute the
//      differences of a chunk into LDS and every lane carries the same dependent adds over it.  Ground truths become considered by
//      the fp64 product of the two overlaps, as written in the reference.  O((n_p + n_g)^2 / 64) loads and O(n_p (n_p + n_g))
//      dependent adds per pair; the pairs are independent workgroups.
//  (b) sm_scan_kernel, ONE workgroup: rows go through LDS in tiles of 512 with all 256 threads, lane c of wave 0 carries column c's
//      running sum strictly left to right and leaves every prefix in the tile, and all threads copy the prefixes at `ends` out.
// Both only enqueue on the handle's stream.  No 16-bit operands: one object for both builds of the library.
#include "common.h"

// contract arithmetic: every difference and every sum rounded on its own
#pragma clang fp contract(off)

namespace {

constexpr int SM_WAVE = 64;
constexpr int SM_SLOTS_PER_BOX = 8;           // per axis: U and G twice (two buffers), W twice over both
constexpr int SC_BLOCK = 256;
constexpr int SC_TILE = 512;                  // rows per LDS tile: 512 x 8 columns x 8 bytes = 32 KiB
constexpr int SC_MAX_COLS = 8;

struct SmIv {
    double s, e;
};

struct SmList {                                // a merged set: n disjoint components, ascending; `nxt` is the other buffer
    SmIv *cur, *nxt;
    int n;
};

struct SmDeltaArgs {
    const double *pred_boxes;                  // [P][4], rank order
    const long long *pred_ptr, *pred_rank;     // [n_pairs + 1], [P]
    const double *gt_boxes;                    // [G][4]
    const long long *gt_ptr;                   // [n_pairs + 1]
    SmIv *slots;                               // [8 (P + G)]
    int *flags;                                // [G]: considered
    double *deltas, *gt_len;                   // [P][4], [n_pairs][2]
    long long P, G;
};

struct SmScanArgs {
    const double *rows;
    const long long *ends;
    double *out;
    long long n, n_ends;
    int cols;
};

// L := merged set of L and [s, e].  Uniform over the wave; ends with the list visible to every lane.
__device__ inline void sm_insert(SmList &L, double s, double e, int lane) {
    int before = 0, upto = 0;                  // components with c.e < s; components with c.s <= e (a superset: both are prefixes)
    for (int base = 0; base < L.n; base += SM_WAVE) {
        const int i = base + lane;
        const bool in = i < L.n;
        SmIv c = {0.0, 0.0};
        if (in) c = L.cur[i];
        before += __popcll(__ballot(in && c.e < s));
        upto += __popcll(__ballot(in && c.s <= e));
    }
    if (upto < before) upto = before;          // (only for operands outside the contract: the list never grows by more than one)
    double ms = s, me = e;
    if (upto > before) {
        ms = fmin(s, L.cur[before].s);
        me = fmax(e, L.cur[upto - 1].e);
    }
    const int gone = upto - before, n2 = L.n - gone + 1;
    for (int base = 0; base < n2; base += SM_WAVE) {
        const int i = base + lane;
        if (i < n2) {
            SmIv c = {ms, me};
            if (i < before) c = L.cur[i];
            else if (i > before) c = L.cur[i + gone - 1];
            L.nxt[i] = c;
        }
    }
    SmIv *t = L.cur;
    L.cur = L.nxt, L.nxt = t, L.n = n2;
    __syncthreads();
}

// ((0.0 + (e0 - s0)) + (e1 - s1)) + ...: the same value in every lane
__device__ inline double sm_length(const SmList &L, double *diff, int lane) {
    double acc = 0.0;
    for (int base = 0; base < L.n; base += SM_WAVE) {
        const int i = base + lane, cnt = L.n - base < SM_WAVE ? L.n - base : SM_WAVE;
        if (i < L.n) {
            const SmIv c = L.cur[i];
            diff[lane] = c.e - c.s;
        }
        __syncthreads();
        for (int j = 0; j < cnt; ++j) acc = acc + diff[j];
        __syncthreads();
    }
    return acc;
}

__global__ __launch_bounds__(SM_WAVE) void sm_delta_kernel(SmDeltaArgs a) {
    __shared__ double diff[SM_WAVE];
    const int lane = threadIdx.x;
    const long long pair = blockIdx.x;
    const long long p0 = a.pred_ptr[pair], p1 = a.pred_ptr[pair + 1], g0 = a.gt_ptr[pair], g1 = a.gt_ptr[pair + 1];
    if (p0 < 0 || p1 < p0 || p1 > a.P || g0 < 0 || g1 < g0 || g1 > a.G) return;      // never outside the buffers, whatever the tables hold
    const long long npl = p1 - p0, ngl = g1 - g0;
    const int np = (int)npl, ng = (int)ngl;
    SmIv *slot = a.slots + SM_SLOTS_PER_BOX * (p0 + g0);
    SmList U[2], Gc[2], W[2];
    for (int ax = 0; ax < 2; ++ax) {
        U[ax] = SmList{slot, slot + npl, 0}, slot += 2 * npl;
        Gc[ax] = SmList{slot, slot + ngl, 0}, slot += 2 * ngl;
        W[ax] = SmList{slot, slot + npl + ngl, 0}, slot += 2 * (npl + ngl);
    }
    const double *gts = a.gt_boxes + 4 * g0;
    int *flag = a.flags + g0;

    // all the pair's ground truths, merged: gt_len
    for (int g = 0; g < ng; ++g) {
        const double *b = gts + 4ll * g;
        sm_insert(W[0], b[0], b[1], lane);
        sm_insert(W[1], b[2], b[3], lane);
    }
    const double l0 = sm_length(W[0], diff, lane), l1 = sm_length(W[1], diff, lane);
    if (lane < 2) a.gt_len[2 * pair + lane] = lane ? l1 : l0;
    W[0].n = W[1].n = 0;
    for (int g = lane; g < ng; g += SM_WAVE) flag[g] = 0;       // lane g % 64 owns flag g from here on

    double i_prev[2] = {0.0, 0.0}, t_prev[2] = {0.0, 0.0}, g_len[2] = {0.0, 0.0};
    for (int k = 0; k < np; ++k) {
        const long long rank = a.pred_rank[p0 + k];
        if (rank < 0 || rank >= a.P) continue;
        const double *pb = a.pred_boxes + 4 * rank;
        const double qs = pb[0], qe = pb[1], rs = pb[2], re = pb[3];
        bool grew = false;
        for (int base = 0; base < ng; base += SM_WAVE) {
            const int g = base + lane;
            bool hit = false;
            if (g < ng && !flag[g]) {
                const double *b = gts + 4ll * g;
                const double q = fmax(fmin(qe, b[1]) - fmax(qs, b[0]), 0.0), r = fmax(fmin(re, b[3]) - fmax(rs, b[2]), 0.0);
                hit = fabs(q * r) > 0.0;                        // the product as written: an underflow is "no overlap" in the reference too
                if (hit) flag[g] = 1;
            }
            unsigned long long mask = __ballot(hit);
            while (mask) {
                const double *b = gts + 4ll * (base + __ffsll((long long)mask) - 1);
                mask &= mask - 1;
                sm_insert(Gc[0], b[0], b[1], lane), sm_insert(W[0], b[0], b[1], lane);
                sm_insert(Gc[1], b[2], b[3], lane), sm_insert(W[1], b[2], b[3], lane);
                grew = true;
            }
        }
        sm_insert(U[0], qs, qe, lane), sm_insert(W[0], qs, qe, lane);
        sm_insert(U[1], rs, re, lane), sm_insert(W[1], rs, re, lane);
        double out[4];
        for (int ax = 0; ax < 2; ++ax) {
            const double t = sm_length(U[ax], diff, lane);
            if (grew) g_len[ax] = sm_length(Gc[ax], diff, lane);
            const double i = (t + g_len[ax]) - sm_length(W[ax], diff, lane);
            out[ax] = i - i_prev[ax], out[2 + ax] = t - t_prev[ax];
            i_prev[ax] = i, t_prev[ax] = t;
        }
        if (lane == 0) {
            double *d = a.deltas + 4 * rank;
            d[0] = out[0], d[1] = out[1], d[2] = out[2], d[3] = out[3];
        }
    }
}

__global__ __launch_bounds__(SC_BLOCK) void sm_scan_kernel(SmScanArgs a) {
    __shared__ double tile[SC_TILE * SC_MAX_COLS];
    __shared__ int s_taken;
    const int tid = threadIdx.x, cols = a.cols;
    double acc = 0.0;                                            // thread c < cols: column c's running sum
    long long e = 0;                                             // ends consumed so far (uniform)
    for (long long r0 = 0; r0 < a.n; r0 += SC_TILE) {
        const int rows = (int)(a.n - r0 < SC_TILE ? a.n - r0 : SC_TILE);
        for (int i = tid; i < rows * cols; i += SC_BLOCK) tile[i] = a.rows[r0 * cols + i];
        __syncthreads();
        if (tid < cols)
            for (int r = 0; r < rows; ++r) {
                acc = acc + tile[r * cols + tid];
                tile[r * cols + tid] = acc;
            }
        __syncthreads();
        for (;;) {                                               // the ends inside this tile: a run of `ends`, SC_BLOCK at a time
            const long long idx = e + tid;
            const long long v = idx < a.n_ends ? a.ends[idx] : -1;
            const bool inside = idx < a.n_ends && v < r0 + rows;
            if (inside && v >= r0)
                for (int c = 0; c < cols; ++c) a.out[idx * cols + c] = tile[(int)(v - r0) * cols + c];
            if (tid == 0) s_taken = 0;
            __syncthreads();
            if (inside && (tid == SC_BLOCK - 1 || !(idx + 1 < a.n_ends && a.ends[idx + 1] < r0 + rows))) s_taken = tid + 1;   // the last one inside
            __syncthreads();
            const int taken = s_taken;
            __syncthreads();
            e += taken;
            if (taken < SC_BLOCK) break;
        }
    }
}

}  // namespace

struct vsc_segment_metric {
    hipStream_t stream = nullptr;
    void *scratch = nullptr;                   // interval slots + considered flags of one deltas call: grow-only, freed with the handle
    size_t scratch_bytes = 0;
};

extern "C" int vsc_segment_metric_create(void *stream, vsc_segment_metric **out) {
    VSC_REQUIRE(out, "segment_metric_create: null pointer");
    vsc_segment_metric *m = new vsc_segment_metric;
    m->stream = (hipStream_t)stream;
    *out = m;
    return VSC_OK;
}

extern "C" void vsc_segment_metric_destroy(vsc_segment_metric *m) {
    if (!m) return;
    if (m->scratch) (void)hipFree(m->scratch);                 // (waits for the device: the handle's launches have finished with it)
    delete m;
}

extern "C" int vsc_segment_metric_deltas_f64(vsc_segment_metric *m, const double *pred_boxes_dev, const int64_t *pred_ptr_dev,
                                             const int64_t *pred_rank_dev, int64_t n_preds, const double *gt_boxes_dev,
                                             const int64_t *gt_ptr_dev, int64_t n_gts, int64_t n_pairs, double *deltas_dev,
                                             double *gt_len_dev) {
    VSC_REQUIRE(m, "segment_metric_deltas: null handle");
    VSC_REQUIRE(n_preds >= 0 && n_preds < (1ll << 31) && n_gts >= 0 && n_gts < (1ll << 31) && n_pairs >= 0 && n_pairs < (1ll << 31),
                "segment_metric_deltas: %lld predictions, %lld ground truths, %lld pairs (each in [0, 2^31))", (long long)n_preds,
                (long long)n_gts, (long long)n_pairs);
    if (n_preds == 0 || n_pairs == 0) return VSC_OK;
    VSC_REQUIRE(pred_boxes_dev && pred_ptr_dev && pred_rank_dev && gt_ptr_dev && deltas_dev && gt_len_dev && (gt_boxes_dev || n_gts == 0),
                "segment_metric_deltas: null pointer");
    const size_t slot_bytes = (size_t)SM_SLOTS_PER_BOX * (size_t)(n_preds + n_gts) * sizeof(SmIv);
    const size_t need = slot_bytes + (size_t)n_gts * sizeof(int);
    if (need > m->scratch_bytes) {
        if (m->scratch) VSC_CHECK_HIP(hipFree(m->scratch));    // (waits for the device: earlier calls have finished with it)
        m->scratch = nullptr, m->scratch_bytes = 0;
        VSC_CHECK_HIP(hipMalloc(&m->scratch, need));
        m->scratch_bytes = need;
    }
    SmDeltaArgs a;
    a.pred_boxes = pred_boxes_dev, a.pred_ptr = (const long long *)pred_ptr_dev, a.pred_rank = (const long long *)pred_rank_dev;
    a.gt_boxes = gt_boxes_dev, a.gt_ptr = (const long long *)gt_ptr_dev;
    a.slots = (SmIv *)m->scratch, a.flags = (int *)((char *)m->scratch + slot_bytes);
    a.deltas = deltas_dev, a.gt_len = gt_len_dev, a.P = n_preds, a.G = n_gts;
    hipLaunchKernelGGL(sm_delta_kernel, dim3((unsigned)n_pairs), dim3(SM_WAVE), 0, m->stream, a);
    VSC_CHECK_LAUNCH();
    return VSC_OK;
}

extern "C" int vsc_segment_metric_scan_f64(vsc_segment_metric *m, const double *rows_dev, int64_t n, int32_t cols, const int64_t *ends_dev,
                                           int64_t n_ends, double *out_dev) {
    VSC_REQUIRE(m, "segment_metric_scan: null handle");
    VSC_REQUIRE(n >= 0 && n_ends >= 0, "segment_metric_scan: %lld rows, %lld ends", (long long)n, (long long)n_ends);
    VSC_REQUIRE(cols >= 1 && cols <= SC_MAX_COLS, "segment_metric_scan: %d columns outside [1, %d]", cols, SC_MAX_COLS);
    if (n == 0 || n_ends == 0) return VSC_OK;
    VSC_REQUIRE(rows_dev && ends_dev && out_dev, "segment_metric_scan: null pointer");
    SmScanArgs a;
    a.rows = rows_dev, a.ends = (const long long *)ends_dev, a.out = out_dev, a.n = n, a.n_ends = n_ends, a.cols = cols;
    hipLaunchKernelGGL(sm_scan_kernel, dim3(1), dim3(SC_BLOCK), 0, m->stream, a);
    VSC_CHECK_LAUNCH();
    return VSC_OK;
}
