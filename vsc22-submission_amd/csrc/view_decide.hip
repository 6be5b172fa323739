// View decisions of the query preprocessing (the reference's image_process: remove_edges, split_imgs and the recursive clean_imgs,
// as src/image_preprocess.py restates them in _borders, _trim, _static_side, _bands, _line_cuts, _split and _clean) on the two maps
// of vsc_frame_var_u8 / vsc_canny_count_u8, which stay on the device.  The contract is stated with vsc_view_decide_f64 in
// include/vsc_hip.h (executable form: tests/view_decide_contract.py): the host path's arithmetic, bit for bit, which is numpy's.
//
// One kernel, one workgroup of 512 threads per video, one argument structure and a 1-D grid (which is also what lets the file run
// on the CPU against tests/hip_emu/common.h).  clean_imgs' recursion is an explicit stack of regions in LDS.  Per region:
//  (1) counts: an (m + 1)-bin histogram of the region (integer LDS atomics; zeros, the bulk, are counted in registers) gives the two
//      order statistics of np.quantile; the sum of avg = count / m in numpy's order for a 2-D region: the row-major flattening in
//      chunks of 8192, each summed pairwise by 8 lanes (one per strided accumulator of numpy's pairwise sum), the chunk sums chained.
//  (2) rows: 8 lanes per row walk numpy's pairwise tree over the row's variances and count the row's edge pixels.
//  (3) columns: one thread per column, rows ascending -- the add chain of a reduction over axis 0 -- and the column's edge pixels.
//  (4) the profile logic (_trim, _bands, _line_cuts) on the four profiles in LDS.  Every thread follows the same scalar control
//      flow; a _static_side call spreads its median over the workgroup (rank by counting) while two threads sum its two means.
// A region the borders left as it was keeps its profiles, histogram and sum for _split.  Edge sums are integers (the edge map is
// 0/1), so they are counted and divided once in float32.  No float atomics: the outputs are a pure function of the inputs.
// The bound is one CU's load latency: a plain 720p video reads its variance map twice and its count map six times through 512
// threads, so every map loop issues eight independent loads per thread before it consumes them in the stated order.
#include "common.h"

// contract arithmetic: add chains and trees in a stated order, correctly rounded divisions; nothing may be contracted or reassociated
#pragma clang fp contract(off)

namespace {

constexpr int VD_BLOCK = 512;
constexpr int VD_CHUNK = VSC_VIEW_DECIDE_CHUNK;          // items per launch: 64 x 32 bytes of kernel arguments (limit 4 KiB)
constexpr int VD_STACK = VSC_VIEW_DECIDE_STACK;          // pending regions
constexpr int VD_MAX_VIEWS = VSC_VIEW_DECIDE_MAX_VIEWS;
constexpr int VD_MAX_SIDE = VSC_VIEW_DECIDE_MAX_SIDE;
constexpr int VD_MAX_SAMPLES = VSC_VIEW_DECIDE_MAX_SAMPLES;
constexpr int VD_PIECES = 64;                            // pieces of one split: each is more than 80 lines of at most 4096
constexpr int VD_SUM_CHUNK = 8192;                       // numpy's reduction buffer, in elements
constexpr int VD_BATCH = 8;                              // independent loads a thread issues before it consumes them
constexpr int VD_MIN_FRAMES = 5, VD_MIN_SIDE = 20, VD_MIN_VIEW = 80, VD_GAP = 5;
static_assert(VD_CHUNK * 32 + 64 <= 4096 && 32 * VD_MAX_SIDE + 8192 <= 160 * 1024 && VD_MAX_SAMPLES <= 255 && VD_MAX_VIEWS <= VD_BLOCK / 4 &&
              VD_MAX_SIDE / (VD_MIN_VIEW + 1) < VD_PIECES && VD_BLOCK >= 128 && VD_MAX_SIDE * VD_MAX_SIDE / VD_SUM_CHUNK + 1 <= VD_MAX_SIDE,
              "include/vsc_hip.h states limits the kernel cannot hold");

struct VdItem {
    long long voff, coff;                     // element offsets of the two maps
    int h, w, m, n;
};

struct VdArgs {
    const double *var;
    const uint16_t *count;
    int32_t *boxes, *counts, *status;         // of this chunk
    double *trace;                            // of this chunk, or null
    int max_views;
    VdItem it[VD_CHUNK];
};

struct VdScalars {
    double q, mean, thr, sel[2], vmean;
    float emean;
    int cmin, np, start;
    uint32_t etotal;
};

// One leaf of numpy's pairwise sum: up to 128 elements in eight strided accumulators, combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)),
// then the remainder in order.  GROUP: lane k of 8 aligned lanes holds accumulator k and the combination is an xor butterfly, which
// forms the same three levels (the two operands of an addition may swap, the grouping may not); every lane returns the sum.
template <class T, bool GROUP, class F>
__device__ inline T vd_leaf(F &load, int off, int n, int k) {
    if (n < 8) {
        T res = (T)0;
        for (int i = 0; i < n; ++i) res += load(off + i);
        return res;
    }
    const int full = n - (n & 7);
    T res;
    if (GROUP) {
        // the lane's elements off + k, off + 8 + k, ...: eight loads in flight, then their adds in order (the loop is latency bound)
        T r = load(off + k);
        int i = 8;
        for (; i + 8 * VD_BATCH <= full; i += 8 * VD_BATCH) {
            T v[VD_BATCH];
#pragma unroll
            for (int u = 0; u < VD_BATCH; ++u) v[u] = load(off + i + 8 * u + k);
#pragma unroll
            for (int u = 0; u < VD_BATCH; ++u) r += v[u];
        }
        for (; i < full; i += 8) r += load(off + i + k);
        r += __shfl_xor(r, 1, 64);
        r += __shfl_xor(r, 2, 64);
        r += __shfl_xor(r, 4, 64);
        res = r;
    } else {
        T r0 = load(off), r1 = load(off + 1), r2 = load(off + 2), r3 = load(off + 3), r4 = load(off + 4), r5 = load(off + 5),
          r6 = load(off + 6), r7 = load(off + 7);
        for (int i = 8; i < full; i += 8) {
            r0 += load(off + i), r1 += load(off + i + 1), r2 += load(off + i + 2), r3 += load(off + i + 3);
            r4 += load(off + i + 4), r5 += load(off + i + 5), r6 += load(off + i + 6), r7 += load(off + i + 7);
        }
        res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    }
    for (int i = full; i < n; ++i) res += load(off + i);
    return res;
}

// numpy's pairwise sum of load(0) .. load(n - 1), n <= 8192: above 128 elements split at n / 2 rounded down to a multiple of 8.
// The recursion is a stack of seven frames at most.  GROUP: called by whole waves whose groups all have the same n.
template <class T, bool GROUP, class F>
__device__ inline T vd_pairwise(F load, int n, int k) {
    int f_off[8], f_n[8], f_stage[8];
    T f_left[8];
    int sp = 1;
    f_off[0] = 0, f_n[0] = n, f_stage[0] = 0;
    T ret = (T)0;
    while (sp > 0) {
        const int t = sp - 1;
        int n2 = f_n[t] / 2;
        n2 -= n2 % 8;
        if (f_stage[t] == 0) {
            if (f_n[t] <= 128) {
                ret = vd_leaf<T, GROUP>(load, f_off[t], f_n[t], k);
                --sp;
            } else {
                f_stage[t] = 1;
                f_off[sp] = f_off[t], f_n[sp] = n2, f_stage[sp] = 0;
                ++sp;
            }
        } else if (f_stage[t] == 1) {
            f_left[t] = ret;
            f_stage[t] = 2;
            f_off[sp] = f_off[t] + n2, f_n[sp] = f_n[t] - n2, f_stage[sp] = 0;
            ++sp;
        } else {
            ret = f_left[t] + ret;
            --sp;
        }
    }
    return ret;
}

struct VdRegion {
    int y0, y1, x0, x1;
};

struct VdMaps {
    const double *var;        // the item's [H][W] maps
    const uint16_t *count;
    int W, m;
    __device__ inline int cnt(int y, int x) const {
        const int c = count[(size_t)y * W + x];
        return c < m ? c : m;          // counts above m are outside the contract; they must not index past the tables
    }
};

// (1) histogram of the region's counts into hist[0..m] and the chunk sums of avg into work[]; thread 0 then leaves q and mean in s
__device__ void vd_count_pass(const VdMaps &mp, const VdRegion &g, uint32_t *hist, const double *avg, double *work, VdScalars *s) {
    const int tid = threadIdx.x, k = tid & 7, grp = tid >> 3;
    const int h = g.y1 - g.y0, w = g.x1 - g.x0, N = h * w;
    if (tid <= VD_MAX_SAMPLES) hist[tid] = 0u;
    __syncthreads();
    uint32_t zeros = 0u;
    for (int f0 = tid; f0 < N; f0 += VD_BLOCK * VD_BATCH) {
        int v[VD_BATCH];
#pragma unroll
        for (int u = 0; u < VD_BATCH; ++u) {
            const int f = f0 + u * VD_BLOCK;
            v[u] = f < N ? mp.cnt(g.y0 + f / w, g.x0 + f % w) : -1;
        }
#pragma unroll
        for (int u = 0; u < VD_BATCH; ++u) {
            if (v[u] == 0) ++zeros;
            else if (v[u] > 0) atomicAdd(&hist[v[u]], 1u);
        }
    }
    if (zeros) atomicAdd(&hist[0], zeros);
    const int whole = N / VD_SUM_CHUNK, tail = N % VD_SUM_CHUNK;
    for (int c0 = 0; c0 < whole; c0 += VD_BLOCK / 8) {
        const int ch = c0 + grp < whole ? c0 + grp : whole - 1;      // a group past the end repeats the last chunk: whole waves shuffle
        const int base = ch * VD_SUM_CHUNK;
        const double sum = vd_pairwise<double, true>([&](int i) { const int f = base + i; return avg[mp.cnt(g.y0 + f / w, g.x0 + f % w)]; },
                                                     VD_SUM_CHUNK, k);
        if (c0 + grp < whole && k == 0) work[ch] = sum;
    }
    if (tail) {       // every group sums the short last chunk, so that every wave runs the same shuffles
        const int base = whole * VD_SUM_CHUNK;
        const double sum = vd_pairwise<double, true>([&](int i) { const int f = base + i; return avg[mp.cnt(g.y0 + f / w, g.x0 + f % w)]; }, tail, k);
        if (tid == 0) work[whole] = sum;
    }
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (int ch = 0; ch < whole + (tail ? 1 : 0); ++ch) total += work[ch];
        s->mean = total / (double)N;
        const double pos = (double)(N - 1) * 0.95;
        const long long lo = (long long)floor(pos), hi = lo + 1 < N ? lo + 1 : N - 1;
        const double t = pos - (double)lo;
        double a = 0.0, b = 0.0;
        long long seen = 0;
        bool have_a = false;
        for (int c = 0; c <= mp.m; ++c) {
            seen += hist[c];
            if (!have_a && seen > lo) a = avg[c], have_a = true;
            if (seen > hi) {
                b = avg[c];
                break;
            }
        }
        const double d = b - a;
        s->q = t < 0.5 ? a + d * t : b - d * (1.0 - t);
    }
    __syncthreads();
}

// min(max(q, 0.2), mean + extra) as Python evaluates it, the least count above it, and the number of edge pixels of the region
__device__ void vd_threshold(const uint32_t *hist, const double *avg, int m, double extra, VdScalars *s) {
    if (threadIdx.x == 0) {
        const double floor_ = 0.2 > s->q ? 0.2 : s->q, cap = s->mean + extra;
        const double thr = cap < floor_ ? cap : floor_;
        int cmin = m + 1;
        for (int c = m; c >= 0 && avg[c] > thr; --c) cmin = c;
        uint32_t total = 0u;
        for (int c = cmin; c <= m; ++c) total += hist[c];
        s->thr = thr, s->cmin = cmin, s->etotal = total;
    }
    __syncthreads();
}

// (2) a.mean(1) of the region's variances into vrow[] (if want_var) and edges.mean(1) into erow[] (if cmin >= 0)
__device__ void vd_row_pass(const VdMaps &mp, const VdRegion &g, bool want_var, int cmin, double *vrow, float *erow) {
    const int tid = threadIdx.x, k = tid & 7, grp = tid >> 3;
    const int h = g.y1 - g.y0, w = g.x1 - g.x0;
    for (int r0 = 0; r0 < h; r0 += VD_BLOCK / 8) {
        const bool valid = r0 + grp < h;
        const int r = valid ? r0 + grp : h - 1;
        if (want_var) {
            const double *row = mp.var + (size_t)(g.y0 + r) * mp.W + g.x0;
            const double sum = vd_pairwise<double, true>([&](int i) { return row[i]; }, w, k);
            if (valid && k == 0) vrow[r] = sum / (double)w;
        }
        if (cmin >= 0) {
            int cnt = 0, c = k;
            for (; c + 8 * (VD_BATCH - 1) < w; c += 8 * VD_BATCH) {
                int v[VD_BATCH];
#pragma unroll
                for (int u = 0; u < VD_BATCH; ++u) v[u] = mp.cnt(g.y0 + r, g.x0 + c + 8 * u);
#pragma unroll
                for (int u = 0; u < VD_BATCH; ++u) cnt += v[u] >= cmin ? 1 : 0;
            }
            for (; c < w; c += 8) cnt += mp.cnt(g.y0 + r, g.x0 + c) >= cmin ? 1 : 0;
            cnt += __shfl_xor(cnt, 1, 64);
            cnt += __shfl_xor(cnt, 2, 64);
            cnt += __shfl_xor(cnt, 4, 64);
            if (valid && k == 0) erow[r] = (float)cnt / (float)w;
        }
    }
}

// (3) a.mean(0): one add chain per column from 0.0 -- except that numpy drops the axis of a region ONE column wide, whose reduction
// is then the inner loop: a pairwise sum down the column
__device__ void vd_col_pass(const VdMaps &mp, const VdRegion &g, bool want_var, int cmin, double *vcol, float *ecol) {
    const int h = g.y1 - g.y0, w = g.x1 - g.x0;
    for (int c = threadIdx.x; c < w; c += VD_BLOCK) {
        const double *col = mp.var + (size_t)g.y0 * mp.W + g.x0 + c;
        if (want_var) {
            double acc = 0.0;
            if (w == 1) {
                acc = vd_pairwise<double, false>([&](int i) { return col[(size_t)i * mp.W]; }, h, 0);
            } else {
                int r = 0;
                for (; r + VD_BATCH <= h; r += VD_BATCH) {      // eight rows in flight, added in row order
                    double v[VD_BATCH];
#pragma unroll
                    for (int u = 0; u < VD_BATCH; ++u) v[u] = col[(size_t)(r + u) * mp.W];
#pragma unroll
                    for (int u = 0; u < VD_BATCH; ++u) acc += v[u];
                }
                for (; r < h; ++r) acc += col[(size_t)r * mp.W];
            }
            vcol[c] = acc / (double)h;
        }
        if (cmin >= 0) {
            int cnt = 0, r = 0;
            for (; r + VD_BATCH <= h; r += VD_BATCH) {
                int v[VD_BATCH];
#pragma unroll
                for (int u = 0; u < VD_BATCH; ++u) v[u] = mp.cnt(g.y0 + r + u, g.x0 + c);
#pragma unroll
                for (int u = 0; u < VD_BATCH; ++u) cnt += v[u] >= cmin ? 1 : 0;
            }
            for (; r < h; ++r) cnt += mp.cnt(g.y0 + r, g.x0 + c) >= cmin ? 1 : 0;
            ecol[c] = (float)cnt / (float)h;
        }
    }
}

// _static_side over lines [lo, hi) of one axis' profiles.  Thread 0 sums the variances, thread 64 the edge levels (float32), and all
// threads rank the variances: the element with `less + equal before it` == k is the k-th order statistic.
__device__ bool vd_static_side(const double *vp, const float *ep, int lo, int hi, float edge_at, VdScalars *s) {
    const int L = hi - lo, tid = threadIdx.x;
    if (L <= 0) return false;            // numpy: the mean of an empty slice is NaN, which compares false
    if (tid == 0) s->vmean = vd_pairwise<double, false>([&](int i) { return vp[lo + i]; }, L, 0) / (double)L;
    if (tid == 64) s->emean = vd_pairwise<float, false>([&](int i) { return ep[lo + i]; }, L, 0) / (float)L;
    const int k1 = (L - 1) / 2, k2 = L / 2;
    for (int j = lo + tid; j < hi; j += VD_BLOCK) {
        const double v = vp[j];
        int rank = 0;
        for (int t = lo; t < hi; ++t) {
            const double x = vp[t];
            rank += (x < v || (x == v && t < j)) ? 1 : 0;
        }
        if (rank == k1) s->sel[0] = v;
        if (rank == k2) s->sel[1] = v;
    }
    __syncthreads();
    const double med = (L & 1) ? s->sel[0] : (s->sel[0] + s->sel[1]) / 2.0;
    const double level = med + s->vmean;
    const bool calm = s->emean < 0.0225f;
    const bool res = (level < 75.0 && calm) || (level < 250.0 && calm && edge_at > 0.65f);
    __syncthreads();
    return res;
}

// _trim along one axis -> the kept [first, end)
__device__ void vd_trim(const double *vp, const float *ep, int size, VdScalars *s, int *first_out, int *end_out) {
    if (threadIdx.x == 64) s->emean = vd_pairwise<float, false>([&](int i) { return ep[i]; }, size, 0) / (float)size;
    __syncthreads();
    const float bar = 0.125f + s->emean;
    __syncthreads();
    int first = 0, end = size;
    for (int i = 1; i < size - 1; ++i) {
        if (!(ep[i] > bar) || i - first < 5) continue;
        const int extra = (int)rint((double)(i - first) * 0.3);
        if (vd_static_side(vp, ep, first, i - extra, ep[i], s)) first = i + 1;
    }
    for (int i = size - 2; i >= 1; --i) {
        if (!(ep[i] > bar) || end - i < 5) continue;
        const int extra = (int)rint((double)(end - i) * 0.3);
        if (vd_static_side(vp, ep, i + extra, end, ep[i], s)) end = i;
    }
    *first_out = first, *end_out = end;
}

// profile[i : i + 5].mean() for every i of split_imgs' scan (all threads): a chain of five, then one division
__device__ void vd_band_levels(const double *p, int size, double *levels) {
    for (int i = threadIdx.x; i < size - VD_GAP; i += VD_BLOCK) levels[i] = ((((p[i] + p[i + 1]) + p[i + 2]) + p[i + 3]) + p[i + 4]) / 5.0;
    __syncthreads();
}

// split_imgs' scan of one axis over those levels (one thread): pieces[np..] = (a, b); returns where the scan's last piece started
__device__ int vd_bands(const double *levels, int size, int start, int (*pieces)[2], int *np) {
    bool inside = false;
    for (int i = 0; i < size - VD_GAP; ++i) {
        const double level = levels[i];
        if (!inside && (level > 0.1 || i - start > 50)) {
            inside = true;
        } else if (inside && level < 0.1) {
            if (i + VD_GAP / 2 - start > VD_MIN_VIEW && *np < VD_PIECES) pieces[*np][0] = start, pieces[*np][1] = i + VD_GAP / 2, ++*np;
            inside = false;
            start = i + VD_GAP / 2;
        }
    }
    return start;
}

// split_imgs' cut_h / cut_w (one thread): pieces between the lines above `level`, from the far end back
__device__ void vd_line_cuts(const float *ep, int size, float level, int (*pieces)[2], int *np) {
    int end = size;
    for (int i = size - 1; i >= 0; --i)
        if (ep[i] > level && end - i > VD_MIN_VIEW && *np < VD_PIECES) pieces[*np][0] = i, pieces[*np][1] = end, ++*np, end = i;
    if (*np && end > VD_MIN_VIEW && *np < VD_PIECES) pieces[*np][0] = 0, pieces[*np][1] = end, ++*np;
}

__global__ __launch_bounds__(VD_BLOCK) void view_decide_kernel(VdArgs a) {
    extern __shared__ __align__(16) unsigned char vd_smem[];
    __shared__ uint32_t s_hist[256];
    __shared__ double s_avg[256];
    __shared__ int s_stack[VD_STACK][4], s_views[VD_MAX_VIEWS][4], s_pieces[VD_PIECES][4], s_line[VD_PIECES][2];
    __shared__ VdScalars s_sc;

    const VdItem it = a.it[blockIdx.x];
    const int tid = threadIdx.x, H = it.h, W = it.w, S = H > W ? H : W;
    int32_t *boxes = a.boxes + (size_t)blockIdx.x * a.max_views * 4;
    if (it.n < VD_MIN_FRAMES) {           // clean_imgs: unchanged, and the maps are not read
        if (tid < a.max_views * 4) boxes[tid] = tid >= 4 ? -1 : tid == 1 ? H : tid == 3 ? W : 0;
        if (tid == 0) a.counts[blockIdx.x] = 1, a.status[blockIdx.x] = 0;
        return;
    }
    double *vrow = (double *)vd_smem, *vcol = vrow + S, *work = vcol + S;      // [S] each
    float *erow = (float *)(work + S), *ecol = erow + S;                       // [S] each
    VdScalars *s = &s_sc;
    VdMaps mp;
    mp.var = a.var + it.voff, mp.count = a.count + it.coff, mp.W = W, mp.m = it.m;

    if (tid <= it.m) s_avg[tid] = (double)tid / (double)it.m;
    if (tid == 0) s_stack[0][0] = 0, s_stack[0][1] = H, s_stack[0][2] = 0, s_stack[0][3] = W;
    __syncthreads();
    int sp = 1, nviews = 0;
    bool fail = false, top = true;
    while (sp > 0 && !fail) {
        --sp;
        const VdRegion box{s_stack[sp][0], s_stack[sp][1], s_stack[sp][2], s_stack[sp][3]};
        const int h = box.y1 - box.y0, w = box.x1 - box.x0;
        // _borders
        vd_count_pass(mp, box, s_hist, s_avg, work, s);
        vd_threshold(s_hist, s_avg, it.m, 0.35, s);
        vd_row_pass(mp, box, true, s->cmin, vrow, erow);
        vd_col_pass(mp, box, true, s->cmin, vcol, ecol);
        __syncthreads();
        if (top && a.trace && tid == 0) {
            double *tr = a.trace + (size_t)blockIdx.x * 8;
            tr[0] = s->q, tr[1] = s->mean, tr[2] = s->thr, tr[3] = (double)((float)s->etotal / (float)(h * w));
            tr[4] = vrow[h / 2], tr[5] = vcol[w / 2], tr[6] = (double)erow[h / 2], tr[7] = (double)ecol[w / 2];
        }
        top = false;
        int b0, b1, a0, a1;
        vd_trim(vrow, erow, h, s, &b0, &b1);
        vd_trim(vcol, ecol, w, s, &a0, &a1);
        const VdRegion cut{box.y0 + b0, box.y0 + b1, box.x0 + a0, box.x0 + a1};
        const int ch = b1 - b0, cw = a1 - a0;
        VdRegion leaf = box;
        int np = -1;                           // -1: the region stays whole
        if ((ch < cw ? ch : cw) >= VD_MIN_SIDE) {
            leaf = cut;
            // _split.  A region the borders left alone keeps its profiles, histogram, q and mean.
            const bool same = ch == h && cw == w;
            if (!same) vd_row_pass(mp, cut, true, -1, vrow, erow);
            __syncthreads();
            vd_band_levels(vrow, ch, work);
            if (tid == 0) {
                int n = 0;
                int start = vd_bands(work, ch, 0, s_line, &n);
                if ((n || start != 0) && ch - start > VD_MIN_VIEW && n < VD_PIECES) s_line[n][0] = start, s_line[n][1] = ch, ++n;
                for (int p = 0; p < n; ++p) s_pieces[p][0] = s_line[p][0], s_pieces[p][1] = s_line[p][1], s_pieces[p][2] = 0, s_pieces[p][3] = cw;
                s->np = n, s->start = start;
            }
            __syncthreads();
            np = s->np;
            if (np == 0) {
                if (!same) vd_col_pass(mp, cut, true, -1, vcol, ecol);
                __syncthreads();
                vd_band_levels(vcol, cw, work);
                if (tid == 0) {
                    int n = 0;
                    int start = vd_bands(work, cw, s->start, s_line, &n);
                    if ((n || start != 0) && cw - start > VD_MIN_VIEW && n < VD_PIECES) s_line[n][0] = start, s_line[n][1] = cw, ++n;
                    for (int p = 0; p < n; ++p) s_pieces[p][0] = 0, s_pieces[p][1] = ch, s_pieces[p][2] = s_line[p][0], s_pieces[p][3] = s_line[p][1];
                    s->np = n;
                }
                __syncthreads();
                np = s->np;
            }
            if (np == 0) {
                if (!same) vd_count_pass(mp, cut, s_hist, s_avg, work, s);
                vd_threshold(s_hist, s_avg, it.m, 0.3, s);
                vd_row_pass(mp, cut, false, s->cmin, vrow, erow);
                vd_col_pass(mp, cut, false, s->cmin, vcol, ecol);
                __syncthreads();
                if (tid == 0) {
                    const float level = 0.45f + (float)s->etotal / (float)(ch * cw);
                    int n = 0;
                    for (int pass = 0; pass < 2 && n == 0; ++pass) {
                        const bool by_cols = (cw > ch) == (pass == 0);
                        if (by_cols) vd_line_cuts(ecol, cw, level, s_line, &n);
                        else vd_line_cuts(erow, ch, level, s_line, &n);
                        for (int p = 0; p < n; ++p) {
                            s_pieces[p][0] = by_cols ? 0 : s_line[p][0], s_pieces[p][1] = by_cols ? ch : s_line[p][1];
                            s_pieces[p][2] = by_cols ? s_line[p][0] : 0, s_pieces[p][3] = by_cols ? s_line[p][1] : cw;
                        }
                    }
                    s->np = n ? n : -1;
                }
                __syncthreads();
                np = s->np;
            }
            if (np == 1 && s_pieces[0][1] - s_pieces[0][0] == ch && s_pieces[0][3] - s_pieces[0][2] == cw) np = -1;
        }
        if (np < 0) {
            if (nviews == a.max_views) {
                fail = true;
            } else {
                if (tid == 0) s_views[nviews][0] = leaf.y0, s_views[nviews][1] = leaf.y1, s_views[nviews][2] = leaf.x0, s_views[nviews][3] = leaf.x1;
                ++nviews;
            }
        } else if (sp + np > VD_STACK) {
            fail = true;
        } else {
            if (tid < np) {      // the first piece is cleaned first: it goes on top
                const int p = np - 1 - tid;
                s_stack[sp + tid][0] = cut.y0 + s_pieces[p][0], s_stack[sp + tid][1] = cut.y0 + s_pieces[p][1];
                s_stack[sp + tid][2] = cut.x0 + s_pieces[p][2], s_stack[sp + tid][3] = cut.x0 + s_pieces[p][3];
            }
            sp += np;
        }
        __syncthreads();
    }
    if (fail) nviews = 0;
    if (tid < a.max_views * 4) boxes[tid] = (tid >> 2) < nviews ? s_views[tid >> 2][tid & 3] : -1;
    if (tid == 0) a.counts[blockIdx.x] = nviews, a.status[blockIdx.x] = fail ? 1 : 0;
}

}  // namespace

int launch_view_decide(const double *var_dev, int64_t var_len, const uint16_t *count_dev, int64_t count_len, const int64_t *items_host,
                       int64_t n_items, int max_views, int32_t *boxes_dev, int32_t *counts_dev, int32_t *status_dev, double *trace_dev,
                       hipStream_t stream) {
    VSC_REQUIRE(n_items >= 0 && n_items < (1ll << 24) && var_len >= 0 && count_len >= 0, "view_decide: %lld items, %lld variances, %lld counts",
                (long long)n_items, (long long)var_len, (long long)count_len);
    VSC_REQUIRE(max_views >= 1 && max_views <= VD_MAX_VIEWS, "view_decide: max_views %d (1 to %d)", max_views, VD_MAX_VIEWS);
    if (n_items == 0) return VSC_OK;
    VSC_REQUIRE(items_host && var_dev && count_dev && boxes_dev && counts_dev && status_dev, "view_decide: null pointer");
    for (int64_t i = 0; i < n_items; ++i) {
        const int64_t *it = items_host + 6 * i;
        VSC_REQUIRE(it[2] >= 1 && it[2] <= VD_MAX_SIDE && it[3] >= 1 && it[3] <= VD_MAX_SIDE, "view_decide: item %lld is %lld x %lld (1 to %d a side)",
                    (long long)i, (long long)it[2], (long long)it[3], VD_MAX_SIDE);
        VSC_REQUIRE(it[4] >= 1 && it[4] <= VD_MAX_SAMPLES, "view_decide: item %lld has %lld Canny samples (1 to %d)", (long long)i, (long long)it[4],
                    VD_MAX_SAMPLES);
        VSC_REQUIRE(it[5] >= 0 && it[5] < (1ll << 31), "view_decide: item %lld has %lld frames", (long long)i, (long long)it[5]);
        VSC_REQUIRE(it[0] >= 0 && it[0] <= var_len && it[2] * it[3] <= var_len - it[0], "view_decide: item %lld = (%lld, %lld x %lld) outside the %lld variances",
                    (long long)i, (long long)it[0], (long long)it[2], (long long)it[3], (long long)var_len);
        VSC_REQUIRE(it[1] >= 0 && it[1] <= count_len && it[2] * it[3] <= count_len - it[1], "view_decide: item %lld = (%lld, %lld x %lld) outside the %lld counts",
                    (long long)i, (long long)it[1], (long long)it[2], (long long)it[3], (long long)count_len);
    }
    VdArgs a;
    a.var = var_dev, a.count = count_dev, a.max_views = max_views;
    for (int64_t base = 0; base < n_items; base += VD_CHUNK) {
        const int n = (int)(n_items - base < VD_CHUNK ? n_items - base : VD_CHUNK);
        long long side = 1;
        for (int i = 0; i < VD_CHUNK; ++i) {
            if (i >= n) {
                a.it[i] = VdItem{0, 0, 1, 1, 1, 0};
                continue;
            }
            const int64_t *it = items_host + 6 * (base + i);
            a.it[i] = VdItem{(long long)it[0], (long long)it[1], (int)it[2], (int)it[3], (int)it[4], (int)it[5]};
            if (it[5] >= VD_MIN_FRAMES) side = it[2] > side ? it[2] : side, side = it[3] > side ? it[3] : side;
        }
        a.boxes = boxes_dev + (size_t)base * max_views * 4, a.counts = counts_dev + base, a.status = status_dev + base;
        a.trace = trace_dev ? trace_dev + (size_t)base * 8 : nullptr;
        const int lds = (int)(32 * side);
        VSC_TRY(vsc_allow_dynamic_lds(view_decide_kernel, lds));
        hipLaunchKernelGGL(view_decide_kernel, dim3((unsigned)n), dim3(VD_BLOCK), (size_t)lds, stream, a);
        VSC_CHECK_LAUNCH();
    }
    return VSC_OK;
}

struct vsc_view_decide {
    hipStream_t stream;
};

extern "C" int vsc_view_decide_create(void *stream, vsc_view_decide **out) {
    VSC_REQUIRE(out, "view_decide_create: null pointer");
    *out = new vsc_view_decide{(hipStream_t)stream};
    return VSC_OK;
}

extern "C" void vsc_view_decide_destroy(vsc_view_decide *h) { delete h; }

extern "C" int vsc_view_decide_f64(vsc_view_decide *h, const double *var_dev, int64_t var_len, const uint16_t *count_dev, int64_t count_len,
                                   const int64_t *items_host, int64_t n_items, int32_t max_views, int32_t *boxes_dev, int32_t *counts_dev,
                                   int32_t *status_dev, double *trace_dev) {
    VSC_REQUIRE(h, "view_decide: null handle");
    return launch_view_decide(var_dev, var_len, count_dev, count_len, items_host, n_items, max_views, boxes_dev, counts_dev, status_dev, trace_dev,
                              h->stream);
}
