// DP and HV temporal alignment of candidate-pair similarity matrices (VCSL's `dp` with `njit_dp_matrix`, `find_path`, `cut_path`,
// infer/vcsl/vta.py:98-127,153-241, and `hv`, :366-426), batched beside TN (tn_align.hip): one wave per pair, the pairs of a launch
// independent, the pair list cut into as few launches as the handle's scratch cap allows.  The contracts are stated with
// vsc_align_dp_f32 / vsc_align_hv_f32 in include/vsc_hip.h (executable form: tests/align_contract.py).
//
// DP, per pair, in one workgroup of 64 lanes:
//  (A) the recurrence as a skewed wavefront over strips of 64 rows: at step t lane l owns column t - l of row i0 + l; `left` is
//      its own last value, `top` and `top-left` are lane l-1's last two values (one cross-lane move each); lane 0 reads the
//      strip above from the dp / acc matrices.  dp (4 B), bt (1 B) and a SATURATING 8-bit acc go to scratch: acc only feeds
//      `acc <= discontinue` and `acc + 1`, so 255 stands for every larger count as long as discontinue <= 254.
//  (B) per row the first maximum of dp (value, column), kept up to date for the rows a round masks: a round's arg-max is a
//      reduction over Q entries, not over the matrix.
//  (C) up to 100 rounds: arg-max (whole wave), back-trace (lane 0), the path's similarities gathered in path order and the
//      path's bounding block masked to -inf (whole wave), rows re-scanned, then lane 0 walks the runs of the path (cut_path),
//      sums every kept sub-path in numpy's pairwise order and emits the boxes.
//  (D) MaxSim of every stored box.
// HV, per pair, in one workgroup of 64 lanes:
//  (A) a lane per diagonal: numpy's pairwise float32 sum of the thresholded diagonal and whether it holds a peak cell;
//  (B) max_peaks selection rounds (descending score, ties to the lower sigma), the IoU test of a round spread over the lanes;
//  (D) MaxSim of every box.
#include <climits>
#include <vector>

#include "common.h"

#pragma clang fp contract(off)   // every sum below is the fp32 sum of the contract: no fused multiply-add

namespace {

constexpr int AL_MAX_DIM = 1 << 16;            // rows and columns of a pair
constexpr long long AL_MAX_CELLS = 1ll << 26;  // cells of a pair (indices inside a pair are 32-bit)
constexpr int AL_MAX_BOXES = 4096;
constexpr int AL_MAX_DISCONTINUE = 254;        // the 8-bit acc saturates at 255
constexpr int AL_ROUNDS = 100;                 // dp(): cnt = 100
constexpr int64_t AL_DEFAULT_CAP = 256ll << 20;

struct AlPair {
    long long off;   // element offset of the [q, r] matrix
    long long sb;    // byte offset of the pair's scratch in its launch's arena
    int q, r;
};

struct DpArgs {
    const float *sims;
    const AlPair *pairs;   // of the launch's first pair
    char *arena;
    float bias, min_sim32, ave_sim32;
    int discontinue, min_length, diagonal_thres, max_boxes;
    int *boxes, *counts;   // of the launch's first pair
    float *maxsim;
};

struct HvArgs {
    const float *sims;
    const AlPair *pairs;
    char *arena;
    float bias, min_sim32;
    double iou_thresh;
    int max_peaks;
    int *boxes, *counts;
    float *maxsim;
};

__device__ inline float al_shfl_xor_f(float v, int m) { return __shfl_xor(v, m, 64); }
__device__ inline int al_shfl_xor_i(int v, int m) { return __shfl_xor(v, m, 64); }

// One leaf of numpy's pairwise sum (n <= 128): fewer than 8 elements in order, else eight strided accumulators combined
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) and the remainder in order.
template <class F>
__device__ inline float al_leaf(F &load, int off, int n) {
    if (n < 8) {
        float res = 0.0f;
        for (int i = 0; i < n; ++i) res += load(off + i);
        return res;
    }
    const int full = n - (n & 7);
    float r0 = load(off), r1 = load(off + 1), r2 = load(off + 2), r3 = load(off + 3), r4 = load(off + 4), r5 = load(off + 5),
          r6 = load(off + 6), r7 = load(off + 7);
    for (int i = 8; i < full; i += 8) {
        r0 += load(off + i), r1 += load(off + i + 1), r2 += load(off + i + 2), r3 += load(off + i + 3);
        r4 += load(off + i + 4), r5 += load(off + i + 5), r6 += load(off + i + 6), r7 += load(off + i + 7);
    }
    float res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (int i = full; i < n; ++i) res += load(off + i);
    return res;
}

// numpy's pairwise float32 sum of load(0) .. load(n - 1), n < 2^18: above 128 elements split at n / 2 rounded down to a multiple
// of 8.  The recursion is a stack of at most 12 frames (every split at least halves the longer part: 2^18 -> 128 in 11 levels).
template <class F>
__device__ inline float al_pairwise(F load, int n) {
    constexpr int DEPTH = 14;
    int f_off[DEPTH], f_n[DEPTH], f_stage[DEPTH];
    float f_left[DEPTH];
    int sp = 1;
    f_off[0] = 0, f_n[0] = n, f_stage[0] = 0;
    float ret = 0.0f;
    while (sp > 0) {
        const int t = sp - 1;
        int n2 = f_n[t] / 2;
        n2 -= n2 % 8;
        if (f_stage[t] == 0) {
            if (f_n[t] <= 128 || sp >= DEPTH) {   // (the depth bound never binds below 2^18 elements)
                ret = al_leaf(load, f_off[t], f_n[t]);
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

// (D) MaxSim of the first n boxes: max of (s + bias) over the half-open box, minus bias; -inf over an empty extent
__device__ inline void al_maxsim(const float *M, int R, float bias, const int *boxes, float *maxsim, int n, int lane) {
    for (int j = 0; j < n; ++j) {
        const int x1 = boxes[4 * j], y1 = boxes[4 * j + 1], x2 = boxes[4 * j + 2], y2 = boxes[4 * j + 3];
        const long long w = y2 - y1, cells = (long long)(x2 - x1) * w;
        float m = -INFINITY;
        for (long long i = lane; i < cells; i += 64) {
            const float v = M[(size_t)(x1 + i / w) * R + y1 + i % w] + bias;
            m = v > m ? v : m;
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const float o = al_shfl_xor_f(m, s);
            m = o > m ? o : m;
        }
        if (lane == 0) maxsim[j] = m - bias;
    }
}

__device__ inline void al_clear(int *boxes, float *maxsim, int slots, int lane) {
    for (int i = lane; i < slots * 4; i += 64) boxes[i] = 0;
    for (int i = lane; i < slots; i += 64) maxsim[i] = 0.0f;
}

// first maximum of row i of dp (ties to the lower column) -> rowmax[i], rowarg[i]; whole wave
__device__ inline void dp_row_scan(const float *dp, int R, int i, float *rowmax, int *rowarg, int lane) {
    const float *row = dp + (size_t)i * R;
    float bv = -INFINITY;
    int bc = INT_MAX;
    for (int c = lane; c < R; c += 64) {
        const float v = row[c];
        if (v > bv || (v == bv && c < bc)) bv = v, bc = c;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ov = al_shfl_xor_f(bv, m);
        const int oc = al_shfl_xor_i(bc, m);
        if (ov > bv || (ov == bv && oc < bc)) bv = ov, bc = oc;
    }
    if (lane == 0) rowmax[i] = bv, rowarg[i] = bc;
}

__global__ __launch_bounds__(64) void dp_align_kernel(DpArgs a) {
    const int lane = threadIdx.x;
    const AlPair P = a.pairs[blockIdx.x];
    const int Q = P.q, R = P.r, slots = a.max_boxes;
    int *boxes = a.boxes + (size_t)blockIdx.x * slots * 4;
    float *maxsim = a.maxsim + (size_t)blockIdx.x * slots;
    al_clear(boxes, maxsim, slots, lane);
    if (Q == 0 || R == 0) {
        if (lane == 0) a.counts[blockIdx.x] = 0;
        return;
    }
    const float *M = a.sims + P.off;
    const float bias = a.bias;
    const int cells = Q * R;
    char *base = a.arena + P.sb;
    float *dp = (float *)base;
    float *rowmax = dp + cells;
    int *rowarg = (int *)(rowmax + Q);
    int *path = rowarg + Q;                       // the walk, last cell first: Q + R - 1 cells at most
    float *psim = (float *)(path + Q + R);        // sim along the path, in path order
    signed char *bt = (signed char *)(psim + Q + R);
    unsigned char *acc = (unsigned char *)(bt + cells);

    // ---- (A) the recurrence ------------------------------------------------------------------------------------------
    for (int i0 = 0; i0 < Q; i0 += 64) {
        const int i = i0 + lane;
        const int rows = Q - i0 < 64 ? Q - i0 : 64;
        float cur_dp = 0.0f, prev_dp = 0.0f, above_dp = 0.0f;   // this row at columns j-1 and j-2; lane 0: row i0-1 at column j-1
        int cur_acc = 0, prev_acc = 0, above_acc = 0;
        for (int t = 0; t < R + rows - 1; ++t) {
            const int j = t - lane;
            float up_dp = __shfl_up(cur_dp, 1, 64), ul_dp = __shfl_up(prev_dp, 1, 64);
            int up_acc = __shfl_up(cur_acc, 1, 64), ul_acc = __shfl_up(prev_acc, 1, 64);
            if (lane < rows && j >= 0 && j < R) {
                const int idx = i * R + j;
                const float s = (M[idx] + bias) + 1.0f;
                if (lane == 0 && i > 0) {
                    up_dp = dp[idx - R], up_acc = acc[idx - R];
                    ul_dp = above_dp, ul_acc = above_acc;
                    above_dp = up_dp, above_acc = up_acc;
                }
                float nd = s;
                int na = 0, nb = -1;
                if (i > 0 && j > 0) {
                    const float hs = 0.5f * s;
                    const float c0 = ul_dp + s, c1 = up_dp + hs, c2 = cur_dp + hs;
                    float best = c0;
                    int k = 0;
                    if (c1 > best) best = c1, k = 1;
                    if (c2 > best) best = c2, k = 2;
                    if (s < a.min_sim32) {
                        const int pa = k == 0 ? ul_acc : (k == 1 ? up_acc : cur_acc);
                        na = pa + 1 > 255 ? 255 : pa + 1;
                    }
                    if (na <= a.discontinue) nb = k, nd = best;
                }
                dp[idx] = nd;
                bt[idx] = (signed char)nb;
                acc[idx] = (unsigned char)na;
                prev_dp = cur_dp, prev_acc = cur_acc;
                cur_dp = nd, cur_acc = na;
            }
        }
        __syncthreads();                          // the next strip's lane 0 reads this strip's last row
    }

    // ---- (B) first maximum per row -----------------------------------------------------------------------------------
    for (int i = 0; i < Q; ++i) dp_row_scan(dp, R, i, rowmax, rowarg, lane);
    __syncthreads();

    // ---- (C) rounds --------------------------------------------------------------------------------------------------
    int count = 0;                                // lane 0's is the count
    for (int round = 0; round < AL_ROUNDS; ++round) {
        float bv = -INFINITY;
        int bi = INT_MAX;
        for (int i = lane; i < Q; i += 64) {
            const float v = rowmax[i];
            if (v > bv || (v == bv && i < bi)) bv = v, bi = i;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float ov = al_shfl_xor_f(bv, m);
            const int oi = al_shfl_xor_i(bi, m);
            if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
        }
        if (!(bv > -INFINITY)) break;             // everything is masked (uniform: every lane holds the same maximum)
        int len = 0, first = 0, last = bi * R + rowarg[bi];
        if (lane == 0) {
            int c = last;
            path[len++] = c;
            for (;;) {
                const int b = bt[c];
                if (b < 0) break;
                const int nc = c - (b == 0 ? R + 1 : (b == 1 ? R : 1));
                if (dp[nc] == -INFINITY) break;
                c = nc;
                path[len++] = c;
            }
            first = c;
        }
        len = __shfl(len, 0, 64), first = __shfl(first, 0, 64);
        __syncthreads();                          // the walk is visible
        for (int k = lane; k < len; k += 64) psim[k] = (M[path[len - 1 - k]] + bias) + 1.0f;
        const int r1 = first / R, c1 = first % R, r2 = last / R, c2 = last % R;
        const int w = c2 - c1 + 1, block = (r2 - r1 + 1) * w;
        for (int x = lane; x < block; x += 64) dp[(r1 + x / w) * R + c1 + x % w] = -INFINITY;
        __syncthreads();
        for (int i = r1; i <= r2; ++i) dp_row_scan(dp, R, i, rowmax, rowarg, lane);
        if (lane == 0) {
            // cut_path: consecutive path cells differ by 1 (same row), R (same column) or R + 1 (diagonal); R == 1 has no steps
            auto cell = [&](int k) { return path[len - 1 - k]; };
            auto range = [&](int s, int e) {
                if (!(e - s > a.min_length)) return;
                const float mean = al_pairwise([&](int x) { return psim[s + x]; }, e - s) / (float)(e - s);
                const int p0 = cell(s), p1 = cell(e - 1);
                const int q0 = p0 / R, r0 = p0 % R, q1 = p1 / R, rr1 = p1 % R;
                if (mean > a.ave_sim32 && q1 - q0 > a.min_length && rr1 - r0 > a.min_length) {
                    if (count < slots) {
                        int *g = boxes + 4 * count;
                        g[0] = q0, g[1] = r0, g[2] = q1, g[3] = rr1;
                    }
                    ++count;
                }
            };
            int prev = 0;
            for (int s = 0; s < len - 1;) {
                const int d = cell(s + 1) - cell(s);
                int e = s + 1;
                if (d == R + 1) {
                    s = e;
                    continue;
                }
                while (e < len - 1 && cell(e + 1) - cell(e) == d) ++e;
                if (e + 1 - s > a.diagonal_thres) {   // steps s .. e-1 cover the cells s .. e
                    range(prev, s);
                    prev = e + 1;
                }
                s = e;
            }
            range(prev, len);
        }
        __syncthreads();
    }
    count = __shfl(count, 0, 64);
    if (lane == 0) a.counts[blockIdx.x] = count;
    __syncthreads();

    // ---- (D) MaxSim ---------------------------------------------------------------------------------------------------
    al_maxsim(M, R, bias, boxes, maxsim, count < slots ? count : slots, lane);
}

__global__ __launch_bounds__(64) void hv_align_kernel(HvArgs a) {
    const int lane = threadIdx.x;
    const AlPair P = a.pairs[blockIdx.x];
    const int Q = P.q, R = P.r, slots = a.max_peaks;
    int *boxes = a.boxes + (size_t)blockIdx.x * slots * 4;
    float *maxsim = a.maxsim + (size_t)blockIdx.x * slots;
    al_clear(boxes, maxsim, slots, lane);
    if (Q == 0 || R == 0) {
        if (lane == 0) a.counts[blockIdx.x] = 0;
        return;
    }
    const float *M = a.sims + P.off;
    const float bias = a.bias, min32 = a.min_sim32;
    const int nd = Q + R - 1;                     // diagonal d is sigma = d - (Q - 1)
    float *score = (float *)(a.arena + P.sb);
    unsigned char *state = (unsigned char *)(score + nd);   // 0: no peak, 1: peak, 2: taken

    // ---- (A) diagonal sums ---------------------------------------------------------------------------------------------
    for (int d = lane; d < nd; d += 64) {
        const int sigma = d - (Q - 1);
        const int b = sigma < 0 ? -sigma : 0;
        int e = R - sigma;
        e = e < 0 ? 0 : e, e = e < Q ? e : Q;
        bool peak = false;
        const float *diag = M + (size_t)b * R + b + sigma;
        score[d] = al_pairwise([&](int x) {
            float v = diag[(size_t)x * (R + 1)] + bias;
            if (v < min32) v = 0.0f;
            peak |= v >= min32;
            return v; }, e - b);
        state[d] = peak ? 1 : 0;
    }
    __syncthreads();

    // ---- (B) peaks in descending score, ties to the lower sigma --------------------------------------------------------
    int accepted = 0;
    for (int round = 0; round < a.max_peaks; ++round) {
        float bv = -INFINITY;
        int bd = INT_MAX;
        for (int d = lane; d < nd; d += 64)
            if (state[d] == 1) {
                const float v = score[d];
                if (bd == INT_MAX || v > bv) bv = v, bd = d;   // ascending d inside a lane: an equal score keeps the lower
            }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float ov = al_shfl_xor_f(bv, m);
            const int od = al_shfl_xor_i(bd, m);
            if (od != INT_MAX && (bd == INT_MAX || ov > bv || (ov == bv && od < bd))) bv = ov, bd = od;
        }
        if (bd == INT_MAX || !(bv > 0.0f)) break;  // no peak left, or only scores <= 0 left: none of them gives a box
        const int sigma = bd - (Q - 1);
        const int b = sigma < 0 ? -sigma : 0;
        int e = R - sigma;
        e = e < 0 ? 0 : e, e = e < Q ? e : Q;
        const int x1 = b, y1 = b + sigma, x2 = e - 1, y2 = e - 1 + sigma;
        bool over = accepted == 0 && 0.0 > a.iou_thresh;
        for (int j = lane; j < accepted; j += 64) {
            const int *g = boxes + 4 * j;
            long long iw = (long long)min(x2, g[2]) - max(x1, g[0]) + 1, ih = (long long)min(y2, g[3]) - max(y1, g[1]) + 1;
            iw = iw > 0 ? iw : 0, ih = ih > 0 ? ih : 0;
            const long long inter = iw * ih;
            const long long ua = ((long long)x2 - x1 + 1) * ((long long)y2 - y1 + 1) +
                                 ((long long)g[2] - g[0] + 1) * ((long long)g[3] - g[1] + 1) - inter;
            over |= (double)inter / (double)ua > a.iou_thresh;
        }
        const bool reject = __ballot(over) != 0ull;
        if (lane == 0) {
            state[bd] = 2;
            if (!reject) {
                int *g = boxes + 4 * accepted;
                g[0] = x1, g[1] = y1, g[2] = x2, g[3] = y2;
            }
        }
        if (!reject) ++accepted;                  // at most max_peaks: every accepted box is stored
        __syncthreads();
    }
    if (lane == 0) a.counts[blockIdx.x] = accepted;
    __syncthreads();

    // ---- (D) MaxSim ---------------------------------------------------------------------------------------------------
    al_maxsim(M, R, bias, boxes, maxsim, accepted, lane);
}

inline size_t dp_pair_bytes(int64_t q, int64_t r) {
    if (q == 0 || r == 0) return 0;
    const size_t cells = (size_t)(q * r);
    return (4 * cells + 8 * (size_t)q + 8 * (size_t)(q + r) + 2 * cells + 15) & ~(size_t)15;
}

inline size_t hv_pair_bytes(int64_t q, int64_t r) {
    if (q == 0 || r == 0) return 0;
    return (5 * (size_t)(q + r - 1) + 15) & ~(size_t)15;
}

}  // namespace

// the handle: the stream every call enqueues on, the scratch cap and what the last call used; it owns no device memory
struct vsc_align {
    hipStream_t stream;
    int64_t cap, last_launches, scratch_bytes;
};

namespace {

// Validates the pair table, lays the pairs' scratch out in launches of at most h->cap bytes (a launch holds at least one pair)
// and uploads the table.  -> the launches as [first, end) pair ranges, the device table, the arena.
int align_plan(vsc_align *h, const char *who, const float *sims_dev, int64_t sims_len, const int64_t *pairs_host, int64_t n_pairs,
               size_t (*pair_bytes)(int64_t, int64_t), std::vector<int64_t> &cuts, const AlPair **table_dev, char **arena) {
    static thread_local std::vector<AlPair> table;
    table.resize((size_t)n_pairs);
    cuts.assign(1, 0);
    size_t used = 0, most = 0;
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int64_t off = pairs_host[3 * p], q = pairs_host[3 * p + 1], r = pairs_host[3 * p + 2];
        VSC_REQUIRE(q >= 0 && q <= AL_MAX_DIM && r >= 0 && r <= AL_MAX_DIM, "%s: pair %lld is %lld x %lld (limit %d rows and columns)", who,
                    (long long)p, (long long)q, (long long)r, AL_MAX_DIM);
        VSC_REQUIRE(q * r <= AL_MAX_CELLS, "%s: pair %lld is %lld x %lld (limit %lld cells)", who, (long long)p, (long long)q,
                    (long long)r, AL_MAX_CELLS);
        VSC_REQUIRE(off >= 0 && off + q * r <= sims_len && (q * r == 0 || sims_dev),
                    "%s: pair %lld = (%lld, %lld, %lld) outside the %lld similarities", who, (long long)p, (long long)off, (long long)q,
                    (long long)r, (long long)sims_len);
        const size_t need = pair_bytes(q, r);
        if (used && used + need > (size_t)h->cap) {
            cuts.push_back(p);
            used = 0;
        }
        table[p] = AlPair{off, (long long)used, (int)q, (int)r};
        used += need;
        most = used > most ? used : most;
    }
    cuts.push_back(n_pairs);
    void *tt, *ar;
    VSC_TRY(search_scratch_get(SCRATCH_ALIGN_TABLE, (size_t)n_pairs * sizeof(AlPair), &tt));
    VSC_TRY(search_scratch_get(SCRATCH_ALIGN_ARENA, most, &ar));
    VSC_CHECK_HIP(hipMemcpyAsync(tt, table.data(), table.size() * sizeof(AlPair), hipMemcpyHostToDevice, h->stream));
    VSC_CHECK_HIP(hipStreamSynchronize(h->stream));   // `table` is reused by the next call
    *table_dev = (const AlPair *)tt, *arena = (char *)ar;
    h->last_launches = (int64_t)cuts.size() - 1;
    h->scratch_bytes = (int64_t)most;
    return VSC_OK;
}

}  // namespace

extern "C" int vsc_align_create(void *stream, vsc_align **out) {
    VSC_REQUIRE(out, "align_create: null pointer");
    *out = new vsc_align{(hipStream_t)stream, AL_DEFAULT_CAP, 0, 0};
    return VSC_OK;
}

extern "C" void vsc_align_destroy(vsc_align *h) { delete h; }

extern "C" int vsc_align_scratch(vsc_align *h, int64_t cap_bytes, int64_t *last_launches, int64_t *scratch_bytes) {
    VSC_REQUIRE(h, "align_scratch: null handle");
    VSC_REQUIRE(cap_bytes >= 0, "align_scratch: cap_bytes %lld < 0 (0 keeps the cap)", (long long)cap_bytes);
    if (cap_bytes > 0) h->cap = cap_bytes;
    if (last_launches) *last_launches = h->last_launches;
    if (scratch_bytes) *scratch_bytes = h->scratch_bytes;
    return VSC_OK;
}

extern "C" int vsc_align_dp_f32(vsc_align *h, const float *sims_dev, int64_t sims_len, const int64_t *pairs_host, int64_t n_pairs, float bias,
                                int32_t discontinue, double min_sim, double ave_sim, int32_t min_length, int32_t diagonal_thres,
                                int32_t max_boxes, int32_t *boxes_dev, int32_t *counts_dev, float *maxsim_dev) {
    VSC_REQUIRE(h, "align_dp: null handle");
    VSC_REQUIRE(n_pairs >= 0 && n_pairs < (1ll << 31), "align_dp: %lld pairs", (long long)n_pairs);
    VSC_REQUIRE(discontinue >= 0 && discontinue <= AL_MAX_DISCONTINUE, "align_dp: discontinue %d outside [0, %d]", discontinue,
                AL_MAX_DISCONTINUE);
    VSC_REQUIRE(min_length >= 0, "align_dp: min_length %d < 0", min_length);
    VSC_REQUIRE(diagonal_thres >= 0, "align_dp: diagonal_thres %d < 0", diagonal_thres);
    VSC_REQUIRE(max_boxes >= 1 && max_boxes <= AL_MAX_BOXES, "align_dp: max_boxes %d outside [1, %d]", max_boxes, AL_MAX_BOXES);
    h->last_launches = 0;
    if (n_pairs == 0) return VSC_OK;
    VSC_REQUIRE(pairs_host && boxes_dev && counts_dev && maxsim_dev, "align_dp: null pointer");
    std::vector<int64_t> cuts;
    DpArgs a;
    const AlPair *table;
    VSC_TRY(align_plan(h, "align_dp", sims_dev, sims_len, pairs_host, n_pairs, dp_pair_bytes, cuts, &table, &a.arena));
    a.sims = sims_dev;
    a.bias = bias, a.min_sim32 = (float)min_sim, a.ave_sim32 = (float)ave_sim;
    a.discontinue = discontinue, a.min_length = min_length, a.diagonal_thres = diagonal_thres, a.max_boxes = max_boxes;
    for (size_t c = 0; c + 1 < cuts.size(); ++c) {
        const int64_t p0 = cuts[c], n = cuts[c + 1] - p0;
        a.pairs = table + p0;
        a.boxes = boxes_dev + p0 * max_boxes * 4, a.counts = counts_dev + p0, a.maxsim = maxsim_dev + p0 * max_boxes;
        hipLaunchKernelGGL(dp_align_kernel, dim3((unsigned)n), dim3(64), 0, h->stream, a);
        VSC_CHECK_LAUNCH();
    }
    return VSC_OK;
}

extern "C" int vsc_align_hv_f32(vsc_align *h, const float *sims_dev, int64_t sims_len, const int64_t *pairs_host, int64_t n_pairs, float bias,
                                double min_sim, double iou_thresh, int32_t max_peaks, int32_t *boxes_dev, int32_t *counts_dev,
                                float *maxsim_dev) {
    VSC_REQUIRE(h, "align_hv: null handle");
    VSC_REQUIRE(n_pairs >= 0 && n_pairs < (1ll << 31), "align_hv: %lld pairs", (long long)n_pairs);
    VSC_REQUIRE(max_peaks >= 1 && max_peaks <= AL_MAX_BOXES, "align_hv: max_peaks %d outside [1, %d]", max_peaks, AL_MAX_BOXES);
    h->last_launches = 0;
    if (n_pairs == 0) return VSC_OK;
    VSC_REQUIRE(pairs_host && boxes_dev && counts_dev && maxsim_dev, "align_hv: null pointer");
    std::vector<int64_t> cuts;
    HvArgs a;
    const AlPair *table;
    VSC_TRY(align_plan(h, "align_hv", sims_dev, sims_len, pairs_host, n_pairs, hv_pair_bytes, cuts, &table, &a.arena));
    a.sims = sims_dev;
    a.bias = bias, a.min_sim32 = (float)min_sim, a.iou_thresh = iou_thresh, a.max_peaks = max_peaks;
    for (size_t c = 0; c + 1 < cuts.size(); ++c) {
        const int64_t p0 = cuts[c], n = cuts[c + 1] - p0;
        a.pairs = table + p0;
        a.boxes = boxes_dev + p0 * max_peaks * 4, a.counts = counts_dev + p0, a.maxsim = maxsim_dev + p0 * max_peaks;
        hipLaunchKernelGGL(hv_align_kernel, dim3((unsigned)n), dim3(64), 0, h->stream, a);
        VSC_CHECK_LAUNCH();
    }
    return VSC_OK;
}
