// Temporal-network (TN) alignment of candidate-pair similarity matrices (VCSL's `tn`, infer/vcsl/vta.py:244-363), batched:
// one wave per pair, the pairs of a launch independent.  The contract is stated with vsc_tn_align_f32 in include/vsc_hip.h.
//
// Per pair, in one workgroup of 64 lanes:
//  (A) top-K per row: each lane keeps a sorted top-K of its strided columns, then K wave-wide argmax rounds merge them
//      (descending biased similarity, ties to the lower column).  The matrix is read once; the bias is added on the fly.
//  (B) predecessor bitmasks: a lane per source row q_i walks q_j = q_i+1 .. q_i+max_step-1 with the running C3 set kept as
//      "smallest intermediate column above col_i" per source node, and ORs edge bits into the target's 64-bit mask
//      (bit (max_step-1-d)*top + c for the source (q_j-d, c): ascending bits = the reference's predecessor order).
//  (C) Kahn ranks, once per pair (the graph never changes, only its weights): generation 0 in node-id order, then every
//      node's successors in (q_j, k) order with the sink edge last -- networkx's topological_sort order.
//  (D) up to max_path+1 rounds: longest-path DP row by row (dist of the last max_step+1 rows in an LDS ring), argmax with
//      ties to the lower rank, traceback, zeroed-edge bits, then box / density / IoU tests on lane 0.
//  (E) MaxSim of every accepted box: max of (s + bias) over the half-open box, minus bias.
// Per-node state lives in the search path's grow-only device scratch (knn.hip).
#include <climits>
#include <vector>

#include "common.h"

namespace {

constexpr int TN_MAX_TOPK = 16;      // top_k limit (register arrays of phases A and B)
constexpr int TN_MASK_BITS = 64;     // (max_step - 1) * top_k limit: predecessor bits per node
constexpr int TN_RING = TN_MASK_BITS + 2 * TN_MAX_TOPK;   // (max_step + 1) * top floats of dist
constexpr int TN_MAX_Q = 1 << 16;
constexpr int TN_MAX_R = 1 << 24;

struct TnPair {
    long long off;   // element offset of the [q, r] matrix
    long long nb;    // node base of the pair in the scratch arrays
    int q, r, top, pad;
};

struct TnArgs {
    const float *sims;
    const TnPair *pairs;
    float bias, min_sim32;
    int step, max_path, min_length;
    double min_sim, max_iou;
    int *topcol;
    float *topval;
    unsigned long long *predm, *zerom;
    int *indeg, *queue, *rank, *back;
    int *boxes, *counts;
    float *maxsim;
};

__device__ inline bool tn_better(float v, int c, float bv, int bc) { return v > bv || (v == bv && c < bc); }

__device__ inline float shfl_xor_f(float v, int m) { return __shfl_xor(v, m, 64); }
__device__ inline int shfl_xor_i(int v, int m) { return __shfl_xor(v, m, 64); }

__global__ __launch_bounds__(64) void tn_align_kernel(TnArgs a) {
    const int lane = threadIdx.x;
    const TnPair P = a.pairs[blockIdx.x];
    const int Q = P.q, R = P.r, top = P.top, step = a.step;
    const int slots = a.max_path + 1;
    int *boxes = a.boxes + (size_t)blockIdx.x * slots * 4;
    float *maxsim = a.maxsim + (size_t)blockIdx.x * slots;
    for (int i = lane; i < slots * 4; i += 64) boxes[i] = 0;
    for (int i = lane; i < slots; i += 64) maxsim[i] = 0.0f;
    if (Q == 0 || top == 0) {
        if (lane == 0) a.counts[blockIdx.x] = 0;
        return;
    }
    const float *M = a.sims + P.off;
    const long long nb = P.nb;
    const int N = 1 + Q * top, sink = N - 1;
    int *topcol = a.topcol + nb;
    float *topval = a.topval + nb;
    unsigned long long *predm = a.predm + nb, *zerom = a.zerom + nb;
    int *indeg = a.indeg + nb, *queue = a.queue + nb, *rank = a.rank + nb, *back = a.back + nb;
    const float bias = a.bias;

    // ---- (A) top-K per row ------------------------------------------------------------------------------------------
    for (int q = 0; q < Q; ++q) {
        const float *row = M + (size_t)q * R;
        float kv[TN_MAX_TOPK];
        int kc[TN_MAX_TOPK];
#pragma unroll
        for (int i = 0; i < TN_MAX_TOPK; ++i) kv[i] = -INFINITY, kc[i] = INT_MAX;
        float worst = -INFINITY;
        for (int c = lane; c < R; c += 64) {
            const float v = row[c] + bias;
            if (!(v > worst)) continue;          // an equal value keeps the earlier (lower) column of this lane
            float cv = v;
            int cc = c;
            bool shift = false;
#pragma unroll
            for (int i = 0; i < TN_MAX_TOPK; ++i)
                if (i < top) {
                    if (shift || cv > kv[i]) {
                        const float tv = kv[i];
                        const int tc = kc[i];
                        kv[i] = cv, kc[i] = cc, cv = tv, cc = tc;
                        shift = true;
                    }
                    if (i == top - 1) worst = kv[i];
                }
        }
        for (int t = 0; t < top; ++t) {
            float bv = kv[0];
            int bc = kc[0];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const float ov = shfl_xor_f(bv, m);
                const int oc = shfl_xor_i(bc, m);
                if (tn_better(ov, oc, bv, bc)) bv = ov, bc = oc;
            }
            if (kc[0] == bc) {                   // columns are unique across lanes: the owner pops its head
#pragma unroll
                for (int i = 0; i + 1 < TN_MAX_TOPK; ++i) kv[i] = kv[i + 1], kc[i] = kc[i + 1];
                kv[TN_MAX_TOPK - 1] = -INFINITY, kc[TN_MAX_TOPK - 1] = INT_MAX;
            }
            if (lane == 0) topcol[1 + q * top + t] = bc, topval[1 + q * top + t] = bv;
        }
    }
    for (int v = lane; v < N; v += 64) predm[v] = 0ull, zerom[v] = 0ull;
    __syncthreads();

    // ---- (B) predecessor bitmasks ------------------------------------------------------------------------------------
    for (int qi = lane; qi < Q; qi += 64) {
        int ci[TN_MAX_TOPK], nx[TN_MAX_TOPK];
#pragma unroll
        for (int c = 0; c < TN_MAX_TOPK; ++c) {
            ci[c] = c < top ? topcol[1 + qi * top + c] : INT_MAX;
            nx[c] = INT_MAX;                      // smallest column of the intermediate set above ci[c]
        }
        for (int d = 1; d < step && qi + d < Q; ++d) {
            const int qj = qi + d;
            unsigned valid = 0;
            for (int k = 0; k < top; ++k) {
                const int colj = topcol[1 + qj * top + k];
                if (!(topval[1 + qj * top + k] >= a.min_sim32)) continue;     // C4
                unsigned long long bits = 0;
#pragma unroll
                for (int c = 0; c < TN_MAX_TOPK; ++c)
                    if (c < top) {
                        const int diff = colj - ci[c];
                        if (diff > 0 && diff < step && !(nx[c] < colj))      // C2, C3
                            bits |= 1ull << ((step - 1 - d) * top + c);
                    }
                if (bits) {
                    atomicOr(&predm[1 + qj * top + k], bits);
                    valid |= 1u << k;
                }
            }
            for (; valid; valid &= valid - 1) {   // the set grows after each q_j
                const int x = topcol[1 + qj * top + __builtin_ctz(valid)];
#pragma unroll
                for (int c = 0; c < TN_MAX_TOPK; ++c)
                    if (x > ci[c] && x < nx[c]) nx[c] = x;
            }
        }
    }
    __syncthreads();

    // ---- sink edges: every node i < N-1 (source included) with q_sink > q_i, col_sink > col_i, both gaps <= max_step.
    // R = regular predecessors of the sink (all of them satisfy it); S \ R are appended in node-id order.  Every edge
    // into the sink weighs 0.
    __shared__ int s_only[TN_RING];
    __shared__ int s_only_n;
    const int qs = Q - 1, cs = topcol[sink];
    const unsigned long long sink_mask = predm[sink];
    if (lane == 0) {
        int n = 0;
        if (Q <= step && cs + 1 <= step) s_only[n++] = 0;
        for (int q = qs - step < 0 ? 0 : qs - step; q < qs; ++q)
            for (int k = 0; k < top; ++k) {
                const int col = topcol[1 + q * top + k];
                if (!(col < cs && cs - col <= step)) continue;
                const int d = qs - q;
                if (d < step && ((sink_mask >> ((step - 1 - d) * top + k)) & 1ull)) continue;   // in R
                s_only[n++] = 1 + q * top + k;
            }
        s_only_n = n;
    }
    __syncthreads();
    const int n_sonly = s_only_n;

    // ---- (C) Kahn ranks ----------------------------------------------------------------------------------------------
    for (int v = lane; v < N; v += 64) indeg[v] = v == 0 ? 0 : (v == sink ? __popcll(sink_mask) + n_sonly : __popcll(predm[v]));
    __syncthreads();
    int tail = 0;
    for (int base = 0; base < N; base += 64) {
        const int v = base + lane;
        const bool z = v < N && indeg[v] == 0;
        const unsigned long long bal = __ballot(z);
        if (z) {
            const int pos = tail + __popcll(bal & ((1ull << lane) - 1ull));
            queue[pos] = v;
            rank[v] = pos;
        }
        tail += __popcll(bal);
    }
    __syncthreads();
    const int nbits = (step - 1) * top;
    for (int head = 0; head < tail; ++head) {
        const int u = queue[head];
        bool z = false;
        int v = 0;
        if (u != 0 && lane < nbits) {
            const int qu = (u - 1) / top, cu = (u - 1) % top;
            const int d = 1 + lane / top, k = lane % top;
            if (qu + d < Q) {
                v = 1 + (qu + d) * top + k;
                if ((predm[v] >> ((step - 1 - d) * top + cu)) & 1ull) {
                    const int left = indeg[v] - 1;
                    indeg[v] = left;
                    z = left == 0;
                }
            }
        }
        const unsigned long long bal = __ballot(z);
        if (z) {
            const int pos = tail + __popcll(bal & ((1ull << lane) - 1ull));
            queue[pos] = v;
            rank[v] = pos;
        }
        tail += __popcll(bal);
        bool in_s_only = false;                   // the new sink edge, last in u's successor list
        for (int i = 0; i < n_sonly; ++i) in_s_only |= s_only[i] == u;
        if (in_s_only) {
            int left = 1;
            if (lane == 0) {
                left = indeg[sink] - 1;
                indeg[sink] = left;
                if (left == 0) queue[tail] = sink, rank[sink] = tail;
            }
            if (__shfl(left, 0, 64) == 0) ++tail;
        }
        __syncthreads();
    }

    // ---- (D) path rounds ---------------------------------------------------------------------------------------------
    if (lane == 0) back[0] = 0;                   // the source has no predecessor: tracebacks end there
    __syncthreads();
    __shared__ float ring[TN_RING];
    const int ring_rows = step + 1;
    int accepted = 0;
    for (int round = 0; round < slots; ++round) {
        // lane k keeps the best (dist, rank) of its nodes; lane 0 starts with the source (dist 0, rank 0)
        float best_d = lane == 0 ? 0.0f : -INFINITY;
        int best_r = lane == 0 ? rank[0] : INT_MAX, best_v = 0;
        for (int qj = 0; qj < Q; ++qj) {
            if (lane < top) {
                const int v = 1 + qj * top + lane;
                float bd = 0.0f;
                int bu = v;
                bool have = false;
                if (v == sink) {
                    for (unsigned long long m = sink_mask; m; m &= m - 1) {
                        const int b = __builtin_ctzll(m);
                        const int d = step - 1 - b / top, c = b % top;
                        const float x = ring[((qj - d) % ring_rows) * top + c] + 0.0f;
                        if (!have || x > bd) bd = x, bu = 1 + (qj - d) * top + c, have = true;
                    }
                    for (int i = 0; i < n_sonly; ++i) {
                        const int u = s_only[i];
                        const float x = (u == 0 ? 0.0f : ring[(((u - 1) / top) % ring_rows) * top + (u - 1) % top]) + 0.0f;
                        if (!have || x > bd) bd = x, bu = u, have = true;
                    }
                } else {
                    const unsigned long long pm = predm[v], zm = zerom[v];
                    const float w = topval[v];
                    for (unsigned long long m = pm; m; m &= m - 1) {
                        const int b = __builtin_ctzll(m);
                        const int d = step - 1 - b / top, c = b % top;
                        const float x = ring[((qj - d) % ring_rows) * top + c] + (((zm >> b) & 1ull) ? 0.0f : w);
                        if (!have || x > bd) bd = x, bu = 1 + (qj - d) * top + c, have = true;
                    }
                }
                if (!have || !(bd >= 0.0f)) bd = 0.0f, bu = v;
                ring[(qj % ring_rows) * top + lane] = bd;
                back[v] = bu;
                const int rv = rank[v];
                if (bd > best_d || (bd == best_d && rv < best_r)) best_d = bd, best_r = rv, best_v = v;
            }
            __syncthreads();
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float od = shfl_xor_f(best_d, m);
            const int orr = shfl_xor_i(best_r, m), ov = shfl_xor_i(best_v, m);
            if (od > best_d || (od == best_d && orr < best_r)) best_d = od, best_r = orr, best_v = ov;
        }
        int stop = 0;
        if (lane == 0) {
            // traceback into queue[] (free after phase C), reversed
            int len = 0, v = best_v;
            queue[len++] = v;
            while (back[v] != v && len < N) v = back[v], queue[len++] = v;   // a path holds at most Q + 1 <= N nodes
            // zero the path's edges (u -> v, v a regular node; edges into the sink weigh 0 already)
            for (int i = len - 1; i > 0; --i) {
                const int u = queue[i], w = queue[i - 1];
                if (w == sink || u == 0) continue;
                const int d = (w - 1) / top - (u - 1) / top, c = (u - 1) % top;
                zerom[w] |= 1ull << ((step - 1 - d) * top + c);
            }
            float score = 0.0f;
            int n = 0, qmin = INT_MAX, qmax = INT_MIN, rmin = INT_MAX, rmax = INT_MIN;
            for (int i = len - 1; i >= 0; --i) {  // path order
                const int u = queue[i];
                if (u == 0 || u == sink) continue;
                score = score + topval[u];
                const int q = (u - 1) / top, r = topcol[u];
                qmin = min(qmin, q), qmax = max(qmax, q), rmin = min(rmin, r), rmax = max(rmax, r);
                ++n;
            }
            if (n == 0) {
                stop = 1;
            } else {
                if (!(score > 0.0f)) qmin = qmax = rmin = rmax = 0;
                const long long dq = (long long)qmax - qmin, dr = (long long)rmax - rmin;
                const double ave = (double)(dr + dq) / 2.0;
                bool ok = score > 0.0f && (double)score / ave > a.min_sim && (dr < dq ? dr : dq) > a.min_length;
                if (ok) {
                    double worst_iou = 0.0;
                    for (int j = 0; j < accepted; ++j) {
                        const int *g = boxes + 4 * j;
                        long long iw = (long long)min(qmax, g[2]) - max(qmin, g[0]) + 1, ih = (long long)min(rmax, g[3]) - max(rmin, g[1]) + 1;
                        iw = iw > 0 ? iw : 0, ih = ih > 0 ? ih : 0;
                        const long long inter = iw * ih;
                        const long long ua = (dq + 1) * (dr + 1) + ((long long)g[2] - g[0] + 1) * ((long long)g[3] - g[1] + 1) - inter;
                        const double iou = (double)inter / (double)ua;
                        if (iou > worst_iou) worst_iou = iou;
                    }
                    ok = worst_iou < a.max_iou;
                }
                if (ok) {
                    int *g = boxes + 4 * accepted;
                    g[0] = qmin, g[1] = rmin, g[2] = qmax, g[3] = rmax;
                    ++accepted;
                }
            }
        }
        stop = __shfl(stop, 0, 64);
        accepted = __shfl(accepted, 0, 64);
        __syncthreads();
        if (stop) break;
    }
    if (lane == 0) a.counts[blockIdx.x] = accepted;

    // ---- (E) MaxSim per accepted box ---------------------------------------------------------------------------------
    for (int j = 0; j < accepted; ++j) {
        const int x1 = boxes[4 * j], y1 = boxes[4 * j + 1], x2 = boxes[4 * j + 2], y2 = boxes[4 * j + 3];
        const long long w = y2 - y1, cells = (long long)(x2 - x1) * w;
        float m = -INFINITY;
        for (long long i = lane; i < cells; i += 64) {
            const float v = M[(size_t)(x1 + i / w) * R + y1 + i % w] + bias;
            m = v > m ? v : m;
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const float o = shfl_xor_f(m, s);
            m = o > m ? o : m;
        }
        if (lane == 0) maxsim[j] = m - bias;
    }
}

}  // namespace

int launch_tn_align(const float *sims_dev, int64_t sims_len, const int64_t *pairs_host, int64_t n_pairs, float bias, int max_step,
                    int top_k, int max_path, double min_sim, int min_length, double max_iou, int32_t *boxes_dev, int32_t *counts_dev,
                    float *maxsim_dev, hipStream_t stream) {
    VSC_REQUIRE(n_pairs >= 0 && n_pairs < (1ll << 31), "tn_align: %lld pairs", (long long)n_pairs);
    VSC_REQUIRE(max_step >= 1, "tn_align: max_step %d < 1", max_step);
    VSC_REQUIRE(top_k >= 1 && top_k <= TN_MAX_TOPK, "tn_align: top_k %d outside [1, %d]", top_k, TN_MAX_TOPK);
    VSC_REQUIRE((int64_t)(max_step - 1) * top_k <= TN_MASK_BITS,
                "tn_align: (max_step - 1) * top_k = %lld exceeds the %d predecessor bits of a node", (long long)(max_step - 1) * top_k,
                TN_MASK_BITS);
    VSC_REQUIRE(max_path >= 0 && max_path < 4096, "tn_align: max_path %d outside [0, 4095]", max_path);
    VSC_REQUIRE(min_length >= 0, "tn_align: min_length %d < 0 (MaxSim needs a non-empty box)", min_length);
    if (n_pairs == 0) return VSC_OK;
    VSC_REQUIRE(pairs_host && boxes_dev && counts_dev && maxsim_dev, "tn_align: null pointer");
    static thread_local std::vector<TnPair> table;
    table.resize((size_t)n_pairs);
    long long nodes = 0;
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int64_t off = pairs_host[3 * p], q = pairs_host[3 * p + 1], r = pairs_host[3 * p + 2];
        VSC_REQUIRE(q >= 0 && q <= TN_MAX_Q && r >= 0 && r <= TN_MAX_R, "tn_align: pair %lld is %lld x %lld (limits %d x %d)",
                    (long long)p, (long long)q, (long long)r, TN_MAX_Q, TN_MAX_R);
        VSC_REQUIRE(off >= 0 && off + q * r <= sims_len && (q * r == 0 || sims_dev),
                    "tn_align: pair %lld = (%lld, %lld, %lld) outside the %lld similarities", (long long)p, (long long)off,
                    (long long)q, (long long)r, (long long)sims_len);
        const int top = (int)(r < top_k ? r : top_k);
        table[p] = TnPair{off, nodes, (int)q, (int)r, top, 0};
        nodes += 1 + q * top;
    }
    VSC_REQUIRE(nodes < (1ll << 31), "tn_align: %lld graph nodes in one launch", nodes);
    void *tt, *arena;
    int rc;
    if ((rc = search_scratch_get(SCRATCH_TN_TABLE, (size_t)n_pairs * sizeof(TnPair), &tt))) return rc;
    const size_t n = (size_t)nodes;
    if ((rc = search_scratch_get(SCRATCH_TN_NODES, n * 40, &arena))) return rc;   // 2 x 8 + 6 x 4 bytes per node
    VSC_CHECK_HIP(hipMemcpyAsync(tt, table.data(), table.size() * sizeof(TnPair), hipMemcpyHostToDevice, stream));
    VSC_CHECK_HIP(hipStreamSynchronize(stream));  // `table` is reused by the next call
    TnArgs a;
    a.sims = sims_dev;
    a.pairs = (const TnPair *)tt;
    a.bias = bias;
    a.min_sim32 = (float)min_sim;                 // C4 compares the fp32 similarity with float32(min_sim)
    a.step = max_step, a.max_path = max_path, a.min_length = min_length;
    a.min_sim = min_sim, a.max_iou = max_iou;
    char *base = (char *)arena;
    a.predm = (unsigned long long *)base, base += n * 8;
    a.zerom = (unsigned long long *)base, base += n * 8;
    a.topcol = (int *)base, base += n * 4;
    a.topval = (float *)base, base += n * 4;
    a.indeg = (int *)base, base += n * 4;
    a.queue = (int *)base, base += n * 4;
    a.rank = (int *)base, base += n * 4;
    a.back = (int *)base;
    a.boxes = boxes_dev, a.counts = counts_dev, a.maxsim = maxsim_dev;
    hipLaunchKernelGGL(tn_align_kernel, dim3((unsigned)n_pairs), dim3(64), 0, stream, a);
    VSC_CHECK_LAUNCH();
    return VSC_OK;
}
