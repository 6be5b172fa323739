// Fused multi-head self-attention for ANY ViT token count (1 .. VSC_ATTENTION_STREAM_MAX_TOKENS), head_dim 64:
//   out[f, t, h*64:(h+1)*64] = softmax(q k^T / 8) v          per frame f and head h
// in the qkv / output layout of attention.hip.  attention_kernel there keeps a whole score row in registers and stops at 320
// tokens; this one streams K and V in key blocks of KB = VSC_ATTENTION_STREAM_KEY_BLOCK with an online softmax: a running row
// maximum m and a running row sum l per query.
//
// Organisation: one workgroup (8 waves) per (frame, head, block of 128 queries); a wave owns 16 queries for the whole launch.
//   * what attention.hip has paid for is kept: scores are computed swapped, mfma(A = K fragment, B = Q fragment) gives
//     D[key][query], so a lane holds the scores of ONE query (lane & 15) and m, l and the rescale factor are in-lane scalars (two
//     xor-shuffles per block for the maximum, no LDS round trip); the probabilities, rounded to the operand type, are directly the
//     B operand of the PV MFMA; the row sum is the sum of those ROUNDED probabilities, taken on the matrix pipe with an A operand of
//     ones in the accumulation order of the PV products; K is staged row-major with the chunk swizzle, V transposed with the key
//     permutation of attention.hip; O leaves as whole 128-byte rows through 2 KiB of wave-private LDS.
//   * K / V double buffer in REGISTERS: the global loads of key block b + 1 are issued before the MFMAs of block b and written to
//     the (single) LDS image after them, behind a barrier -- the issue-early / write-late split.  Waves 0..3 carry V (one task =
//     4 keys x 8 head-dim columns), waves 4..7 carry K (four 16-byte chunks per thread): 16 staging VGPRs per thread either way.
//   * rescale rule: the maximum is taken EXACTLY at every block.  m' = max(m, block maximum); alpha = exp2((m - m') * c) with
//     c = log2(e) / 8 multiplies O and l once; the block's probabilities are exp2(s c - m' c), so nothing that was exponentiated
//     against m' is touched again.  Where the maximum does not move alpha is exp2(0) = 1.0 and the multiplication is the identity.
//   * first block: m starts at -FLT_MAX (finite), so alpha = exp2(-huge) = 0 multiplies the zero accumulators and no
//     (-inf) - (-inf) occurs.  Pad keys exist only in the last key block (which always holds at least one real key) and are masked
//     to -inf there only; their K and V rows are zeros in LDS (never read from memory: row < tokens guards every load, so a frame
//     reads nothing of the frame behind it).
#include <float.h>

#include "common.h"

namespace {

constexpr int DH = 64;
constexpr int KB = VSC_ATTENTION_STREAM_KEY_BLOCK;   // keys per block
constexpr int QB = 128;                              // queries per workgroup: 8 waves x 16
static_assert(KB == 128, "the staging split (waves 0..3: V, waves 4..7: K) and the tile counts below are written for 128 keys");
constexpr int VSTRIDE = KB * 2 + 32;                 // bytes per head-dim row of V^T (attention.hip: conflict-free ds_read_b128)
constexpr int LDS_K = KB * 128, LDS_V = 64 * VSTRIDE, LDS_O = 8 * 2048;
constexpr int LDS_BYTES = LDS_K + LDS_V + LDS_O;     // 51 200: three workgroups fit a CU's 160 KiB

__device__ __forceinline__ float max3(float a, float b, float c) {   // attention.hip: scores are never signalling NaNs
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

__global__ __launch_bounds__(512, 4) void attention_stream_kernel(const uint16_t *__restrict__ qkv, uint16_t *__restrict__ out,
                                                                  int tokens, int heads, int qblocks) {
    lp_kernel_entry();
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *klds = smem;                  // [KB][64], 128-byte rows, chunk ^= (row >> 1) & 7
    char *vt = smem + LDS_K;            // [64][VSTRIDE]
    char *ost = vt + LDS_V;             // 8 waves x 2 KiB: write-out transposition

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int item = (int)blockIdx.x / qblocks, qb = (int)blockIdx.x - item * qblocks;   // consecutive workgroups share K / V in L2
    const int frame = item / heads, head = item - frame * heads;
    const int width = heads * DH;
    const int64_t ld = 3 * (int64_t)width;
    const int fr = lane & 15, g = lane >> 4;
    const float scale = 0.125f * 1.44269504088896340736f;  // 1/sqrt(64) * log2(e)
    const uint16_t *qptr = qkv + (int64_t)frame * tokens * ld + head * DH;
    const uint16_t *kptr = qptr + width, *vptr = qptr + 2 * width;
    const int nb = (tokens + KB - 1) / KB;
    const int q0 = qb * QB + wave * 16;            // this wave's first query
    const bool active = q0 < tokens;               // wave-uniform; an idle wave still stages and keeps the barriers

    bf16x8_t qf[2];
    {
        int qrow = q0 + fr;
        qrow = qrow < tokens ? qrow : tokens - 1;
        qf[0] = *(const bf16x8_t *)(qptr + qrow * ld + g * 8);
        qf[1] = *(const bf16x8_t *)(qptr + qrow * ld + g * 8 + 32);
    }

    // ---- staging of one key block through registers.  V task e = tid (0..255) as in attention.hip: 16 consecutive lanes take 16
    //      consecutive 4-key groups of one 8-column block.  K chunk e = (tid - 256) + 256 i.
    const int vc8 = (tid >> 4) & 7, vkg = (tid >> 7) * 16 + (tid & 15);
    auto load_kv = [&](int kb0, uint4 (&st)[4]) {
        if (wave < 4) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = kb0 + vkg * 4 + i;
                st[i] = make_uint4(0, 0, 0, 0);
                if (row < tokens) st[i] = *(const uint4 *)(vptr + row * ld + vc8 * 8);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = tid - 256 + i * 256, row = kb0 + (e >> 3);
                st[i] = make_uint4(0, 0, 0, 0);
                if (row < tokens) st[i] = *(const uint4 *)(kptr + row * ld + (e & 7) * 8);
            }
        }
    };
    auto store_kv = [&](const uint4 (&st)[4]) {
        if (wave < 4) {
            const uint32_t *w0 = (const uint32_t *)&st[0], *w1 = (const uint32_t *)&st[1], *w2 = (const uint32_t *)&st[2],
                           *w3 = (const uint32_t *)&st[3];
            char *dst = vt + (vc8 * 8) * VSTRIDE + ((vkg & ~7) | ((vkg & 3) << 1) | ((vkg >> 2) & 1)) * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int sh = (j & 1) * 16;
                uint2 pk;
                pk.x = ((w0[j >> 1] >> sh) & 0xffffu) | (((w1[j >> 1] >> sh) & 0xffffu) << 16);
                pk.y = ((w2[j >> 1] >> sh) & 0xffffu) | (((w3[j >> 1] >> sh) & 0xffffu) << 16);
                *(uint2 *)(dst + j * VSTRIDE) = pk;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = tid - 256 + i * 256, row = e >> 3, c = e & 7;
                *(uint4 *)(klds + row * 128 + ((c ^ ((row >> 1) & 7)) << 4)) = st[i];
            }
        }
    };

    float m = -FLT_MAX;
    f32x4_t osum = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    f32x4_t o[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) o[ct] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    auto compute = [&](int kb0, bool last) {
        // scores: s[t][r] = <q[query = fr], k[key = kb0 + 16 t + 4 g + r]>
        f32x4_t s[KB / 16];
#pragma unroll
        for (int t = 0; t < KB / 16; ++t) {
            s[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
            const int krow = t * 16 + fr;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const bf16x8_t kf = *(const bf16x8_t *)(klds + krow * 128 + (((g + 4 * kk) ^ ((krow >> 1) & 7)) << 4));
                s[t] = lp_mfma16(kf, qf[kk], s[t]);
            }
            if ((t & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        if (last) {   // workgroup-uniform: pad keys exist in the last key block only
#pragma unroll
            for (int t = 0; t < KB / 16; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (kb0 + t * 16 + g * 4 + r >= tokens) s[t][r] = -INFINITY;
        }
        float mx = m;   // the running maximum joins the block's: m' = max(m, block maximum), exactly
#pragma unroll
        for (int t = 0; t < KB / 16; ++t) mx = max3(max3(mx, s[t][0], s[t][1]), s[t][2], s[t][3]);
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float alpha = __builtin_amdgcn_exp2f((m - mx) * scale);   // first block: exp2(-huge) = 0 on zero accumulators
        m = mx;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) o[ct] *= alpha;
        osum *= alpha;
        const float mxs = mx * scale;
        const f32x2_t sc2 = (f32x2_t){scale, scale}, nm2 = (f32x2_t){-mxs, -mxs};
        bf16x8_t pb[KB / 32];
#pragma unroll
        for (int u = 0; u < KB / 32; ++u) {
            float e[8];
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const f32x4_t &sv = s[2 * u + (h >> 1)];
                const f32x2_t d = (f32x2_t){sv[2 * (h & 1)], sv[2 * (h & 1) + 1]} * sc2 + nm2;
                e[2 * h] = __builtin_amdgcn_exp2f(d[0]);
                e[2 * h + 1] = __builtin_amdgcn_exp2f(d[1]);
            }
            union { uint32_t w[4]; bf16x8_t v; } pk;
#pragma unroll
            for (int r = 0; r < 4; ++r) pk.w[r] = lp_pack2(e[2 * r], e[2 * r + 1]);
            pb[u] = pk.v;
        }
        // O^T[dh][query] += V^T[dh][key] . P^T[key][query]; the ones operand adds the same rounded P to l in the same order
        const bf16x8_t ones = LP_ONES;
#pragma unroll
        for (int u = 0; u < KB / 32; ++u) {
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                const bf16x8_t vf = *(const bf16x8_t *)(vt + (ct * 16 + fr) * VSTRIDE + (32 * u + 8 * g) * 2);
                o[ct] = lp_mfma16(vf, pb[u], o[ct]);
            }
            osum = lp_mfma16(ones, pb[u], osum);
            if (u & 1) __builtin_amdgcn_sched_barrier(0);
        }
    };

    {
        uint4 st[4];
        load_kv(0, st);
        store_kv(st);
    }
    __syncthreads();
    for (int b = 0; b < nb; ++b) {
        const bool more = b + 1 < nb;   // workgroup-uniform
        uint4 nxt[4];
        if (more) load_kv((b + 1) * KB, nxt);          // issued early: in flight under this block's MFMAs
        if (active) compute(b * KB, !more);
        if (!more) break;
        __syncthreads();                               // every wave is done with this block's K / V
        store_kv(nxt);                                 // written late
        __syncthreads();
    }
    if (!active) return;

    // write-out through 2 KiB of wave-private LDS as whole 128-byte rows (attention.hip)
    const float inv = __builtin_amdgcn_rcpf(osum[0]);
    char *reg = ost + wave * 2048;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        uint2 pk;
        pk.x = lp_pack2(o[ct][0] * inv, o[ct][1] * inv);
        pk.y = lp_pack2(o[ct][2] * inv, o[ct][3] * inv);
        const int chunk = 2 * ct + (g >> 1);
        *(uint2 *)(reg + fr * 128 + ((chunk ^ (fr & 7)) << 4) + ((g ^ (fr >> 3)) & 1) * 8) = pk;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int c = lane & 7;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int row = it * 8 + (lane >> 3);
        uint4 d = *(const uint4 *)(reg + row * 128 + ((c ^ (row & 7)) << 4));
        if (it & 1) d = make_uint4(d.z, d.w, d.x, d.y);
        const int q = q0 + row;
        if (q < tokens) *(uint4 *)(out + ((int64_t)frame * tokens + q) * width + head * DH + c * 8) = d;
    }
}

}  // namespace

int launch_attention_stream_bf16(const uint16_t *qkv, uint16_t *out, int frames, int tokens, int heads, hipStream_t stream) {
    VSC_REQUIRE(qkv && out, "attention_stream: null operand");
    VSC_REQUIRE(tokens >= 1 && tokens <= VSC_ATTENTION_STREAM_MAX_TOKENS, "attention_stream: %d tokens outside 1..%d", tokens,
                VSC_ATTENTION_STREAM_MAX_TOKENS);
    VSC_REQUIRE(frames >= 1 && heads >= 1, "attention_stream: %d frames, %d heads (each >= 1)", frames, heads);
    const int qblocks = (tokens + QB - 1) / QB;
    VSC_REQUIRE((int64_t)frames * heads * qblocks < (1ll << 31), "attention_stream: grid too large (%d frames x %d heads x %d query blocks)",
                frames, heads, qblocks);
    VSC_TRY(vsc_allow_dynamic_lds(attention_stream_kernel, LDS_BYTES));
    hipLaunchKernelGGL(attention_stream_kernel, dim3(frames * heads * qblocks), dim3(512), LDS_BYTES, stream, qkv, out, tokens, heads,
                       qblocks);
    VSC_CHECK_LAUNCH();
    return VSC_OK;
}
