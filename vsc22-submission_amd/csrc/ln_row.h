// LayerNorm of ONE row of NV x 256 columns by one wave: the arithmetic of layernorm_light_kernel (elementwise.hip), shared with the
// LayerNorm tail of the persistent residual GEMM (gemm_bf16.hip, VSC_EPI_RESADD_LN_F32).  Both callers produce the same bits: the
// order and the rounding points of every operation are pinned here -- sequential sums, the DPP butterfly, centred squares by inline
// asm, and every fused multiply-add written as one (what the compiler's contraction made of the kernel's `a * b + c` expressions is
// spelled out, so that a second caller cannot be contracted differently): var / W + eps, x rstd + shift, and t gamma + beta.
#pragma once
#include <type_traits>

#include "common.h"

// sum over the 64 lanes without index registers: four DPP adds inside each row of 16 (as row16_sum of the GEMM write-out), then
// the four row sums by v_readlane (__shfl_xor costs an address VGPR per butterfly step, kept live for the second reduction)
__device__ __forceinline__ float wave_sum_dpp(float x) {
    auto dpp = [](float v, auto ctrl) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), decltype(ctrl)::value, 0xf, 0xf, true));
    };
    x += dpp(x, std::integral_constant<int, 0xB1>{});   // quad_perm [1,0,3,2]
    x += dpp(x, std::integral_constant<int, 0x4E>{});   // quad_perm [2,3,0,1]
    x += dpp(x, std::integral_constant<int, 0x141>{});  // row_half_mirror
    x += dpp(x, std::integral_constant<int, 0x140>{});  // row_mirror
    const int xi = __builtin_bit_cast(int, x);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 48));
    return (r0 + r1) + (r2 + r3);
}

// the row's NV x 16 bytes per lane: off = lane * 16, soff = byte offset of the row inside the descriptor (0 when the descriptor is
// the row), AUX = cache policy of the loads (0, or 16 = sc1: agent scope, never served from this CU's L1)
template <int NV, int AUX>
__device__ __forceinline__ void ln_row_load(f32x4_t (&v)[NV], __amdgpu_buffer_rsrc_t rx, uint32_t off, uint32_t soff) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rx, off, soff + i * 1024, AUX));
}

// (mean, rstd) -> rstd and shift = -mean rstd of the row held in v
template <int NV>
__device__ __forceinline__ void ln_row_stats(const f32x4_t (&v)[NV], float eps, float &rstd, float &shift) {
    constexpr int W = NV * 256;
    // (the empty asm statements below keep the reductions sequential: left alone, the compiler packs them into v_pk_add_f32 /
    //  interleaved chains whose operand copies and temporaries are a dozen registers -- the light kernel's budget is 24)
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            sum += v[i][r];
            asm volatile("" : "+v"(sum));
        }
    const float mean = wave_sum_dpp(sum) * (1.0f / W);
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float d;   // one temporary, dead after its statement: (x - mean)^2 accumulated in order
            asm volatile("v_sub_f32 %1, %2, %3\n\tv_fmac_f32 %0, %1, %1" : "+v"(sq), "=&v"(d) : "v"(v[i][r]), "v"(mean));
        }
    rstd = rsqrtf(fmaf(wave_sum_dpp(sq), 1.0f / W, eps));
    shift = -mean * rstd;
}

// y = (x rstd + shift) * gamma + beta of the row in v, rounded and stored.  HOIST = false (the 24-register kernel): gamma / beta
// are fetched through rg / rb one 256-column round at a time; HOIST = true (the GEMM tail): the lane's 4 values of round i are
// gh[i * 64] / bh[i * 64] (a copy in LDS).  ro: the output descriptor, soff_o the row's byte offset inside it.
template <bool OUT_F32, int NV, bool HOIST>
__device__ __forceinline__ void ln_row_finish(const f32x4_t (&v)[NV], __amdgpu_buffer_rsrc_t rg, __amdgpu_buffer_rsrc_t rb, const f32x4_t *gh,
                                              const f32x4_t *bh, __amdgpu_buffer_rsrc_t ro, uint32_t off, uint32_t soff_o, float eps) {
    typedef __attribute__((__vector_size__(2 * sizeof(unsigned int)))) unsigned int u32x2_t;
    float rstd, shift;
    ln_row_stats<NV>(v, eps, rstd, shift);
    // gamma / beta one round at a time, in place: their offset register is made to depend on rstd (and on the previous round)
    // by an empty asm -- independent loads are otherwise all hoisted to the top of the kernel (36-44 registers)
    uint32_t off_gb = off;
    asm volatile("" : "+v"(off_gb) : "v"(rstd));
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        f32x4_t y = v[i];
        f32x4_t g;
        if (HOIST) g = gh[i * 64];
        else g = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rg, off_gb, i * 1024, 0));
#pragma unroll
        for (int r = 0; r < 4; ++r) y[r] = fmaf(y[r], rstd, shift);
        if (!HOIST) asm volatile("" : "+v"(off_gb) : "v"(y[0]), "v"(y[1]), "v"(y[2]), "v"(y[3]));   // beta is asked for behind gamma
        f32x4_t bt;
        if (HOIST) bt = bh[i * 64];
        else bt = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rb, off_gb, i * 1024, 0));
#pragma unroll
        for (int r = 0; r < 4; ++r) y[r] = fmaf(y[r], g[r], bt[r]);   // ONE rounding: fma(x rstd + shift, gamma, beta)
        if (!HOIST) asm volatile("" : "+v"(off_gb) : "v"(y[0]), "v"(y[1]), "v"(y[2]), "v"(y[3]));
        if (OUT_F32) {
            buffer_store_b128_soff(__builtin_bit_cast(vsc_u32x4_t, y), ro, off, soff_o + i * 1024);
        } else {
            u32x2_t pk = {lp_pack2(y[0], y[1]), lp_pack2(y[2], y[3])};
            uint32_t off_o;   // lane * 8, formed per round in a register that is free by now (as a value of the whole kernel it is the 25th)
            asm volatile("v_lshrrev_b32 %0, 1, %1" : "=v"(off_o) : "v"(off_gb));
            __builtin_amdgcn_raw_buffer_store_b64(pk, ro, off_o, soff_o + i * 512, 0);
        }
        if (!HOIST) __builtin_amdgcn_sched_barrier(0);
    }
}
