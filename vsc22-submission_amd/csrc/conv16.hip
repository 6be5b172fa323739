// Convolutions of the CNN descriptor backbone (SSCD ResNet-50) on the 16-bit matrix pipe: implicit GEMM over NHWC activations in the
// build's operand type (bf16 / fp16, common.h "lp"), fp32 accumulation (v_mfma_f32_16x16x32_{bf16,f16}).
//
//   out[m, co] = act(bias[co] + sum_k A[m, k] W[co, k] (+ residual[m, co]))      m = (n, ho, wo),  k = (r, s, ci)
//
// M = n Ho Wo output pixels, N = Cout, K = R S Cin.  Cin is a multiple of 64, so a K-step of 64 lies inside ONE tap (r, s): the A tile of
// a K-step is, per output pixel, 128 contiguous bytes of one input pixel -- or zeros, when the tap lies in the padding or the row is past
// M.  Nothing is clamped: a tap outside the image is staged as zero, exactly what the padded convolution adds.
//
// Workgroup: 256 threads = 4 waves (2 along M x 2 along N), output tile 128 x 128, wave tile 64 x 64 = 4 x 4 MFMA tiles of 16 x 16
// (64 accumulator registers).  A K-step is fetched global -> registers (4 + 4 dwordx4 per thread) while the MFMAs of the step before
// run out of LDS; two LDS buffers of 2 x 16 KiB, one workgroup barrier per K-step.  LDS rows are 128 bytes (one K-step); 16-byte chunk
// c of row r sits at chunk c ^ ((r >> 1) & 7), the layout mainloop64.h reads conflict-free with ds_read_b128.
// The MFMA takes W as its first operand and A as its second: a lane then owns FOUR CONSECUTIVE output channels of one pixel, which is
// one 8-byte store into the NHWC row.
//
// Every output element is one accumulator chain over k in a fixed order that depends on (Cin, R) alone: a frame's bits do not depend
// on how many frames share the call, nor on where its rows fall in a tile.
//
// Also here: the stem's im2col rows (7 x 7 stride 2 pad 3 over 3 channels, K = 147 zero-padded to 192; uint8 frames are normalised in
// the reference's fp32 order first) -- the rows then go through the kernel above as a 1 x 1 case -- and the 3 x 3 stride-2 max-pool.
#include <math.h>

#include "conv16.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = BM * BK * 2;   // 16 KiB: one operand tile of one K-step

struct Conv16Args {
    const uint16_t *in;     // [n, h, w, cin]
    const uint16_t *wgt;    // [cout, r, s, cin]
    const float *bias;      // [cout] or null
    const uint16_t *res;    // [m, cout] or null
    uint16_t *out;          // [m, cout]
    int64_t m;              // n * ho * wo
    int h, w, cin, cout, ho, wo, ksize, stride, pad, relu;
};

__device__ __forceinline__ uint32_t lds_chunk_off(int row, int chunk) { return (uint32_t)(row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4)); }

__global__ __launch_bounds__(256) void conv16_igemm_kernel(Conv16Args p) {
    lp_kernel_entry();
    __shared__ __attribute__((aligned(16))) char lds[2][2][TILE_BYTES];   // [buffer][A / W]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int kdim = p.ksize * p.ksize * p.cin;
    const int nk = kdim / BK;

    // staging: thread t owns 16-byte chunk (t & 7) of rows (t >> 3) + 32 i, i = 0..3, of both tiles
    const int chunk = tid & 7;
    int64_t a_pix[4];     // element offset of input pixel (n, ho * stride - pad, wo * stride - pad), channel 0 (may point outside: never dereferenced then)
    int a_hi[4], a_wi[4]; // that pixel's coordinates; a_hi = INT_MIN / 2 for rows past M
    const uint16_t *w_row[4];
    bool w_ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (tid >> 3) + 32 * i;
        const int64_t m = m0 + row;
        if (m < p.m) {
            const int64_t hw = (int64_t)p.ho * p.wo;
            const int64_t n = m / hw;
            const int rem = (int)(m - n * hw);
            const int ho = rem / p.wo, wo = rem - ho * p.wo;
            a_hi[i] = ho * p.stride - p.pad;
            a_wi[i] = wo * p.stride - p.pad;
            a_pix[i] = ((n * p.h + a_hi[i]) * p.w + a_wi[i]) * p.cin;
        } else {
            a_hi[i] = -(1 << 30);
            a_wi[i] = 0;
            a_pix[i] = 0;
        }
        w_ok[i] = n0 + row < p.cout;
        w_row[i] = p.wgt + (int64_t)(w_ok[i] ? n0 + row : 0) * kdim;
    }

    bf16x8_t ra[4], rw[4];
    const bf16x8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
    auto fetch = [&](int kt) {
        const int k0 = kt * BK;
        const int tap = k0 / p.cin, ci0 = k0 - tap * p.cin;
        const int r = tap / p.ksize, s = tap - r * p.ksize;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int hi = a_hi[i] + r, wi = a_wi[i] + s;
            const bool ok = hi >= 0 && hi < p.h && wi >= 0 && wi < p.w;
            ra[i] = ok ? *(const bf16x8_t *)(p.in + a_pix[i] + ((int64_t)r * p.w + s) * p.cin + ci0 + chunk * 8) : zero;
            rw[i] = w_ok[i] ? *(const bf16x8_t *)(w_row[i] + k0 + chunk * 8) : zero;
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = (tid >> 3) + 32 * i;
            *(bf16x8_t *)(lds[buf][0] + lds_chunk_off(row, chunk)) = ra[i];
            *(bf16x8_t *)(lds[buf][1] + lds_chunk_off(row, chunk)) = rw[i];
        }
    };

    f32x4_t acc[4][4];   // [pixel tile i][channel tile j]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    fetch(0);
    stash(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) fetch(kt + 1);
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
            bf16x8_t af[4], wf[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                af[i] = *(const bf16x8_t *)(lds[buf][0] + lds_chunk_off(wm * 64 + i * 16 + (lane & 15), kh * 4 + (lane >> 4)));
                wf[i] = *(const bf16x8_t *)(lds[buf][1] + lds_chunk_off(wn * 64 + i * 16 + (lane & 15), kh * 4 + (lane >> 4)));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = lp_mfma16(wf[j], af[i], acc[i][j]);
        }
        if (kt + 1 < nk) stash(buf ^ 1);   // last read by the MFMAs of step kt - 1: the barrier that closed that step lies in between
        __syncthreads();
    }

    // write-out: lane owns pixel m0 + wm 64 + 16 i + (lane & 15), channels n0 + wn 64 + 16 j + 4 (lane >> 4) + 0..3
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t m = m0 + wm * 64 + i * 16 + (lane & 15);
        if (m >= p.m) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = n0 + wn * 64 + j * 16 + 4 * (lane >> 4);
            if (co >= p.cout) continue;   // cout is a multiple of 4: a lane's four channels exist together
            const int64_t o = m * p.cout + co;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[i][j][e] + (p.bias ? p.bias[co + e] : 0.f);
            if (p.res) {
                const bf16x4_t r = *(const bf16x4_t *)(p.res + o);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += lp_to_f32((uint16_t)r[e]);
            }
            if (p.relu) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
            }
            uint2 pk;
            pk.x = lp_pack2(v[0], v[1]);
            pk.y = lp_pack2(v[2], v[3]);
            *(uint2 *)(p.out + o) = pk;
        }
    }
}

// ---- stem rows: rows[(n, ho, wo)][k], k = (r * 7 + s) * 3 + c for k < 147, zero for 147 <= k < 192 and for taps outside the image.
// A thread writes 8 consecutive k (16 bytes).  U8: frames [n, h, w, 3] uint8, value = (v / 255 - mean[c]) / std[c] in fp32 (ToTensor,
// then Normalize).  Otherwise frames [n, 3, h, w] float32, already normalised.
constexpr int STEM_K = 147, STEM_KPAD = VSC_STEM_KPAD;
template <bool U8>
__global__ __launch_bounds__(256) void stem_rows_kernel(const void *__restrict__ frames, uint16_t *__restrict__ rows, int64_t n, int h, int w,
                                                        int ho, int wo, float m0, float m1, float m2, float s0, float s1, float s2) {
    lp_kernel_entry();
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = n * ho * wo * (STEM_KPAD / 8);
    if (idx >= total) return;
    const int64_t row = idx / (STEM_KPAD / 8);
    const int k0 = (int)(idx - row * (STEM_KPAD / 8)) * 8;
    const int64_t hw = (int64_t)ho * wo;
    const int64_t f = row / hw;
    const int rem = (int)(row - f * hw);
    const int oy = rem / wo, ox = rem - oy * wo;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = k0 + e;
        const int tap = k / 3, c = k - tap * 3;
        const int r = tap / 7, s = tap - r * 7;
        const int y = oy * 2 - 3 + r, x = ox * 2 - 3 + s;
        float val = 0.f;
        if (k < STEM_K && y >= 0 && y < h && x >= 0 && x < w) {
            if (U8) {
                const float px = (float)((const uint8_t *)frames)[((f * h + y) * w + x) * 3 + c] / 255.0f;
                const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
                val = (px - mean) / sd;
            } else {
                val = ((const float *)frames)[((f * 3 + c) * h + y) * w + x];
            }
        }
        v[e] = val;
    }
    uint4 pk;
    pk.x = lp_pack2(v[0], v[1]);
    pk.y = lp_pack2(v[2], v[3]);
    pk.z = lp_pack2(v[4], v[5]);
    pk.w = lp_pack2(v[6], v[7]);
    *(uint4 *)(rows + row * STEM_KPAD + k0) = pk;
}

// ---- max-pool 3 x 3, stride 2, pad 1 on NHWC: the maximum over the taps INSIDE the image (the centre tap always is), so padding never
// wins.  A thread owns 8 consecutive channels of one output pixel.  Values are compared as fp32 (exact for both operand types).
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(const uint16_t *__restrict__ in, uint16_t *__restrict__ out, int64_t n, int h, int w,
                                                           int c, int ho, int wo) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c8 = c / 8;
    if (idx >= n * ho * wo * c8) return;
    const int64_t pix = idx / c8;
    const int ch = (int)(idx - pix * c8) * 8;
    const int64_t hw = (int64_t)ho * wo;
    const int64_t f = pix / hw;
    const int rem = (int)(pix - f * hw);
    const int oy = rem / wo, ox = rem - oy * wo;
    float best[8];
    bf16x8_t bits = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 8; ++e) best[e] = -INFINITY;
    for (int r = 0; r < 3; ++r) {
        const int y = oy * 2 - 1 + r;
        if (y < 0 || y >= h) continue;
        for (int s = 0; s < 3; ++s) {
            const int x = ox * 2 - 1 + s;
            if (x < 0 || x >= w) continue;
            const bf16x8_t v = *(const bf16x8_t *)(in + ((f * h + y) * w + x) * c + ch);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float fv = lp_to_f32((uint16_t)v[e]);
                if (fv > best[e] || best[e] == -INFINITY) {   // (the first tap is taken as it is, whatever its value)
                    best[e] = fv;
                    bits[e] = v[e];
                }
            }
        }
    }
    *(bf16x8_t *)(out + pix * c + ch) = bits;
}

}  // namespace

// ---- launchers (declared in conv16.h) ----------------------------------------------------------------------------------------------

int conv16_out_extent(int in, int ksize, int stride) { return (in + 2 * ((ksize - 1) / 2) - ksize) / stride + 1; }

int launch_conv16(const uint16_t *in, const uint16_t *wgt, const float *bias, const uint16_t *res, uint16_t *out, int64_t n, int h, int w, int cin, int cout, int ksize, int stride, int relu, hipStream_t stream) {
    VSC_REQUIRE(in && wgt && out, "conv2d_nhwc: null operand");
    VSC_REQUIRE(n >= 1 && h >= 1 && w >= 1, "conv2d_nhwc: n %lld, h %d, w %d must be >= 1", (long long)n, h, w);
    VSC_REQUIRE(ksize == 1 || ksize == 3, "conv2d_nhwc: kernel size %d (1 or 3)", ksize);
    VSC_REQUIRE(stride == 1 || stride == 2, "conv2d_nhwc: stride %d (1 or 2)", stride);
    VSC_REQUIRE(cin >= 64 && cin % 64 == 0, "conv2d_nhwc: cin %d must be a multiple of 64", cin);
    VSC_REQUIRE(cout >= 4 && cout % 4 == 0, "conv2d_nhwc: cout %d must be a multiple of 4", cout);
    const int ho = conv16_out_extent(h, ksize, stride), wo = conv16_out_extent(w, ksize, stride);
    const int64_t m = n * ho * wo;
    VSC_REQUIRE(n * h * w < (1ll << 31) && m * cout < (1ll << 40), "conv2d_nhwc: n h w = %lld exceeds 2^31 pixels", (long long)(n * h * w));
    const int64_t gx = (m + BM - 1) / BM, gy = (cout + BN - 1) / BN;
    VSC_REQUIRE(gx < (1ll << 31) && gy < 65536, "conv2d_nhwc: grid %lld x %lld", (long long)gx, (long long)gy);
    Conv16Args p;
    p.in = in; p.wgt = wgt; p.bias = bias; p.res = res; p.out = out;
    p.m = m; p.h = h; p.w = w; p.cin = cin; p.cout = cout; p.ho = ho; p.wo = wo; p.ksize = ksize; p.stride = stride;
    p.pad = (ksize - 1) / 2; p.relu = relu;
    hipLaunchKernelGGL(conv16_igemm_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, stream, p);
    VSC_CHECK_LAUNCH();
    return VSC_OK;
}

int launch_stem_rows(const uint8_t *frames_u8, const float *frames_f32, uint16_t *rows, int64_t n, int h, int w, const float *mean,
                     const float *std, hipStream_t stream) {
    VSC_REQUIRE((frames_u8 || frames_f32) && rows, "stem_rows: null operand");
    VSC_REQUIRE(n >= 1 && h >= 1 && w >= 1, "stem_rows: n %lld, h %d, w %d must be >= 1", (long long)n, h, w);
    VSC_REQUIRE(n * h * w < (1ll << 31), "stem_rows: n h w = %lld exceeds 2^31 pixels", (long long)(n * h * w));
    VSC_REQUIRE(!frames_u8 || (mean && std), "stem_rows: uint8 frames need mean and std");
    const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
    const int64_t total = n * ho * wo * (STEM_KPAD / 8);
    const unsigned grid = (unsigned)((total + 255) / 256);
    if (frames_u8)
        hipLaunchKernelGGL(stem_rows_kernel<true>, dim3(grid), dim3(256), 0, stream, (const void *)frames_u8, rows, n, h, w, ho, wo, mean[0],
                           mean[1], mean[2], std[0], std[1], std[2]);
    else
        hipLaunchKernelGGL(stem_rows_kernel<false>, dim3(grid), dim3(256), 0, stream, (const void *)frames_f32, rows, n, h, w, ho, wo, 0.f, 0.f,
                           0.f, 1.f, 1.f, 1.f);
    VSC_CHECK_LAUNCH();
    return VSC_OK;
}

int launch_maxpool3x3s2(const uint16_t *in, uint16_t *out, int64_t n, int h, int w, int c, hipStream_t stream) {
    VSC_REQUIRE(in && out, "maxpool3x3s2: null operand");
    VSC_REQUIRE(n >= 1 && h >= 1 && w >= 1, "maxpool3x3s2: n %lld, h %d, w %d must be >= 1", (long long)n, h, w);
    VSC_REQUIRE(c >= 8 && c % 8 == 0, "maxpool3x3s2: channels %d must be a multiple of 8", c);
    VSC_REQUIRE(n * h * w < (1ll << 31), "maxpool3x3s2: n h w = %lld exceeds 2^31 pixels", (long long)(n * h * w));
    const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
    const int64_t total = n * ho * wo * (c / 8);
    hipLaunchKernelGGL(maxpool3x3s2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, in, out, n, h, w, c, ho, wo);
    VSC_CHECK_LAUNCH();
    return VSC_OK;
}

// ---- C ABI: the building blocks (include/vsc_hip.h) ---------------------------------------------------------------------------------
extern "C" int vsc_conv2d_nhwc_bf16(void *stream, const uint16_t *in_dev, const uint16_t *w_dev, const float *bias_dev, const uint16_t *residual_dev,
                                    uint16_t *out_dev, int64_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t ksize,
                                    int32_t stride, int32_t relu) {
    VSC_REQUIRE_ALIGNED("conv2d_nhwc", in_dev, 16);
    VSC_REQUIRE_ALIGNED("conv2d_nhwc", w_dev, 16);
    VSC_REQUIRE_ALIGNED("conv2d_nhwc", bias_dev, 4);
    VSC_REQUIRE_ALIGNED("conv2d_nhwc", residual_dev, 8);
    VSC_REQUIRE_ALIGNED("conv2d_nhwc", out_dev, 8);
    return launch_conv16(in_dev, w_dev, bias_dev, residual_dev, out_dev, n, h, w, cin, cout, ksize, stride, relu,
                         (hipStream_t)stream);
}

extern "C" int vsc_maxpool3x3s2_nhwc_bf16(void *stream, const uint16_t *in_dev, uint16_t *out_dev, int64_t n, int32_t h, int32_t w, int32_t c) {
    VSC_REQUIRE_ALIGNED("maxpool3x3s2", in_dev, 16);
    VSC_REQUIRE_ALIGNED("maxpool3x3s2", out_dev, 16);
    return launch_maxpool3x3s2(in_dev, out_dev, n, h, w, c, (hipStream_t)stream);
}

extern "C" int vsc_stem_rows_u8(void *stream, const uint8_t *frames_u8_dev, const float *frames_f32_dev, int64_t n, int32_t h, int32_t w, const float *mean,
                                const float *std, uint16_t *rows_dev) {
    VSC_REQUIRE(!(frames_u8_dev && frames_f32_dev), "stem_rows: give uint8 frames or float32 frames, not both");
    VSC_REQUIRE_ALIGNED("stem_rows", frames_f32_dev, 4);
    VSC_REQUIRE_ALIGNED("stem_rows", rows_dev, 16);
    return launch_stem_rows(frames_u8_dev, frames_f32_dev, rows_dev, n, h, w, mean, std, (hipStream_t)stream);
}
