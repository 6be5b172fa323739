// Query view preprocessing (src/image_preprocess.py): the per-pixel variance map over all frames of a video, the per-pixel Canny
// edge count over sampled frames, and the PIL-exact crop + bicubic resize of every view.  Contracts: vsc_frame_var_u8,
// vsc_canny_count_u8 and vsc_resize_bicubic_u8 in include/vsc_hip.h.  Nothing here depends on the encoders' operand type: one
// object serves both builds of the library (Makefile: BF16_ONLY).  All kernels are memory-bound integer / fp64 code.
//
// fp64 results must equal numpy's and Pillow's bit for bit: no contraction into FMAs anywhere in this file (device or host).
#pragma clang fp contract(off)

#include <math.h>

#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "common.h"
#include "resample_coeffs.h"

namespace {

constexpr int BLOCK = 256;

inline unsigned blocks_for(int64_t items) { return (unsigned)((items + BLOCK - 1) / BLOCK); }

// ---- (a) variance map ---------------------------------------------------------------------------------------------------
// One thread per pixel, two passes over the frames (mean, then squared deviations), numpy's order: per channel the frame-order
// sum (exact in uint32) / n, then sum over frames in frame order of (x - mean)^2 in fp64, / n; channels (v0 + v1) + v2.
__global__ __launch_bounds__(BLOCK) void frame_var_kernel(const uint8_t *__restrict__ frames, int64_t n, int64_t hw,
                                                          double *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= hw) return;
    const uint8_t *src = frames + p * 3;
    const int64_t stride = hw * 3;
    uint32_t s0 = 0, s1 = 0, s2 = 0;
    for (int64_t i = 0; i < n; ++i) {
        const uint8_t *q = src + i * stride;
        s0 += q[0];
        s1 += q[1];
        s2 += q[2];
    }
    const double dn = (double)n;
    const double m0 = (double)s0 / dn, m1 = (double)s1 / dn, m2 = (double)s2 / dn;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        const uint8_t *q = src + i * stride;
        const double d0 = (double)q[0] - m0, d1 = (double)q[1] - m1, d2 = (double)q[2] - m2;
        a0 = a0 + d0 * d0;
        a1 = a1 + d1 * d1;
        a2 = a2 + d2 * d2;
    }
    out[p] = (a0 / dn + a1 / dn) + a2 / dn;
}

// ---- (b) Canny edge counts ----------------------------------------------------------------------------------------------
// Per chunk of sampled frames, five launches: gradient -> NMS + thresholds -> union (8-connected components of weak | strong)
// -> compress + mark components holding a strong pixel -> count.  Labels are pixel indices inside the chunk; a component's root
// is whichever index the unions leave, which may differ from run to run -- the edge set does not.
constexpr int CANNY_CHUNK_FRAMES = 32;
constexpr int64_t CANNY_CHUNK_PIXELS = int64_t(1) << 25;   // scratch: 8 bytes per pixel of a chunk
constexpr int TG22 = 13573;                                  // tan(22.5 deg), Q15

struct FrameList {
    int64_t off[CANNY_CHUNK_FRAMES];   // byte offset of each frame of the chunk
};

enum : uint16_t { DIR_H = 0, DIR_V = 1, DIR_DIAG_POS = 2, DIR_DIAG_NEG = 3 };

// Sobel 3x3 (replicated border) of every channel, the channel with the largest |dx| + |dy| (ties: lower channel), packed as
// magnitude (bits 0-11, <= 2040) | NMS direction (bits 12-13).
__global__ __launch_bounds__(BLOCK) void canny_grad_kernel(const uint8_t *__restrict__ frames, FrameList fl, int64_t total, int h,
                                                           int w, uint16_t *__restrict__ grad) {
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= total) return;
    const int64_t hw = (int64_t)h * w;
    const int f = (int)(p / hw);
    const int q = (int)(p - f * hw);
    const int y = q / w, x = q - y * w;
    const uint8_t *img = frames + fl.off[f];
    const int ym = y > 0 ? y - 1 : 0, yp = y < h - 1 ? y + 1 : h - 1;
    const int xm = x > 0 ? x - 1 : 0, xp = x < w - 1 ? x + 1 : w - 1;
    const uint8_t *r0 = img + (int64_t)ym * w * 3, *r1 = img + (int64_t)y * w * 3, *r2 = img + (int64_t)yp * w * 3;
    int best_m = -1, best_dx = 0, best_dy = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int a = r0[xm * 3 + c], b = r0[x * 3 + c], cc = r0[xp * 3 + c];
        const int d = r1[xm * 3 + c], e = r1[xp * 3 + c];
        const int g = r2[xm * 3 + c], hh = r2[x * 3 + c], ii = r2[xp * 3 + c];
        const int dx = (cc + 2 * e + ii) - (a + 2 * d + g);
        const int dy = (g + 2 * hh + ii) - (a + 2 * b + cc);
        const int m = abs(dx) + abs(dy);
        if (m > best_m) {
            best_m = m;
            best_dx = dx;
            best_dy = dy;
        }
    }
    const int ax = abs(best_dx), ay = abs(best_dy) << 15;
    const int tg22x = ax * TG22, tg67x = tg22x + (ax << 16);
    uint16_t dir;
    if (ay < tg22x) dir = DIR_H;
    else if (ay > tg67x) dir = DIR_V;
    else dir = (best_dx ^ best_dy) < 0 ? DIR_DIAG_NEG : DIR_DIAG_POS;
    grad[p] = (uint16_t)(best_m | (dir << 12));
}

__device__ inline int mag_at(const uint16_t *grad, int64_t base, int y, int x, int h, int w) {
    if (y < 0 || y >= h || x < 0 || x >= w) return 0;   // outside the image: magnitude 0
    return grad[base + (int64_t)y * w + x] & 0xfff;
}

// Threshold + non-maximum suppression -> label = own index for weak / strong pixels, -1 otherwise; strong flag; has = 0.
__global__ __launch_bounds__(BLOCK) void canny_nms_kernel(const uint16_t *__restrict__ grad, int64_t total, int h, int w, int low,
                                                          int high, int32_t *__restrict__ label, uint8_t *__restrict__ strong,
                                                          uint8_t *__restrict__ has) {
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= total) return;
    const int64_t hw = (int64_t)h * w;
    const int64_t f = p / hw;
    const int q = (int)(p - f * hw);
    const int y = q / w, x = q - y * w;
    const int64_t base = f * hw;
    const uint16_t g = grad[p];
    const int m = g & 0xfff, dir = g >> 12;
    bool keep = false;
    if (m > low) {
        if (dir == DIR_H) keep = m > mag_at(grad, base, y, x - 1, h, w) && m >= mag_at(grad, base, y, x + 1, h, w);
        else if (dir == DIR_V) keep = m > mag_at(grad, base, y - 1, x, h, w) && m >= mag_at(grad, base, y + 1, x, h, w);
        else {
            const int s = dir == DIR_DIAG_NEG ? -1 : 1;
            keep = m > mag_at(grad, base, y - 1, x - s, h, w) && m > mag_at(grad, base, y + 1, x + s, h, w);
        }
    }
    label[p] = keep ? (int32_t)p : -1;
    strong[p] = keep && m > high;
    has[p] = 0;
}

__device__ inline int32_t find_root(int32_t *label, int32_t x) {
    int32_t y = __hip_atomic_load(label + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (y != x) {
        x = y;
        y = __hip_atomic_load(label + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return x;
}

// Lock-free union: link the larger root under the smaller index with atomicMin.  Every retry strictly lowers a or b, so the loop
// ends; a stale read only costs a retry (labels only ever decrease and always point inside the component).
__device__ inline void unite(int32_t *label, int32_t a, int32_t b) {
    for (;;) {
        a = find_root(label, a);
        b = find_root(label, b);
        if (a == b) return;
        if (a < b) {
            const int32_t old = atomicMin(label + b, a);
            if (old == b) return;
            b = old;
        } else {
            const int32_t old = atomicMin(label + a, b);
            if (old == a) return;
            a = old;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void canny_union_kernel(int32_t *label, int64_t total, int h, int w) {
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= total || label[p] < 0) return;       // foreground-ness does not change during the unions
    const int64_t hw = (int64_t)h * w;
    const int q = (int)(p % hw);
    const int y = q / w, x = q - y * w;
    const int32_t self = (int32_t)p;
    if (x > 0 && label[p - 1] >= 0) unite(label, self, self - 1);
    if (y > 0) {
        const int32_t up = self - w;
        if (x > 0 && label[up - 1] >= 0) unite(label, self, up - 1);
        if (label[up] >= 0) unite(label, self, up);
        if (x < w - 1 && label[up + 1] >= 0) unite(label, self, up + 1);
    }
}

__global__ __launch_bounds__(BLOCK) void canny_compress_kernel(int32_t *label, const uint8_t *__restrict__ strong, int64_t total,
                                                               uint8_t *has) {
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= total || label[p] < 0) return;
    const int32_t r = find_root(label, (int32_t)p);
    label[p] = r;
    if (strong[p]) has[r] = 1;
}

__global__ __launch_bounds__(BLOCK) void canny_count_kernel(const int32_t *__restrict__ label, const uint8_t *__restrict__ has,
                                                            int frames, int64_t hw, int accumulate, uint16_t *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= hw) return;
    int c = accumulate ? out[p] : 0;
    for (int f = 0; f < frames; ++f) {
        const int32_t r = label[f * hw + p];
        c += r >= 0 && has[r];
    }
    out[p] = (uint16_t)c;
}

// ---- (c) crop + bicubic resize, Pillow's 8-bit resample ----------------------------------------------------------------
constexpr int PRECISION_BITS = RESAMPLE_PRECISION_BITS;

using Coeffs = ResampleCoeffs;

// the process-wide table cache of resample_coeffs.h
std::map<std::tuple<int, int, int>, Coeffs> g_coeffs;
std::mutex g_coeffs_mutex;

inline int coeffs_get(int in, int out, Coeffs *res) { return resample_coeffs_get("resize_bicubic", in, out, res); }

__device__ inline uint8_t clip8(int v) {
    v >>= PRECISION_BITS;
    return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// The two passes read a strided source -- pixel (i, y, x) at src + i * frame_stride + y * pitch + x * 3, bytes -- and write a
// packed destination, so either can read the crop inside the frames or the other pass's packed result.
// Horizontal pass: rows [0, rows) of every frame, width -> S along x (coef) -> dst [n, rows, S, 3]
__global__ __launch_bounds__(BLOCK) void resize_h_kernel(const uint8_t *__restrict__ src, int64_t frame_stride, int64_t pitch, int64_t n,
                                                         int rows, int s, const int32_t *__restrict__ coef, int ksize,
                                                         uint8_t *__restrict__ dst) {
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n * rows * s) return;
    const int xx = (int)(p % s);
    const int64_t row = p / s;                 // i * rows + y
    const int64_t i = row / rows;
    const int y = (int)(row - i * rows);
    const int32_t *k = coef + (int64_t)xx * (2 + ksize);
    const int xmin = k[0], cnt = k[1];
    const uint8_t *q = src + i * frame_stride + y * pitch + (int64_t)xmin * 3;
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int t = 0; t < cnt; ++t) {
        const int wt = k[2 + t];
        s0 += q[t * 3 + 0] * wt;
        s1 += q[t * 3 + 1] * wt;
        s2 += q[t * 3 + 2] * wt;
    }
    uint8_t *o = dst + p * 3;
    o[0] = clip8(s0);
    o[1] = clip8(s1);
    o[2] = clip8(s2);
}

// Vertical pass: columns [0, cols) of every frame, height -> S along y (coef) -> dst [n, S, cols, 3]
__global__ __launch_bounds__(BLOCK) void resize_v_kernel(const uint8_t *__restrict__ src, int64_t frame_stride, int64_t pitch, int64_t n,
                                                         int cols, int s, const int32_t *__restrict__ coef, int ksize,
                                                         uint8_t *__restrict__ dst) {
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n * s * cols) return;
    const int xx = (int)(p % cols);
    const int64_t r = p / cols;                // i * S + yy
    const int64_t i = r / s;
    const int yy = (int)(r - i * s);
    const int32_t *k = coef + (int64_t)yy * (2 + ksize);
    const int ymin = k[0], cnt = k[1];
    const uint8_t *q = src + i * frame_stride + ymin * pitch + (int64_t)xx * 3;
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int t = 0; t < cnt; ++t) {
        const int wt = k[2 + t];
        s0 += q[t * pitch + 0] * wt;
        s1 += q[t * pitch + 1] * wt;
        s2 += q[t * pitch + 2] * wt;
    }
    uint8_t *o = dst + p * 3;
    o[0] = clip8(s0);
    o[1] = clip8(s1);
    o[2] = clip8(s2);
}

// Pillow 12's Image.resize runs the vertical pass first when the image is more than 100 times taller than wide and shrinks in
// height (a resize to (w, S), then to (S, S)); otherwise ImagingResample's order, horizontal first.
inline bool vertical_first(int hc, int wc, int s) { return hc > (int64_t)wc * 100 && s < hc; }

}  // namespace

int resample_coeffs_get(const char *who, int in, int out, ResampleCoeffs *res) {
    int dev = 0;
    VSC_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_coeffs_mutex);
    auto key = std::make_tuple(dev, in, out);
    auto it = g_coeffs.find(key);
    if (it != g_coeffs.end()) {
        *res = it->second;
        return VSC_OK;
    }
    Coeffs c;
    auto *table = new std::vector<int32_t>(resample_coeffs(in, out, &c.ksize));     // kept: ResampleCoeffs::host
    const size_t bytes = table->size() * sizeof(int32_t);
    hipError_t e = hipMalloc((void **)&c.dev, bytes);
    if (e != hipSuccess) {
        delete table;
        vsc_set_error("%s: hipMalloc(%zu) failed: %s", who, bytes, hipGetErrorString(e));
        return VSC_ERR_NOMEM;
    }
    e = hipMemcpy(c.dev, table->data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(c.dev);
        delete table;
        vsc_set_error("%s: coefficient upload failed: %s", who, hipGetErrorString(e));
        return VSC_ERR_HIP;
    }
    c.host = table->data();
    g_coeffs[key] = c;
    *res = c;
    return VSC_OK;
}

int launch_frame_var_u8(const uint8_t *frames_dev, int64_t n, int h, int w, double *out_dev, hipStream_t stream) {
    VSC_REQUIRE(n >= 1 && n < (int64_t(1) << 24), "frame_var: %lld frames (1 .. 2^24 - 1)", (long long)n);
    VSC_REQUIRE(h >= 1 && w >= 1 && (int64_t)h * w <= (int64_t(1) << 28), "frame_var: %d x %d frames unsupported", h, w);
    VSC_REQUIRE(frames_dev && out_dev, "frame_var: null pointer");
    const int64_t hw = (int64_t)h * w;
    hipLaunchKernelGGL(frame_var_kernel, dim3(blocks_for(hw)), dim3(BLOCK), 0, stream, frames_dev, n, hw, out_dev);
    VSC_CHECK_LAUNCH();
    return VSC_OK;
}

int launch_canny_count_u8(const uint8_t *frames_dev, int64_t n, const int32_t *idx_host, int m, int h, int w, double low, double high,
                          uint16_t *out_dev, hipStream_t st) {
    VSC_REQUIRE(h >= 1 && w >= 1 && (int64_t)h * w <= CANNY_CHUNK_PIXELS, "canny_count: %d x %d frames unsupported", h, w);
    VSC_REQUIRE(m >= 0 && m <= 65535, "canny_count: %d frames (0 .. 65535)", m);
    VSC_REQUIRE(out_dev && (m == 0 || (frames_dev && idx_host)), "canny_count: null pointer");
    VSC_REQUIRE(low >= 0.0 && high >= low && high < 4096.0, "canny_count: thresholds %g / %g unsupported", low, high);
    for (int j = 0; j < m; ++j)
        VSC_REQUIRE(idx_host[j] >= 0 && idx_host[j] < n, "canny_count: frame index %d outside [0, %lld)", idx_host[j], (long long)n);
    const int64_t hw = (int64_t)h * w;
    if (m == 0) {
        VSC_CHECK_HIP(hipMemsetAsync(out_dev, 0, hw * sizeof(uint16_t), st));
        return VSC_OK;
    }
    const int lo = (int)floor(low), hi = (int)floor(high);
    int chunk = (int)(CANNY_CHUNK_PIXELS / hw);
    if (chunk > CANNY_CHUNK_FRAMES) chunk = CANNY_CHUNK_FRAMES;
    if (chunk > m) chunk = m;
    const int64_t px = hw * chunk;
    void *buf = nullptr;
    int rc = search_scratch_get(SCRATCH_VIEW_CANNY, (size_t)px * 8, &buf);
    if (rc != VSC_OK) return rc;
    int32_t *label = (int32_t *)buf;
    uint16_t *grad = (uint16_t *)((uint8_t *)buf + px * 4);
    uint8_t *strong = (uint8_t *)buf + px * 6;
    uint8_t *has = (uint8_t *)buf + px * 7;
    for (int j0 = 0; j0 < m; j0 += chunk) {
        const int cnt = m - j0 < chunk ? m - j0 : chunk;
        FrameList fl;
        for (int f = 0; f < CANNY_CHUNK_FRAMES; ++f) fl.off[f] = f < cnt ? (int64_t)idx_host[j0 + f] * hw * 3 : 0;
        const int64_t total = hw * cnt;
        const dim3 grid(blocks_for(total));
        hipLaunchKernelGGL(canny_grad_kernel, grid, dim3(BLOCK), 0, st, frames_dev, fl, total, h, w, grad);
        VSC_CHECK_LAUNCH();
        hipLaunchKernelGGL(canny_nms_kernel, grid, dim3(BLOCK), 0, st, grad, total, h, w, lo, hi, label, strong, has);
        VSC_CHECK_LAUNCH();
        hipLaunchKernelGGL(canny_union_kernel, grid, dim3(BLOCK), 0, st, label, total, h, w);
        VSC_CHECK_LAUNCH();
        hipLaunchKernelGGL(canny_compress_kernel, grid, dim3(BLOCK), 0, st, label, strong, total, has);
        VSC_CHECK_LAUNCH();
        hipLaunchKernelGGL(canny_count_kernel, dim3(blocks_for(hw)), dim3(BLOCK), 0, st, label, has, cnt, hw, j0 > 0 ? 1 : 0, out_dev);
        VSC_CHECK_LAUNCH();
    }
    return VSC_OK;
}

int launch_resize_bicubic_u8(const uint8_t *frames_dev, int64_t n, int h, int w, const int32_t *boxes_host, int k, int size,
                             uint8_t *out_dev, hipStream_t st) {
    VSC_REQUIRE(n >= 0 && h >= 1 && w >= 1 && k >= 0, "resize_bicubic: bad shape n=%lld %d x %d, %d boxes", (long long)n, h, w, k);
    VSC_REQUIRE(size >= 1 && size <= 4096, "resize_bicubic: output size %d (1 .. 4096)", size);
    VSC_REQUIRE(k == 0 || boxes_host, "resize_bicubic: null boxes");
    for (int b = 0; b < k; ++b) {
        const int32_t *bx = boxes_host + 4 * b;
        VSC_REQUIRE(0 <= bx[0] && bx[0] < bx[1] && bx[1] <= h && 0 <= bx[2] && bx[2] < bx[3] && bx[3] <= w,
                    "resize_bicubic: box %d (%d, %d, %d, %d) outside the %d x %d frame", b, bx[0], bx[1], bx[2], bx[3], h, w);
    }
    if (n == 0 || k == 0) return VSC_OK;
    VSC_REQUIRE(frames_dev && out_dev, "resize_bicubic: null pointer");
    int64_t tmp_px = 0;     // the first pass's result per frame: hc x S (horizontal first) or S x wc (vertical first)
    for (int b = 0; b < k; ++b) {
        const int hc = boxes_host[4 * b + 1] - boxes_host[4 * b], wc = boxes_host[4 * b + 3] - boxes_host[4 * b + 2];
        const int64_t px = vertical_first(hc, wc, size) ? (int64_t)size * wc : (int64_t)hc * size;
        if (px > tmp_px) tmp_px = px;
    }
    // one thread per output pixel of a pass: the grids stay below 2^31 work-items
    VSC_REQUIRE(n * tmp_px < (int64_t(1) << 31) && n * size * size < (int64_t(1) << 31),
                "resize_bicubic: %lld frames with %lld-pixel passes into %d x %d: split the call", (long long)n, (long long)tmp_px, size,
                size);
    void *tmp = nullptr;
    int rc = search_scratch_get(SCRATCH_VIEW_RESIZE, (size_t)(n * tmp_px * 3), &tmp);
    if (rc != VSC_OK) return rc;
    uint8_t *t = (uint8_t *)tmp;
    const int64_t view_bytes = n * (int64_t)size * size * 3, frame_bytes = (int64_t)h * w * 3, pitch = (int64_t)w * 3;
    for (int b = 0; b < k; ++b) {
        const int y0 = boxes_host[4 * b], hc = boxes_host[4 * b + 1] - y0, x0 = boxes_host[4 * b + 2], wc = boxes_host[4 * b + 3] - x0;
        const uint8_t *crop = frames_dev + ((int64_t)y0 * w + x0) * 3;
        uint8_t *out = out_dev + b * view_bytes;
        Coeffs ch, cv;
        if ((rc = coeffs_get(wc, size, &ch)) != VSC_OK) return rc;
        if ((rc = coeffs_get(hc, size, &cv)) != VSC_OK) return rc;
        if (vertical_first(hc, wc, size)) {
            hipLaunchKernelGGL(resize_v_kernel, dim3(blocks_for(n * size * wc)), dim3(BLOCK), 0, st, crop, frame_bytes, pitch, n, wc, size,
                               cv.dev, cv.ksize, t);
            VSC_CHECK_LAUNCH();
            hipLaunchKernelGGL(resize_h_kernel, dim3(blocks_for(n * size * size)), dim3(BLOCK), 0, st, (const uint8_t *)t,
                               (int64_t)size * wc * 3, (int64_t)wc * 3, n, size, size, ch.dev, ch.ksize, out);
        } else {
            hipLaunchKernelGGL(resize_h_kernel, dim3(blocks_for(n * hc * size)), dim3(BLOCK), 0, st, crop, frame_bytes, pitch, n, hc, size,
                               ch.dev, ch.ksize, t);
            VSC_CHECK_LAUNCH();
            hipLaunchKernelGGL(resize_v_kernel, dim3(blocks_for(n * size * size)), dim3(BLOCK), 0, st, (const uint8_t *)t,
                               (int64_t)hc * size * 3, (int64_t)size * 3, n, size, size, cv.dev, cv.ksize, out);
        }
        VSC_CHECK_LAUNCH();
    }
    return VSC_OK;
}
