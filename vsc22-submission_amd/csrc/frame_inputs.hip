// Model inputs of a video from its uploaded frames: every (box, Pillow BICUBIC resize, window) target of vsc_frame_inputs_u8 in
// one call.  The contract is stated with that entry in include/vsc_hip.h (executable form: tests/frame_inputs_contract.py).
//
// frame_inputs_kernel, one workgroup per (frame, band of output rows, tile of FI_TILE output columns), one launch per target, one
// argument structure and a 1-D grid (which is also what lets the file run on the CPU against tests/hip_emu/common.h):
//  (0) the tile's rows of the horizontal coefficient table and the band's rows of the vertical one are copied to LDS: every tap
//      weight is read 40 to 400 times by the workgroup, and lanes that fetch them from global memory touch a cache line each.
//  (1) horizontal pass over the source rows the band's output rows read, the tile's columns only.  Rows come in chunks: the chunk's
//      source bytes are staged into LDS with aligned dword loads (neighbouring outputs share most of their taps), then one thread
//      per (row, output column) sums its taps from LDS in Pillow's 22-bit fixed point and writes the rounded, clipped uint8 pixel
//      to the band's intermediate rows, which live in LDS only.
//  (2) vertical pass from those rows.  A thread owns one ALIGNED dword of global memory inside an output row's segment of the
//      tile: where the segment starts dword-aligned (always when crop_w * 3 is a multiple of 4 and the tensor is dword-aligned:
//      tiles start at multiples of 4 pixels) it reads one LDS dword per tap and stores one dword; at an odd segment start it
//      computes its four bytes one by one and still stores them packed; only the partial dwords at the two ends of a segment are
//      byte stores, each byte by its owner, so neighbouring tiles and rows never write the same byte.
// The band height is the largest whose intermediate rows ((band span + vertical support) rows of the tile's bytes) fit FI_LDS_SOFT
// beside the two tables and up to FI_LDS_STAGE of staged rows, so that three workgroups share a CU; a target whose single output
// row needs more stages one row at a time and grows up to the whole VSC_FRAME_INPUTS_LDS_BYTES.  What does not fit even then, and
// Pillow's vertical-first shape, take frame_inputs_pass_kernel twice over the scratch slot SCRATCH_VIEW_RESIZE: one thread per
// output pixel of a pass, windowed and rectangular, frames in chunks so that no grid or buffer grows with n.
//
// Integer arithmetic throughout: the coefficient tables (resample_coeffs.h) hold the only floating-point results.
#pragma clang fp contract(off)

#include "common.h"
#include "resample_coeffs.h"

namespace {

constexpr int FI_BLOCK = 256;
constexpr int FI_TILE = 64;                            // output columns per workgroup; a multiple of 4: tile offsets keep the row's dword phase
constexpr int FI_LDS_MAX = VSC_FRAME_INPUTS_LDS_BYTES;
constexpr int FI_LDS_SOFT = FI_LDS_MAX < 52 * 1024 ? FI_LDS_MAX : 52 * 1024;   // three workgroups per CU
constexpr int FI_LDS_STAGE = 16 * 1024;               // of which the staged source rows take up to this much
constexpr int FI_MAX_BAND = 64;                        // output rows per workgroup at most
constexpr int FI_MAX_STAGE_ROWS = 16;                  // source rows per staging chunk at most
constexpr long long FI_PASS_CHUNK_BYTES = 256ll << 20; // two-pass path: scratch per chunk of frames
constexpr int FI_MAX_SIDE = VSC_FRAME_INPUTS_MAX_SIDE;
static_assert(FI_LDS_MAX <= 160 * 1024 && FI_TILE % 4 == 0, "include/vsc_hip.h states a budget the device does not have");

struct FiArgs {
    const uint8_t *src, *src_end;             // all frames of the call: the staging loads stay inside [src, src_end)
    uint8_t *dst;                             // [n, crop_h, crop_w, 3]
    const int32_t *ch, *cv;                   // tables [out_w][2 + kh], [out_h][2 + kv]
    long long frame_bytes, frame0;            // h * w * 3; first frame of the launch
    int pitch, kh, kv;                        // w * 3
    int y0, x0;                               // the box's corner
    int top, left, crop_h, crop_w;            // the window
    int bh, bands, tiles;                     // output rows per band, bands per frame, column tiles per band
    int mid_pitch, stage_off, stage_pitch, stage_rows, hk_off, vk_off;
};

struct FiPassArgs {
    const uint8_t *src;                       // pixel (i, y, x) at src + i * frame_bytes + y * pitch + x * 3
    uint8_t *dst;                             // packed [frames, rows, cols, 3]
    const int32_t *coef;
    long long frame_bytes, pitch, items;      // items = frames * rows * cols
    int rows, cols, ksize;
    int first, origin;                        // table row of output 0 along the resampled axis; source index of tap 0 of the buffer
    int vertical;
};

__device__ inline uint8_t fi_clip8(int v) {
    v >>= RESAMPLE_PRECISION_BITS;
    return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// the aligned dword at p, of which only the bytes inside [lo, hi) exist
__device__ inline uint32_t fi_load_dword(const uint8_t *p, const uint8_t *lo, const uint8_t *hi) {
    if (p >= lo && p + 4 <= hi) return *(const uint32_t *)p;
    uint32_t v = 0;
    for (int e = 0; e < 4; ++e)
        if (p + e >= lo && p + e < hi) v |= (uint32_t)p[e] << (8 * e);
    return v;
}

// one byte of the vertical pass: the taps k (count, then weights) down the column that starts at m
__device__ inline uint8_t fi_vbyte(const uint8_t *m, int mid_pitch, const int32_t *k) {
    const int cnt = k[1];
    int s = 1 << (RESAMPLE_PRECISION_BITS - 1);
    for (int t = 0; t < cnt; ++t) s += m[t * mid_pitch] * k[2 + t];
    return fi_clip8(s);
}

__global__ __launch_bounds__(FI_BLOCK) void frame_inputs_kernel(FiArgs a) {
    extern __shared__ __align__(16) unsigned char fi_smem[];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x % a.tiles, band = (blockIdx.x / a.tiles) % a.bands;
    const long long frame = a.frame0 + blockIdx.x / (a.tiles * a.bands);
    const int r0 = band * a.bh, r1 = r0 + a.bh < a.crop_h ? r0 + a.bh : a.crop_h;
    const int c0 = tile * FI_TILE, cw = c0 + FI_TILE < a.crop_w ? FI_TILE : a.crop_w - c0;
    const int hstride = 2 + a.kh, vstride = 2 + a.kv;
    uint8_t *mid = fi_smem;                                   // [s1 - s0][mid_pitch]
    uint8_t *stage = fi_smem + a.stage_off;                   // [stage_rows][stage_pitch]
    int32_t *hk = (int32_t *)(fi_smem + a.hk_off);            // [cw][2 + kh]
    int32_t *vk = (int32_t *)(fi_smem + a.vk_off);            // [r1 - r0][2 + kv]

    // (0) the two tables' rows of this workgroup: contiguous in global memory
    const int32_t *gh = a.ch + (long long)(a.left + c0) * hstride, *gv = a.cv + (long long)(a.top + r0) * vstride;
    for (int i = tid; i < cw * hstride; i += FI_BLOCK) hk[i] = gh[i];
    for (int i = tid; i < (r1 - r0) * vstride; i += FI_BLOCK) vk[i] = gv[i];
    __syncthreads();
    const int32_t *vlast = vk + (r1 - r0 - 1) * vstride, *hlast = hk + (cw - 1) * hstride;
    const int s0 = vk[0], s1 = vlast[0] + vlast[1];           // box rows [s0, s1) feed the band: first taps and ends are monotone
    const int xlo = hk[0], seg_bytes = (hlast[0] + hlast[1] - xlo) * 3;   // box columns from xlo feed the tile
    const uint8_t *fsrc = a.src + frame * a.frame_bytes + (long long)a.y0 * a.pitch + (long long)(a.x0 + xlo) * 3;
    const int dwp = a.stage_pitch >> 2;

    // (1) horizontal pass, a chunk of source rows at a time
    for (int c = s0; c < s1; c += a.stage_rows) {
        const int rows = s1 - c < a.stage_rows ? s1 - c : a.stage_rows;
        for (int item = tid; item < rows * dwp; item += FI_BLOCK) {
            const int r = item / dwp, d = item - r * dwp;
            const uint8_t *g = fsrc + (long long)(c + r) * a.pitch;
            const int head = (int)((uintptr_t)g & 3);
            if (d * 4 < head + seg_bytes) *(uint32_t *)(stage + r * a.stage_pitch + d * 4) = fi_load_dword(g - head + d * 4, a.src, a.src_end);
        }
        __syncthreads();
        for (int item = tid; item < rows * cw; item += FI_BLOCK) {
            const int r = item / cw, xx = item - r * cw;
            const int32_t *k = hk + xx * hstride;
            const int cnt = k[1];
            const int head = (int)((uintptr_t)(fsrc + (long long)(c + r) * a.pitch) & 3);
            const uint8_t *q = stage + r * a.stage_pitch + head + (k[0] - xlo) * 3;
            int p0 = 1 << (RESAMPLE_PRECISION_BITS - 1), p1 = p0, p2 = p0;
            for (int t = 0; t < cnt; ++t) {
                const int wt = k[2 + t];
                p0 += q[t * 3 + 0] * wt;
                p1 += q[t * 3 + 1] * wt;
                p2 += q[t * 3 + 2] * wt;
            }
            uint8_t *o = mid + (c - s0 + r) * a.mid_pitch + xx * 3;
            o[0] = fi_clip8(p0);
            o[1] = fi_clip8(p1);
            o[2] = fi_clip8(p2);
        }
        __syncthreads();
    }

    // (2) vertical pass: thread = (output row, aligned dword of global memory inside the row's segment of this tile)
    const int rowbytes = a.crop_w * 3, segbytes = cw * 3;
    const int dwr = (segbytes + 6) >> 2;                       // dwords that cover a segment starting up to 3 bytes into one
    uint8_t *out0 = a.dst + (frame * a.crop_h + r0) * (long long)rowbytes + c0 * 3;
    for (int item = tid; item < (r1 - r0) * dwr; item += FI_BLOCK) {
        const int r = item / dwr, d = item - r * dwr;
        uint8_t *seg = out0 + (long long)r * rowbytes;
        const int off = d * 4 - (int)((uintptr_t)seg & 3);
        if (off >= segbytes) continue;
        const int32_t *k = vk + r * vstride;
        const uint8_t *m = mid + (k[0] - s0) * a.mid_pitch;
        if (off >= 0 && off + 4 <= segbytes) {
            uint32_t v;
            if (!(off & 3)) {
                const int cnt = k[1];
                int p0 = 1 << (RESAMPLE_PRECISION_BITS - 1), p1 = p0, p2 = p0, p3 = p0;
                for (int t = 0; t < cnt; ++t) {
                    const uint32_t x = *(const uint32_t *)(m + off + t * a.mid_pitch);
                    const int wt = k[2 + t];
                    p0 += (int)(x & 255u) * wt;
                    p1 += (int)((x >> 8) & 255u) * wt;
                    p2 += (int)((x >> 16) & 255u) * wt;
                    p3 += (int)(x >> 24) * wt;
                }
                v = (uint32_t)fi_clip8(p0) | (uint32_t)fi_clip8(p1) << 8 | (uint32_t)fi_clip8(p2) << 16 | (uint32_t)fi_clip8(p3) << 24;
            } else {
                v = 0;
                for (int e = 0; e < 4; ++e) v |= (uint32_t)fi_vbyte(m + off + e, a.mid_pitch, k) << (8 * e);
            }
            *(uint32_t *)(seg + off) = v;
        } else {
            for (int e = 0; e < 4; ++e)
                if (off + e >= 0 && off + e < segbytes) seg[off + e] = fi_vbyte(m + off + e, a.mid_pitch, k);
        }
    }
}

// One pass of the two-pass path: along x (vertical == 0: output column c uses table row first + c) or along y (output row r uses
// table row first + r), from a strided source into a packed destination.
__global__ __launch_bounds__(FI_BLOCK) void frame_inputs_pass_kernel(FiPassArgs a) {
    const long long p = (long long)blockIdx.x * FI_BLOCK + threadIdx.x;
    if (p >= a.items) return;
    const int c = (int)(p % a.cols);
    const long long rr = p / a.cols;
    const long long i = rr / a.rows;
    const int r = (int)(rr - i * a.rows);
    const int32_t *k = a.coef + (long long)(a.first + (a.vertical ? r : c)) * (2 + a.ksize);
    const int cnt = k[1];
    const long long step = a.vertical ? a.pitch : 3;
    const uint8_t *q = a.src + i * a.frame_bytes + (a.vertical ? (long long)(k[0] - a.origin) * a.pitch + (long long)c * 3
                                                               : (long long)r * a.pitch + (long long)(k[0] - a.origin) * 3);
    int p0 = 1 << (RESAMPLE_PRECISION_BITS - 1), p1 = p0, p2 = p0;
    for (int t = 0; t < cnt; ++t) {
        const int wt = k[2 + t];
        p0 += q[t * step + 0] * wt;
        p1 += q[t * step + 1] * wt;
        p2 += q[t * step + 2] * wt;
    }
    uint8_t *o = a.dst + p * 3;
    o[0] = fi_clip8(p0);
    o[1] = fi_clip8(p1);
    o[2] = fi_clip8(p2);
}

// Pillow 12's Image.resize: vertical pass first when the image is more than 100 times taller than wide and shrinks in height
inline bool fi_vertical_first(int hc, int wc, int out_h) { return hc > (long long)wc * 100 && out_h < hc; }

struct FiPlan {
    int y0, x0, hc, wc, out_h, out_w, top, left, crop_h, crop_w;
    ResampleCoeffs ch, cv;
    int xlo, xhi, ylo, yhi;                   // box columns / rows the window reads
    bool fused;
    int bh, mid_rows, stage_rows;             // fused
    long long tmp_frame_bytes;                // two-pass: first pass's result per frame
};

// longest run of box rows a band of bh output rows reads
inline int fi_span(const FiPlan &p, int bh) {
    const int stride = 2 + p.cv.ksize;
    int span = 0;
    for (int r0 = 0; r0 < p.crop_h; r0 += bh) {
        const int r1 = r0 + bh < p.crop_h ? r0 + bh : p.crop_h;
        const int32_t *kf = p.cv.host + (size_t)(p.top + r0) * stride, *kl = p.cv.host + (size_t)(p.top + r1 - 1) * stride;
        const int s = kl[0] + kl[1] - kf[0];
        span = s > span ? s : span;
    }
    return span;
}

inline int fi_tile_cols(const FiPlan &p) { return p.crop_w < FI_TILE ? p.crop_w : FI_TILE; }
inline int fi_mid_pitch(const FiPlan &p) { return (fi_tile_cols(p) * 3 + 3) & ~3; }
// staged bytes per source row: the widest tile's taps, up to 3 bytes of misalignment in front, whole dwords
inline int fi_stage_pitch(const FiPlan &p) {
    const int stride = 2 + p.ch.ksize;
    int px = 0;
    for (int c0 = 0; c0 < p.crop_w; c0 += FI_TILE) {
        const int c1 = (c0 + FI_TILE < p.crop_w ? c0 + FI_TILE : p.crop_w) - 1;
        const int32_t *kf = p.ch.host + (size_t)(p.left + c0) * stride, *kl = p.ch.host + (size_t)(p.left + c1) * stride;
        px = kl[0] + kl[1] - kf[0] > px ? kl[0] + kl[1] - kf[0] : px;
    }
    return (px * 3 + 3 + 3) & ~3;
}
inline long long fi_hk_bytes(const FiPlan &p) { return (long long)fi_tile_cols(p) * (2 + p.ch.ksize) * 4; }
inline long long fi_vk_bytes(const FiPlan &p, int bh) { return (long long)bh * (2 + p.cv.ksize) * 4; }

// the fused kernel's band height with `budget` bytes of LDS for the intermediate rows and the band's vertical table (0: not even
// one output row fits)
inline int fi_band(const FiPlan &p, long long budget, int *mid_rows) {
    const int cap = p.crop_h < FI_MAX_BAND ? p.crop_h : FI_MAX_BAND;
    for (int bh = cap; bh >= 1; --bh) {
        const int span = fi_span(p, bh);
        if ((long long)span * fi_mid_pitch(p) + fi_vk_bytes(p, bh) <= budget) {
            *mid_rows = span;
            return bh;
        }
    }
    return 0;
}

int fi_launch_fused(const FiPlan &p, const uint8_t *frames, int64_t n, int h, int w, uint8_t *out, hipStream_t stream) {
    FiArgs a;
    a.src = frames, a.src_end = frames + n * (long long)h * w * 3, a.dst = out;
    a.ch = p.ch.dev, a.cv = p.cv.dev, a.kh = p.ch.ksize, a.kv = p.cv.ksize;
    a.frame_bytes = (long long)h * w * 3, a.pitch = w * 3;
    a.y0 = p.y0, a.x0 = p.x0, a.top = p.top, a.left = p.left, a.crop_h = p.crop_h, a.crop_w = p.crop_w;
    a.bh = p.bh, a.bands = (p.crop_h + p.bh - 1) / p.bh, a.tiles = (p.crop_w + FI_TILE - 1) / FI_TILE;
    a.mid_pitch = fi_mid_pitch(p), a.stage_off = (p.mid_rows * a.mid_pitch + 15) & ~15;
    a.stage_pitch = fi_stage_pitch(p), a.stage_rows = p.stage_rows;
    a.hk_off = (a.stage_off + a.stage_rows * a.stage_pitch + 15) & ~15;
    a.vk_off = (int)((a.hk_off + fi_hk_bytes(p) + 15) & ~15ll);
    const int lds = a.vk_off + (int)fi_vk_bytes(p, p.bh);
    VSC_TRY(vsc_allow_dynamic_lds(frame_inputs_kernel, lds));
    const int64_t per_frame = (int64_t)a.bands * a.tiles;
    const int64_t per_launch = (int64_t(1) << 30) / per_frame;   // the grid stays below 2^31 workgroups whatever n is
    for (int64_t f0 = 0; f0 < n; f0 += per_launch) {
        const int64_t cnt = n - f0 < per_launch ? n - f0 : per_launch;
        a.frame0 = f0;
        hipLaunchKernelGGL(frame_inputs_kernel, dim3((unsigned)(cnt * per_frame)), dim3(FI_BLOCK), (size_t)lds, stream, a);
        VSC_CHECK_LAUNCH();
    }
    return VSC_OK;
}

int fi_launch_pass(const FiPassArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(frame_inputs_pass_kernel, dim3((unsigned)((a.items + FI_BLOCK - 1) / FI_BLOCK)), dim3(FI_BLOCK), 0, stream, a);
    VSC_CHECK_LAUNCH();
    return VSC_OK;
}

int fi_launch_two_pass(const FiPlan &p, const uint8_t *frames, int64_t n, int h, int w, uint8_t *out, uint8_t *tmp, hipStream_t stream) {
    const bool vfirst = fi_vertical_first(p.hc, p.wc, p.out_h);
    const long long frame_bytes = (long long)h * w * 3, pitch = (long long)w * 3;
    const int seg = p.xhi - p.xlo, nrows = p.yhi - p.ylo;
    // frames per chunk: the scratch stays below FI_PASS_CHUNK_BYTES (one frame may exceed it) and every grid below 2^31 work-items
    int64_t chunk = FI_PASS_CHUNK_BYTES / p.tmp_frame_bytes;
    const int64_t px = (int64_t)p.crop_h * p.crop_w > p.tmp_frame_bytes / 3 ? (int64_t)p.crop_h * p.crop_w : p.tmp_frame_bytes / 3;
    if (chunk > (int64_t(1) << 30) / px) chunk = (int64_t(1) << 30) / px;
    if (chunk < 1) chunk = 1;
    for (int64_t f0 = 0; f0 < n; f0 += chunk) {
        const int64_t cnt = n - f0 < chunk ? n - f0 : chunk;
        FiPassArgs a, b;
        b.dst = out + f0 * (long long)p.crop_h * p.crop_w * 3;
        b.rows = p.crop_h, b.cols = p.crop_w, b.items = cnt * p.crop_h * p.crop_w;
        a.dst = tmp, b.src = tmp;
        if (vfirst) {
            // window rows of the box's columns [xlo, xhi), then the window's columns of those
            a.src = frames + f0 * frame_bytes + (long long)p.y0 * pitch + (long long)(p.x0 + p.xlo) * 3;
            a.frame_bytes = frame_bytes, a.pitch = pitch, a.rows = p.crop_h, a.cols = seg, a.items = cnt * p.crop_h * seg;
            a.coef = p.cv.dev, a.ksize = p.cv.ksize, a.first = p.top, a.origin = 0, a.vertical = 1;
            b.frame_bytes = (long long)p.crop_h * seg * 3, b.pitch = (long long)seg * 3;
            b.coef = p.ch.dev, b.ksize = p.ch.ksize, b.first = p.left, b.origin = p.xlo, b.vertical = 0;
        } else {
            // window columns of the box's rows [ylo, yhi), then the window's rows of those
            a.src = frames + f0 * frame_bytes + (long long)(p.y0 + p.ylo) * pitch + (long long)p.x0 * 3;
            a.frame_bytes = frame_bytes, a.pitch = pitch, a.rows = nrows, a.cols = p.crop_w, a.items = cnt * nrows * p.crop_w;
            a.coef = p.ch.dev, a.ksize = p.ch.ksize, a.first = p.left, a.origin = 0, a.vertical = 0;
            b.frame_bytes = (long long)nrows * p.crop_w * 3, b.pitch = (long long)p.crop_w * 3;
            b.coef = p.cv.dev, b.ksize = p.cv.ksize, b.first = p.top, b.origin = p.ylo, b.vertical = 1;
        }
        VSC_TRY(fi_launch_pass(a, stream));
        VSC_TRY(fi_launch_pass(b, stream));
    }
    return VSC_OK;
}

}  // namespace

int launch_frame_inputs_u8(const uint8_t *frames_dev, int64_t n, int h, int w, const int32_t *targets_host, int n_targets,
                           uint8_t *const *outs_host, hipStream_t stream) {
    VSC_REQUIRE(n >= 0 && h >= 1 && w >= 1 && w <= (1 << 29) && n_targets >= 0,
                "frame_inputs: bad shape n=%lld %d x %d, %d targets", (long long)n, h, w, n_targets);
    VSC_REQUIRE(n_targets == 0 || (targets_host && outs_host), "frame_inputs: null target table");
    std::vector<FiPlan> plans((size_t)n_targets);
    for (int t = 0; t < n_targets; ++t) {
        const int32_t *g = targets_host + 10 * t;
        FiPlan &p = plans[t];
        VSC_REQUIRE(0 <= g[0] && g[0] < g[1] && g[1] <= h && 0 <= g[2] && g[2] < g[3] && g[3] <= w,
                    "frame_inputs: target %d: box (%d, %d, %d, %d) outside the %d x %d frame", t, g[0], g[1], g[2], g[3], h, w);
        VSC_REQUIRE(g[4] >= 1 && g[4] <= FI_MAX_SIDE && g[5] >= 1 && g[5] <= FI_MAX_SIDE, "frame_inputs: target %d: output %d x %d (1 .. %d a side)", t,
                    g[4], g[5], FI_MAX_SIDE);
        VSC_REQUIRE(g[6] >= 0 && g[8] >= 0 && g[6] <= g[4] - g[8] && g[7] >= 0 && g[9] >= 0 && g[7] <= g[5] - g[9],
                    "frame_inputs: target %d: window (top %d, left %d, %d x %d) outside the %d x %d output", t, g[6], g[7], g[8], g[9], g[4], g[5]);
        p.y0 = g[0], p.hc = g[1] - g[0], p.x0 = g[2], p.wc = g[3] - g[2];
        p.out_h = g[4], p.out_w = g[5], p.top = g[6], p.left = g[7], p.crop_h = g[8], p.crop_w = g[9];
        VSC_REQUIRE(p.crop_h == 0 || p.crop_w == 0 || n == 0 || outs_host[t], "frame_inputs: target %d: null output", t);
    }
    if (n == 0 || n_targets == 0) return VSC_OK;
    VSC_REQUIRE(frames_dev, "frame_inputs: null frames");

    long long scratch = 0;
    for (int t = 0; t < n_targets; ++t) {
        FiPlan &p = plans[t];
        if (p.crop_h == 0 || p.crop_w == 0) continue;
        VSC_TRY(resample_coeffs_get("frame_inputs", p.wc, p.out_w, &p.ch));
        VSC_TRY(resample_coeffs_get("frame_inputs", p.hc, p.out_h, &p.cv));
        const int32_t *hf = p.ch.host + (size_t)p.left * (2 + p.ch.ksize), *hl = p.ch.host + (size_t)(p.left + p.crop_w - 1) * (2 + p.ch.ksize);
        const int32_t *vf = p.cv.host + (size_t)p.top * (2 + p.cv.ksize), *vl = p.cv.host + (size_t)(p.top + p.crop_h - 1) * (2 + p.cv.ksize);
        p.xlo = hf[0], p.xhi = hl[0] + hl[1], p.ylo = vf[0], p.yhi = vl[0] + vl[1];
        p.fused = false;
        if (!fi_vertical_first(p.hc, p.wc, p.out_h)) {
            // 48 bytes: the three 16-byte roundings between the four LDS arrays
            const long long fixed = fi_hk_bytes(p) + 48, pitch = fi_stage_pitch(p);
            int rows = (int)(FI_LDS_STAGE / pitch);
            rows = rows > FI_MAX_STAGE_ROWS ? FI_MAX_STAGE_ROWS : rows < 1 ? 1 : rows;
            p.bh = fi_band(p, (long long)FI_LDS_SOFT - fixed - rows * pitch, &p.mid_rows);
            if (!p.bh) p.bh = fi_band(p, (long long)FI_LDS_MAX - fixed - (rows = 1) * pitch, &p.mid_rows);
            if (p.bh) {
                p.fused = true;
                p.stage_rows = rows > p.mid_rows ? p.mid_rows : rows;
            }
        }
        if (!p.fused) {
            p.tmp_frame_bytes = fi_vertical_first(p.hc, p.wc, p.out_h) ? (long long)p.crop_h * (p.xhi - p.xlo) * 3 : (long long)(p.yhi - p.ylo) * p.crop_w * 3;
            long long bytes = n * p.tmp_frame_bytes;
            if (bytes > FI_PASS_CHUNK_BYTES) bytes = p.tmp_frame_bytes > FI_PASS_CHUNK_BYTES ? p.tmp_frame_bytes : FI_PASS_CHUNK_BYTES;
            scratch = bytes > scratch ? bytes : scratch;
        }
    }
    void *tmp = nullptr;
    if (scratch) VSC_TRY(search_scratch_get(SCRATCH_VIEW_RESIZE, (size_t)scratch, &tmp));
    for (int t = 0; t < n_targets; ++t) {
        const FiPlan &p = plans[t];
        if (p.crop_h == 0 || p.crop_w == 0) continue;
        if (p.fused) VSC_TRY(fi_launch_fused(p, frames_dev, n, h, w, outs_host[t], stream));
        else VSC_TRY(fi_launch_two_pass(p, frames_dev, n, h, w, outs_host[t], (uint8_t *)tmp, stream));
    }
    return VSC_OK;
}

struct vsc_frame_inputs {
    hipStream_t stream;
};

extern "C" int vsc_frame_inputs_create(void *stream, vsc_frame_inputs **out) {
    VSC_REQUIRE(out, "frame_inputs_create: null pointer");
    *out = new vsc_frame_inputs{(hipStream_t)stream};
    return VSC_OK;
}

extern "C" void vsc_frame_inputs_destroy(vsc_frame_inputs *h) { delete h; }

extern "C" int vsc_frame_inputs_u8(vsc_frame_inputs *h, const uint8_t *frames_dev, int64_t n, int32_t fh, int32_t fw, const int32_t *targets_host,
                                   int32_t n_targets, uint8_t *const *outs_host) {
    VSC_REQUIRE(h, "frame_inputs: null handle");
    return launch_frame_inputs_u8(frames_dev, n, fh, fw, targets_host, n_targets, outs_host, h->stream);
}
