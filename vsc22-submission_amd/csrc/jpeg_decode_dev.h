// What the kernels of csrc/jpeg_decode.hip (one wave per frame) and csrc/jpeg_split.hip (one wave per item of a frame) share: the
// frame table, the bit reader, the Huffman lookups, jpeg_idct_islow, the decode body of a run of blocks, the colour kernel's body,
// and on the host the checks of a call's operands, the table sets and the handle.  Included after common.h (or its stand-in under
// tests/hip_emu); every definition is internal to the translation unit that includes it.
#pragma once
#include <cstring>
#include <map>
#include <string>
#include <vector>

// a value every lane of the wave holds: kept in a scalar register
#ifndef JD_UNIFORM
#define JD_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#endif

namespace {

constexpr int JD_WAVE = 64;
constexpr int JD_COLOR_BLOCK = 256;
constexpr int JD_BAND = 16, JD_TILE = 64;              // rows and columns of the colour kernel's workgroup
constexpr int JD_LOOK = 9;                             // bits of the Huffman lookup table
constexpr int JD_HUFF_BYTES = (1 << JD_LOOK) * 2 + 18 * 4 + 18 * 4 + 256;
constexpr int JD_SET_BYTES = 512 + 4 * JD_HUFF_BYTES;  // a table set as the kernel reads it
constexpr int JD_WINDOW = 256;                         // bytes of the bitstream held in LDS
constexpr long long JD_DEFAULT_CAP = 1ll << 30;        // plane scratch per chunk of frames
static_assert(JD_SET_BYTES % 16 == 0 && JD_HUFF_BYTES % 4 == 0, "the table set is copied to LDS in dwords");

constexpr int JD_FRAME_ROW = VSC_JPEG_FRAME_ROW;
static_assert(JD_FRAME_ROW == 10 && VSC_JPEG_TABLE_SET_BYTES == 1608, "include/vsc_hip.h states another table format");

struct JdFrame {                                       // the frame table as the kernels read it
    long long seg_off, out_off, plane_off;             // plane_off: the frame's Y plane in the chunk's scratch, Cb and Cr behind it
    int seg_len, h, w, sampling, restart, set, comp;
    int wg0;                                           // colour kernel: the frame's first workgroup in its chunk's grid
};

struct JdArgs {
    const uint8_t *bytes;
    const JdFrame *frames;                             // the chunk's frames
    const uint32_t *sets;                              // [n sets][JD_SET_BYTES / 4]
    uint8_t *planes, *out;
    int32_t *status;                                   // the chunk's entries
    int n;
};

// natural (row-major) position of the k-th coefficient of a block
__host__ __device__ inline int jd_zigzag(int k) {
    constexpr unsigned char t[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return t[k];
}

// geometry of a frame: luma blocks per MCU along x and y, MCUs per row and column, plane pitches and sizes
struct JdGeom {
    int hs, vs, mx, my, ypitch, cpitch, ncomp;
    long long ybytes, cbytes;
};
__host__ __device__ inline JdGeom jd_geom(int h, int w, int sampling) {
    JdGeom g;
    g.hs = sampling >= 2 ? 2 : 1, g.vs = sampling == 3 ? 2 : 1, g.ncomp = sampling == 0 ? 1 : 3;
    g.mx = (w + 8 * g.hs - 1) / (8 * g.hs), g.my = (h + 8 * g.vs - 1) / (8 * g.vs);
    g.ypitch = g.mx * 8 * g.hs, g.cpitch = g.mx * 8;
    g.ybytes = (long long)g.ypitch * g.my * 8 * g.vs, g.cbytes = g.ncomp == 3 ? (long long)g.cpitch * g.my * 8 : 0;
    return g;
}

// the aligned dword at p, of which only the bytes inside [lo, hi) exist
__device__ inline uint32_t jd_load_dword(const uint8_t *p, const uint8_t *lo, const uint8_t *hi) {
    if (p >= lo && p + 4 <= hi) return *(const uint32_t *)p;
    uint32_t v = 0;
    for (int e = 0; e < 4; ++e)
        if (p + e >= lo && p + e < hi) v |= (uint32_t)p[e] << (8 * e);
    return v;
}

// ---- the bit reader: wave-uniform state ---------------------------------------------------------------------------------------------
template <bool RAW> struct JdBitsT {
    static constexpr bool raw = RAW;   // keeps ff: only a reader that is asked for raw positions (jd_rawpos) pays for it
    const uint8_t *seg;
    uint32_t *win;             // LDS, JD_WINDOW bytes
    int len, pos;              // bytes of the segment; next byte to take
    int wbase;                 // the window holds bytes [wbase, wbase + JD_WINDOW) of the segment; seg + wbase is dword-aligned
    unsigned long long bb;     // the low nb bits are the next bits of the stream
    int nb, avail;             // avail: how many of them are the stream's (zeros are fed behind a marker or the end)
    int stop;                  // a marker or the end of the segment has been reached
    uint32_t ff;               // bit i: a stuffed zero followed the i-th newest byte of bb (jd_rawpos)
};
using JdBits = JdBitsT<false>;
using JdRawBits = JdBitsT<true>;

template <class B> __device__ inline int jd_byte(B &b, int p) {
    if (p < b.wbase || p >= b.wbase + JD_WINDOW) {
        const int head = (int)((uintptr_t)b.seg & 3);
        b.wbase = ((p + head) & ~3) - head - 4;          // four bytes back: the byte before p stays readable
        __syncthreads();
        b.win[threadIdx.x] = jd_load_dword(b.seg + b.wbase + 4 * (int)threadIdx.x, b.seg, b.seg + b.len);
        __syncthreads();
    }
    const int o = p - b.wbase;
    return JD_UNIFORM((int)((b.win[o >> 2] >> (8 * (o & 3))) & 255u));
}

template <class B> __device__ inline void jd_fill(B &b) {
    while (b.nb <= 48) {
        int v = 0;
        uint32_t stuffed = 0;
        if (!b.stop) {
            if (b.pos >= b.len) b.stop = 1;
            else {
                v = jd_byte(b, b.pos);
                if (v != 0xFF) b.pos += 1;
                else if (b.pos + 1 < b.len && jd_byte(b, b.pos + 1) == 0) b.pos += 2, stuffed = 1;       // a stuffed zero
                else b.stop = 1, v = 0;                                                    // a marker: it stays where it is
            }
            if (!b.stop) b.avail += 8;
        }
        b.bb = b.bb << 8 | (unsigned long long)v;
        if constexpr (B::raw) b.ff = b.ff << 1 | stuffed;
        b.nb += 8;
    }
}

// the reader at bit `bit` (0 .. 7) of the segment's byte `byte`, which is taken as data whatever stands in front of it; the window stays
template <class B> __device__ inline void jd_start(B &b, int byte, int bit) {
    b.pos = byte, b.bb = 0, b.nb = 0, b.avail = 0, b.stop = 0, b.ff = 0;
    if (bit) {
        jd_fill(b);
        b.nb -= bit, b.avail -= bit;
    }
}

// raw position, in bits from the segment's start, of the next unread bit (avail >= 0): across FF 00 pairs, which count as two bytes
__device__ inline long long jd_rawpos(const JdRawBits &b) {
    const int whole = b.avail >> 3, part = b.avail & 7, pads = (b.nb - b.avail) >> 3;
    const int q = b.pos - whole - (int)__popcll((unsigned long long)((b.ff >> pads) & ((1u << whole) - 1u)));
    if (!part) return 8ll * q;
    return 8ll * (q - 1 - (int)((b.ff >> (pads + whole)) & 1u)) + 8 - part;
}

template <class B> __device__ inline int jd_peek(const B &b, int n) { return (int)(b.bb >> (b.nb - n)) & ((1 << n) - 1); }
template <class B> __device__ inline void jd_skip(B &b, int n) { b.nb -= n, b.avail -= n; }

struct JdHuff {                // one Huffman table in LDS
    const uint16_t *lut;
    const int32_t *maxcode, *valoff;
    const uint8_t *vals;
};
__device__ inline JdHuff jd_huff(const uint32_t *set, int t) {
    const uint8_t *p = (const uint8_t *)set + 512 + t * JD_HUFF_BYTES;
    JdHuff h;
    h.lut = (const uint16_t *)p, h.maxcode = (const int32_t *)(p + (2 << JD_LOOK)), h.valoff = h.maxcode + 18, h.vals = (const uint8_t *)(h.valoff + 18);
    return h;
}

// the next symbol, or -1 when no code of the table starts the next bits
template <class B> __device__ inline int jd_symbol(B &b, const JdHuff &h) {
    jd_fill(b);
    const int e = JD_UNIFORM((int)h.lut[jd_peek(b, JD_LOOK)]);
    if (e) {
        jd_skip(b, e >> 8);
        return e & 255;
    }
    const int code16 = jd_peek(b, 16);
    for (int l = JD_LOOK + 1; l <= 16; ++l) {
        const int code = code16 >> (16 - l);
        if (code <= JD_UNIFORM(h.maxcode[l])) {
            jd_skip(b, l);
            return JD_UNIFORM((int)h.vals[(JD_UNIFORM(h.valoff[l]) + code) & 255]);
        }
    }
    return -1;
}

// s more bits as a signed value (libjpeg's HUFF_EXTEND); s in 1 .. 16
template <class B> __device__ inline int jd_receive(B &b, int s) {
    jd_fill(b);
    const int x = jd_peek(b, s);
    jd_skip(b, s);
    return x >> (s - 1) ? x : x - (1 << s) + 1;
}

// ---- jpeg_idct_islow ----------------------------------------------------------------------------------------------------------------
// one pass over d[0 .. 7]; wrapping arithmetic, arithmetic shift: libjpeg's for every value an encoder's stream produces
__device__ inline void jd_idct8(uint32_t *d, int shift) {
    const uint32_t F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633, F_1_501 = 12299, F_1_847 = 15137,
                   F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;
    uint32_t z2 = d[2], z3 = d[6];
    uint32_t z1 = (z2 + z3) * F_0_541;
    uint32_t tmp2 = z1 - z3 * F_1_847, tmp3 = z1 + z2 * F_0_765;
    z2 = d[0], z3 = d[4];
    uint32_t tmp0 = (z2 + z3) << 13, tmp1 = (z2 - z3) << 13;
    const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = d[7], tmp1 = d[5], tmp2 = d[3], tmp3 = d[1];
    z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
    uint32_t z4 = tmp1 + tmp3;
    const uint32_t z5 = (z3 + z4) * F_1_175;
    tmp0 *= F_0_298, tmp1 *= F_2_053, tmp2 *= F_3_072, tmp3 *= F_1_501;
    z1 = 0u - z1 * F_0_899, z2 = 0u - z2 * F_2_562, z3 = z5 - z3 * F_1_961, z4 = z5 - z4 * F_0_390;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    const uint32_t r = 1u << (shift - 1);
    const uint32_t o[8] = {tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3};
    for (int i = 0; i < 8; ++i) d[i] = (uint32_t)((int32_t)(o[i] + r) >> shift);
}

// libjpeg's post-IDCT range-limit table read through its 10-bit mask
__device__ inline uint32_t jd_range_limit(uint32_t x) {
    const uint32_t m = x & 1023u;
    return m < 128u ? m + 128u : m < 512u ? 255u : m < 896u ? 0u : m - 896u;
}

// ---- the decode body: blocks [j0, j1) of a frame in scan order ---------------------------------------------------------------------
// Block j is slot j % bpm of MCU j / bpm (bpm blocks per MCU: the luma blocks row by row, then Cb, then Cr).  The reader stands at
// block j0's first bit and pred[] holds the DC predictors there.  Where the restart interval ends inside the run the stream must be
// byte-aligned with less than a byte of padding in front of the RSTn in sequence; with end_off >= 0 the same holds behind block
// j1 - 1, and that marker stands at byte end_off of the segment (an item that is not its frame's last: the next one starts behind
// it).  Scan + dequantisation + IDCT + plane store per block; -> 0 or the VSC_JPEG_STATUS_* that stopped the run.
__device__ inline int jd_restart_ahead(JdBits &b, int number) {
    jd_fill(b);
    return b.stop && b.avail < 8 && b.pos + 2 <= b.len && jd_byte(b, b.pos) == 0xFF && jd_byte(b, b.pos + 1) == 0xD0 + number;
}

// WHOLE: the run is the frame (j0 == 0, j1 == its block count, end_off < 0), which the compiler is told so that the one-wave kernel
// pays nothing for the general case.
template <bool WHOLE> __device__ inline int jd_decode_blocks(const JdFrame &f, const JdGeom &g, JdBits &b, const uint32_t *jd_set, uint32_t (*jd_ws)[64], uint8_t *planes, int j0, int j1,
                                       int *pred, int end_off) {
    const int lane = threadIdx.x;
    const int ylum = g.hs * g.vs, bpm = g.ncomp == 3 ? ylum + 2 : 1;
    const int mcu0 = WHOLE ? 0 : j0 / bpm, slot0 = WHOLE ? 0 : j0 - mcu0 * bpm;
    const int mcus = g.mx * g.my;
    int status = 0;
    int mrow = mcu0 / g.mx, mcol = mcu0 - mrow * g.mx;
    int left = j1 - j0;                                    // blocks still to decode
    int mcu = mcu0;
    for (; (WHOLE ? mcu < mcus : left > 0) && !status; ++mcu) {
        if (f.restart > 0 && mcu > mcu0 && mcu % f.restart == 0) {
            // byte-align: what is left of the interval must be less than one byte of padding in front of the marker
            if (!jd_restart_ahead(b, (mcu / f.restart - 1) & 7)) {
                status = VSC_JPEG_STATUS_RESTART;
                break;
            }
            jd_start(b, b.pos + 2, 0);
            pred[0] = pred[1] = pred[2] = 0;
        }
        for (int c = 0; c < g.ncomp && !status; ++c) {
            const int sel = f.comp >> (8 * c);
            const uint16_t *quant = (const uint16_t *)jd_set + (sel & 3) * 64;
            const JdHuff dc = jd_huff(jd_set, (sel >> 2) & 1), ac = jd_huff(jd_set, 2 + ((sel >> 3) & 1));
            const int bw = c == 0 ? g.hs : 1, bh = c == 0 ? g.vs : 1, pitch = c == 0 ? g.ypitch : g.cpitch;
            const int first = c == 0 ? 0 : ylum + c - 1;   // the component's first slot in the MCU
            uint8_t *plane = planes + f.plane_off + (c == 0 ? 0 : g.ybytes + (c - 1) * g.cbytes);
            for (int blk = 0; blk < bw * bh && !status; ++blk) {
                if constexpr (!WHOLE) {
                    if (mcu == mcu0 && first + blk < slot0) continue;      // in front of the run's first block
                    if (left <= 0) break;
                    --left;
                }
                int coef = 0;
                // DC
                int s = jd_symbol(b, dc);
                if (s < 0 || s > 16) status = VSC_JPEG_STATUS_CODE;
                else {
                    if (s) pred[c] = (int16_t)(pred[c] + jd_receive(b, s));
                    if (lane == 0) coef = pred[c];
                    // AC
                    int k = 1;
                    while (k < 64) {
                        s = jd_symbol(b, ac);
                        if (s < 0) {
                            status = VSC_JPEG_STATUS_CODE;
                            break;
                        }
                        const int r = s >> 4;
                        s &= 15;
                        if (s) {
                            k += r;
                            if (k > 63) {
                                status = VSC_JPEG_STATUS_RUN;
                                break;
                            }
                            const int v = jd_receive(b, s);
                            if (lane == jd_zigzag(k)) coef = v;
                            ++k;
                        } else if (r == 15) k += 16;
                        else break;
                    }
                }
                if (!status && b.avail < 0) status = VSC_JPEG_STATUS_DATA;
                if (status) break;
                // dequantise; columns, then rows, on lanes 0 .. 7
                jd_ws[0][lane] = (uint32_t)coef * (uint32_t)quant[lane];
                __syncthreads();
                uint32_t d[8];
                if (lane < 8) {
                    for (int i = 0; i < 8; ++i) d[i] = jd_ws[0][8 * i + lane];
                    jd_idct8(d, 11);
                    for (int i = 0; i < 8; ++i) jd_ws[1][8 * i + lane] = d[i];
                }
                __syncthreads();
                if (lane < 8) {
                    for (int i = 0; i < 8; ++i) d[i] = jd_ws[1][8 * lane + i];
                    jd_idct8(d, 18);
                    uint32_t lo = 0, hi = 0;
                    for (int i = 0; i < 4; ++i) lo |= jd_range_limit(d[i]) << (8 * i), hi |= jd_range_limit(d[4 + i]) << (8 * i);
                    const int by = mrow * bh + blk / bw, bx = mcol * bw + blk % bw;
                    uint32_t *row = (uint32_t *)(plane + (long long)(by * 8 + lane) * pitch + bx * 8);     // planes and pitches are multiples of 8
                    row[0] = lo, row[1] = hi;
                }
            }
        }
        if (++mcol == g.mx) mcol = 0, ++mrow;
    }
    if (!WHOLE && !status && end_off >= 0) {
        // the run ended with the MCU in front of `mcu`: the RSTn of that place, at the byte the row gives
        if (f.restart <= 0 || j1 % bpm != 0 || mcu != j1 / bpm || mcu >= mcus || mcu % f.restart != 0 || !jd_restart_ahead(b, (mcu / f.restart - 1) & 7) || b.pos != end_off)
            status = VSC_JPEG_STATUS_RESTART;
    }
    return status;
}

// the whole decode of one wave: the frame's table set to LDS, the reader at (byte, bit), the blocks
#define JD_DECODE_LDS                                   \
    __shared__ uint32_t jd_set[JD_SET_BYTES / 4];       \
    __shared__ uint32_t jd_win[JD_WINDOW / 4];          \
    __shared__ uint32_t jd_ws[2][64]

__device__ inline void jd_load_set(uint32_t *jd_set, const uint32_t *sets, int set) {
    const uint32_t *gset = sets + (size_t)set * (JD_SET_BYTES / 4);
    for (int i = threadIdx.x; i < JD_SET_BYTES / 4; i += JD_WAVE) jd_set[i] = gset[i];
    __syncthreads();
}

template <class B> __device__ inline void jd_open(B &b, const uint8_t *seg, int len, uint32_t *win) {
    b.seg = seg, b.win = win, b.len = len, b.wbase = -(1 << 30);
}

// ---- upsampling and colour ---------------------------------------------------------------------------------------------------------
struct JdPixel {
    const uint8_t *y, *cb, *cr;
    int sampling, ypitch, cpitch, dw, dh;     // dw, dh: the chroma planes' real size
};

__device__ inline int jd_chroma(const uint8_t *p, const JdPixel &q, int yy, int x) {
    if (q.sampling == 1) return p[(long long)yy * q.cpitch + x];
    const int i = x >> 1;
    if (q.sampling == 2) {
        const uint8_t *row = p + (long long)yy * q.cpitch;
        if (q.dw <= 2) return row[i];
        const int c = row[i];
        return x & 1 ? (3 * c + row[i + 1 < q.dw ? i + 1 : i] + 2) >> 2 : (3 * c + row[i > 0 ? i - 1 : 0] + 1) >> 2;
    }
    const int r = yy >> 1;
    if (q.dw <= 2) return p[(long long)r * q.cpitch + i];
    const int r2 = yy & 1 ? (r + 1 < q.dh ? r + 1 : r) : (r > 0 ? r - 1 : 0);
    const uint8_t *near = p + (long long)r * q.cpitch, *far = p + (long long)r2 * q.cpitch;
    const int j = x & 1 ? (i + 1 < q.dw ? i + 1 : i) : (i > 0 ? i - 1 : 0);
    const int here = 3 * near[i] + far[i], side = 3 * near[j] + far[j];
    return (3 * here + side + (x & 1 ? 7 : 8)) >> 4;
}

__device__ inline int jd_clip(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// the pixel as r | g << 8 | b << 16
__device__ inline uint32_t jd_rgb(const JdPixel &q, int yy, int x) {
    const int y = q.y[(long long)yy * q.ypitch + x];
    if (q.sampling == 0) return (uint32_t)y * 0x010101u;
    const int cb = jd_chroma(q.cb, q, yy, x) - 128, cr = jd_chroma(q.cr, q, yy, x) - 128;
    const int r = jd_clip(y + ((91881 * cr + 32768) >> 16));
    const int g = jd_clip(y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    const int bl = jd_clip(y + ((116130 * cb + 32768) >> 16));
    return (uint32_t)r | (uint32_t)g << 8 | (uint32_t)bl << 16;
}

// the colour kernel's body: one workgroup of JD_COLOR_BLOCK threads per (frame, band, tile) of the chunk a describes
__device__ inline void jd_color_tile(const JdArgs &a) {
    // the frame of this workgroup: the last whose first workgroup is not behind it
    int lo = 0, hi = a.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.frames[mid].wg0 <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const JdFrame f = a.frames[lo];
    const JdGeom g = jd_geom(f.h, f.w, f.sampling);
    const int tiles = (f.w + JD_TILE - 1) / JD_TILE;
    const int local = (int)blockIdx.x - f.wg0, band = local / tiles, tile = local - band * tiles;
    const int r0 = band * JD_BAND, r1 = r0 + JD_BAND < f.h ? r0 + JD_BAND : f.h;
    if (r0 >= f.h) return;
    const int c0 = tile * JD_TILE, cw = c0 + JD_TILE < f.w ? JD_TILE : f.w - c0;
    JdPixel q;
    q.y = a.planes + f.plane_off, q.cb = q.y + g.ybytes, q.cr = q.cb + g.cbytes;
    q.sampling = f.sampling, q.ypitch = g.ypitch, q.cpitch = g.cpitch;
    q.dw = (f.w + g.hs - 1) / g.hs, q.dh = (f.h + g.vs - 1) / g.vs;

    const long long rowbytes = (long long)f.w * 3;
    const int segbytes = cw * 3;
    const int dwr = (segbytes + 6) >> 2;                       // dwords that cover a segment starting up to 3 bytes into one
    uint8_t *out0 = a.out + f.out_off + r0 * rowbytes + c0 * 3;
    for (int item = threadIdx.x; item < (r1 - r0) * dwr; item += JD_COLOR_BLOCK) {
        const int r = item / dwr, d = item - r * dwr;
        uint8_t *seg = out0 + r * rowbytes;
        const int off = d * 4 - (int)((uintptr_t)seg & 3);     // the dword's first byte, from the segment's start
        if (off >= segbytes) continue;
        // bytes off .. off + 3 lie in at most two pixels of the tile
        const int first = off < 0 ? 0 : off, last = off + 3 < segbytes ? off + 3 : segbytes - 1;
        const int p0 = first / 3, p1 = last / 3;
        const unsigned long long two = (unsigned long long)jd_rgb(q, r0 + r, c0 + p0) | (p1 != p0 ? (unsigned long long)jd_rgb(q, r0 + r, c0 + p1) << 24 : 0ull);
        if (off >= 0 && off + 4 <= segbytes) *(uint32_t *)(seg + off) = (uint32_t)(two >> (8 * (off - 3 * p0)));
        else
            for (int e = first; e <= last; ++e) seg[e] = (uint8_t)(two >> (8 * (e - 3 * p0)));
    }
}
// ---- host ---------------------------------------------------------------------------------------------------------------------------
// a caller's table set (VSC_JPEG_TABLE_SET_BYTES) -> the kernel's; false: a Huffman table whose code lengths describe no prefix code
bool jd_build_set(const uint8_t *src, uint32_t *dst_words) {
    uint8_t *dst = (uint8_t *)dst_words;
    memset(dst, 0, JD_SET_BYTES);
    uint16_t *quant = (uint16_t *)dst;
    for (int t = 0; t < 4; ++t)
        for (int k = 0; k < 64; ++k) quant[t * 64 + jd_zigzag(k)] = (uint16_t)(src[(t * 64 + k) * 2] | src[(t * 64 + k) * 2 + 1] << 8);
    const int hmask = src[1601];
    for (int t = 0; t < 4; ++t) {
        uint8_t *p = dst + 512 + t * JD_HUFF_BYTES;
        uint16_t *lut = (uint16_t *)p;
        int32_t *maxcode = (int32_t *)(p + (2 << JD_LOOK)), *valoff = maxcode + 18;
        uint8_t *vals = (uint8_t *)(valoff + 18);
        for (int l = 0; l < 18; ++l) maxcode[l] = -1, valoff[l] = 0;
        if (!(hmask >> t & 1)) continue;
        const uint8_t *bits = src + 512 + 16 * t, *v = src + 576 + 256 * t;
        memcpy(vals, v, 256);
        int code = 0, k = 0;
        for (int l = 1; l <= 16; ++l) {
            valoff[l] = k - code;
            for (int i = 0; i < bits[l - 1]; ++i, ++code, ++k) {
                if (k >= 256 || code >= (1 << l)) return false;
                if (l <= JD_LOOK)
                    for (int e = 0; e < (1 << (JD_LOOK - l)); ++e) lut[(code << (JD_LOOK - l)) + e] = (uint16_t)(l << 8 | v[k]);
            }
            if (bits[l - 1]) maxcode[l] = code - 1;
            code <<= 1;
        }
    }
    return true;
}

struct JdBuffer {              // grow-only device memory of a handle
    void *ptr = nullptr;
    size_t bytes = 0;
};
int jd_grow(JdBuffer &b, size_t bytes) {
    if (bytes <= b.bytes) return VSC_OK;
    if (b.ptr) VSC_CHECK_HIP(hipFree(b.ptr));      // waits for what still reads it
    b.ptr = nullptr, b.bytes = 0;
    VSC_CHECK_HIP(hipMalloc(&b.ptr, bytes));
    b.bytes = bytes;
    return VSC_OK;
}

}  // namespace

struct vsc_jpeg_decode {
    hipStream_t stream;
    long long cap = JD_DEFAULT_CAP;
    long long last_chunks = 0;
    JdBuffer planes, meta;                                            // meta: the call's frame table and table sets as the kernels read them
    std::map<std::string, std::vector<uint32_t>> built;              // table sets by content
    // vsc_jpeg_decode_split_u8 (csrc/jpeg_split.hip)
    int split_mode = 3, sub_bytes = 1024, rounds = 2, item_bytes = 1024;
    JdBuffer sync;                                                    // sub-stream states (two buffers), item statuses, per-frame fallback flags
    long long stat_markers = 0, stat_subs = 0, stat_unsplit = 0, stat_items = 0, stat_frames = 0;
    size_t stat_flags_at = 0;                                         // where the last call's fallback flags (int32 per frame) stand in sync
};

namespace {

struct JdPlan {                                        // a call's frames, checked, and its chunks
    std::vector<JdFrame> frames;
    std::vector<int64_t> chunk_first;                  // first frame of every chunk
    std::vector<int> chunk_wgs;                        // workgroups of its colour launch
    long long most = 0;                                // plane bytes of the largest chunk
};

// the operands of vsc_jpeg_decode_u8, every frame checked before anything is launched -> the frame table and the chunks
int jd_plan(vsc_jpeg_decode *h, int64_t bytes_len, const int64_t *frames_host, int64_t n_frames, const uint8_t *tables_host, int32_t n_table_sets,
            int64_t out_len, JdPlan &p) {
    for (int s = 0; s < n_table_sets; ++s)
        VSC_REQUIRE(!(tables_host[(size_t)s * VSC_JPEG_TABLE_SET_BYTES + 1600] & ~15) && !(tables_host[(size_t)s * VSC_JPEG_TABLE_SET_BYTES + 1601] & ~15),
                    "jpeg_decode: table set %d: bad presence masks", s);
    std::vector<JdFrame> &frames = p.frames;
    std::vector<int64_t> &chunk_first = p.chunk_first;
    std::vector<int> &chunk_wgs = p.chunk_wgs;
    frames.resize((size_t)n_frames);
    long long used = 0, most = 0;
    for (int64_t i = 0; i < n_frames; ++i) {
        const int64_t *r = frames_host + JD_FRAME_ROW * i;
        JdFrame &f = frames[(size_t)i];
        VSC_REQUIRE(r[0] >= 0 && r[1] >= 0 && r[1] < (1ll << 31) && r[0] <= bytes_len - r[1], "jpeg_decode: frame %lld: segment [%lld, +%lld) outside the %lld bytes",
                    (long long)i, (long long)r[0], (long long)r[1], (long long)bytes_len);
        VSC_REQUIRE(r[2] >= 1 && r[2] <= VSC_JPEG_MAX_SIDE && r[3] >= 1 && r[3] <= VSC_JPEG_MAX_SIDE, "jpeg_decode: frame %lld: %lld x %lld pixels (1 .. %d a side)",
                    (long long)i, (long long)r[2], (long long)r[3], VSC_JPEG_MAX_SIDE);
        VSC_REQUIRE(r[4] >= 0 && r[4] <= 3, "jpeg_decode: frame %lld: sampling class %lld", (long long)i, (long long)r[4]);
        VSC_REQUIRE(r[5] >= 0 && r[5] <= 65535, "jpeg_decode: frame %lld: restart interval %lld", (long long)i, (long long)r[5]);
        VSC_REQUIRE(r[6] >= 0 && r[6] < n_table_sets, "jpeg_decode: frame %lld: table set %lld of %d", (long long)i, (long long)r[6], n_table_sets);
        VSC_REQUIRE(r[7] >= 0 && r[7] <= out_len - r[2] * r[3] * 3, "jpeg_decode: frame %lld: output [%lld, +%lld) outside the %lld bytes", (long long)i,
                    (long long)r[7], (long long)(r[2] * r[3] * 3), (long long)out_len);
        const int ncomp = r[4] == 0 ? 1 : 3;
        VSC_REQUIRE(r[8] >= 0 && r[8] < (1ll << (8 * ncomp)), "jpeg_decode: frame %lld: component word %lld", (long long)i, (long long)r[8]);
        const uint8_t *set = tables_host + (size_t)r[6] * VSC_JPEG_TABLE_SET_BYTES;
        for (int c = 0; c < ncomp; ++c) {
            const int sel = (int)(r[8] >> (8 * c)) & 255;
            VSC_REQUIRE(sel < 16 && (set[1600] >> (sel & 3) & 1) && (set[1601] >> ((sel >> 2) & 1) & 1) && (set[1601] >> (2 + ((sel >> 3) & 1)) & 1),
                        "jpeg_decode: frame %lld: component %d uses a table its set does not hold", (long long)i, c);
        }
        f.seg_off = r[0], f.seg_len = (int)r[1], f.h = (int)r[2], f.w = (int)r[3], f.sampling = (int)r[4], f.restart = (int)r[5], f.set = (int)r[6];
        f.out_off = r[7], f.comp = (int)r[8];
        const JdGeom g = jd_geom(f.h, f.w, f.sampling);
        const long long need = (g.ybytes + 2 * g.cbytes + 15) & ~15ll;
        const long long wgs = (long long)((f.h + JD_BAND - 1) / JD_BAND) * ((f.w + JD_TILE - 1) / JD_TILE);
        // a new chunk where the planes would pass the cap (one frame may exceed it) or the colour grid 2^30 workgroups
        if (chunk_first.empty() || used + need > h->cap || chunk_wgs.back() + wgs > (1ll << 30)) chunk_first.push_back(i), chunk_wgs.push_back(0), used = 0;
        f.plane_off = used, f.wg0 = chunk_wgs.back();
        used += need, chunk_wgs.back() += (int)wgs;
        most = used > most ? used : most;
    }
    p.most = most;
    return VSC_OK;
}

// the table sets as the kernels read them (built once per content and handle) into words[0 .. n_table_sets * JD_SET_BYTES / 4)
int jd_sets(vsc_jpeg_decode *h, const uint8_t *tables_host, int32_t n_table_sets, uint32_t *words) {
    const size_t set_words = JD_SET_BYTES / 4;
    for (int s = 0; s < n_table_sets; ++s) {
        const std::string key((const char *)tables_host + (size_t)s * VSC_JPEG_TABLE_SET_BYTES, VSC_JPEG_TABLE_SET_BYTES);
        auto it = h->built.find(key);
        if (it == h->built.end()) {
            std::vector<uint32_t> built(set_words);
            VSC_REQUIRE(jd_build_set((const uint8_t *)key.data(), built.data()), "jpeg_decode: table set %d: a Huffman table's lengths describe no prefix code", s);
            it = h->built.emplace(key, std::move(built)).first;
        }
        memcpy(words + (size_t)s * set_words, it->second.data(), JD_SET_BYTES);
    }
    return VSC_OK;
}

}  // namespace
