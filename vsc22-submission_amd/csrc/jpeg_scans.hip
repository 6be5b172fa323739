// JPEG files of several scans to uint8 [H, W, 3] on the device: vsc_jpeg_decode_scans_u8 -- progressive files (SOF2), sequential
// files of one scan per component, Huffman table ids 0 .. 3, and in the same call the single-scan frames of vsc_jpeg_decode_u8
// (same bytes, same status).  The contract is stated with the entry in include/vsc_hip.h (executable form:
// tests/jpeg_scans_contract.py): the scans of a complete file accumulate the quantised coefficients of its sequential twin, and from
// the coefficients on everything is csrc/jpeg_decode.hip's, bit for bit.
//
// Three launches per chunk of frames, each with one argument structure and a 1-D grid:
//
// jpeg_scans_kernel, one wave per frame.  The wave zeroes the frame's coefficient planes (int16, 64 per block in natural order,
//   over the MCU-padded grid of every component, in the handle's scratch) and walks the frame's scans in file order.  The bit
//   reader, the Huffman lookup and the restart check are jpeg_decode_dev.h's: wave-uniform state, bytes staged in LDS, decisions
//   on the scalar side.  Lane k holds coefficient k (zigzag order) of the current block in a register, and the state the scan's
//   chain depends on is a 64-bit scalar mask of the block's non-zero coefficients:
//     AC first    no history is read: symbols place values << Al on their lanes, lanes Ss .. Se store once; the blocks of an
//                 EOBRUN are skipped by arithmetic.
//     AC refine   the block is loaded once (lane k its coefficient; the next block's load is issued before this block's symbols
//                 are decoded) and __ballot gives the mask.  A symbol (r, s) then costs no walk over coefficients: the (r + 1)-th
//                 zero bit of the mask from the current position on is the landing place, the non-zero bits in front of it say
//                 how many correction bits follow; they are read in one go (up to 63) and every lane picks its own by the
//                 popcount of the mask below it.  The chain is per SYMBOL, not per coefficient.  One store per block.
//     DC          lane 0 stores predictor << Al, or ORs the refinement bit in.
//     sequential  csrc/jpeg_decode.hip's block, stored instead of transformed.
//   EOBRUN is checked against the blocks left in its restart interval or scan when it is decoded, runs against the end of the
//   band, every block against the end of its segment: a damaged scan sets the frame's status and ends the frame.
// jpeg_scans_idct_kernel, eight lanes per block over ALL blocks of the chunk: dequantisation and jpeg_idct_islow (column pass from
//   registers, row pass through LDS), range limit, the block's 8 x 8 bytes into the component's plane.
// jpeg_scans_color_kernel: csrc/jpeg_decode.hip's colour launch (jd_color_tile).
//
// Stores are plain vector stores; no launch waits on the host.
#include "common.h"
#include <cstring>
#include <map>
#include <string>
#include <vector>

#ifndef JD_UNIFORM
#define JD_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#endif

#include "jpeg_decode_dev.h"

namespace {

constexpr int JP_SCAN_ROW = VSC_JPEG_SCAN_ROW;
constexpr int JP_HOST_SET_BYTES = VSC_JPEG_SCAN_TABLE_SET_BYTES;
constexpr int JP_SET_BYTES = 512 + 8 * JD_HUFF_BYTES;   // as the kernel reads it: DC0 DC1 AC0 AC1 DC2 DC3 AC2 AC3 behind the quantisation tables
constexpr int JP_IDCT_THREADS = 256, JP_IDCT_BLOCKS = JP_IDCT_THREADS / 8, JP_IDCT_PITCH = 72;
static_assert(JP_SCAN_ROW == 10 && JP_HOST_SET_BYTES == 512 + 8 * 16 + 8 * 256 + 8, "include/vsc_hip.h states another scan format");
static_assert(JP_SET_BYTES % 16 == 0, "the table set is copied to LDS in dwords");

struct alignas(16) JpQuad {
    uint32_t x[4] = {0u, 0u, 0u, 0u};
};

struct JpScan {                                         // 48 bytes
    long long seg_off;
    int seg_len, comps, ss, se, ah, al, restart, set, huff, pad;
};

struct JpFrame {
    long long coef_off;                                 // the frame's coefficient planes in the chunk's scratch (bytes), Y, Cb, Cr
    int scan0, nscans;                                  // its rows of the call's scan table
    int blk0, nblk;                                     // its blocks in the chunk's IDCT grid
};

struct JpArgs {
    JdArgs jd;                                          // frames, sets, planes, out, status, n: the chunk's
    const JpFrame *pf;
    const JpScan *scans;                                // the call's
    int blocks;                                         // of the chunk
    int limit;                                          // measurement aid: only the first `limit` scans of every frame (0: all)
};

__device__ inline int jp_dc_table(int id) { return (id & 1) + 4 * (id >> 1); }
__device__ inline int jp_ac_table(int id) { return 2 + (id & 1) + 4 * (id >> 1); }

// bits [lo, hi] of a 64-bit mask; lo > hi: none
__device__ inline unsigned long long jp_band(int lo, int hi) {
    if (lo > hi || lo > 63) return 0ull;
    const unsigned long long upto = hi >= 63 ? ~0ull : (1ull << (hi + 1)) - 1ull;
    return upto & ~((1ull << lo) - 1ull);
}

// n more bits (0 .. 24) as an unsigned value
__device__ inline int jp_bits(JdBits &b, int n) {
    if (n == 0) return 0;
    jd_fill(b);
    const int x = jd_peek(b, n);
    jd_skip(b, n);
    return x;
}

// one correction bit for every coefficient of `passed`, in ascending order: the lane of a set bit adds 1 << al away from zero
__device__ inline void jp_correct(JdBits &b, int &v, int lane, unsigned long long passed, int al) {
    const int n = __popcll(passed);
    if (n == 0) return;
    unsigned long long corr = 0;                        // the first bit read is bit n - 1
    for (int got = 0; got < n;) {
        const int t = n - got < 24 ? n - got : 24;
        corr = corr << t | (unsigned long long)(unsigned)jp_bits(b, t);
        got += t;
    }
    if (passed >> lane & 1ull) {
        const int idx = __popcll(passed & ((1ull << lane) - 1ull));
        const int p1 = 1 << al;
        if ((corr >> (n - 1 - idx) & 1ull) && !(v & p1)) v = (int16_t)(v >= 0 ? v + p1 : v - p1);
    }
}

// EOBRUN of the symbol (r, 0), r < 15; -1: longer than the `left` blocks of its restart interval or scan
__device__ inline int jp_eobrun(JdBits &b, int r, int left) {
    const int run = (1 << r) + jp_bits(b, r);
    return run > left ? -1 : run;
}

// one scan of one frame -> 0 or the status that stops the frame
__device__ inline int jp_scan(const JpScan &s, const JdGeom &g, const JdFrame &f, JdBits &b, const uint32_t *set, int16_t *coef, int nat) {
    const int lane = threadIdx.x;
    const int nc = __popcll((unsigned long long)(s.comps & 7));
    const bool seq = s.ss == 0 && s.se == 63, dcscan = s.se == 0;
    if (nc == 0 || (s.comps & ~7) || (g.ncomp == 1 && s.comps != 1) || (!seq && !dcscan && nc != 1) || s.ss > s.se || s.se > 63 || s.al > 13)
        return VSC_JPEG_STATUS_SCRIPT;
    // the units the scan walks: the component's own blocks, or the frame's MCUs
    int units, per_row;
    if (nc == 1) {
        const int c = __ffsll((long long)s.comps) - 1;
        const int cw = c == 0 ? f.w : (f.w + g.hs - 1) / g.hs, ch = c == 0 ? f.h : (f.h + g.vs - 1) / g.vs;
        per_row = (cw + 7) >> 3, units = per_row * ((ch + 7) >> 3);
    } else
        per_row = g.mx, units = g.mx * g.my;
    const bool inband = lane >= s.ss && lane <= s.se;
    const bool refine_ac = !seq && !dcscan && s.ah != 0;
    int pred[3] = {0, 0, 0};
    int eobrun = 0, status = 0;
    // AC refine: the coefficient of the block the loop stands at, loaded one block ahead
    int ahead = 0;
    if (refine_ac && inband) {
        const int c = __ffsll((long long)s.comps) - 1;
        ahead = (coef + (c == 0 ? 0 : g.ybytes + (c - 1) * g.cbytes))[nat];
    }
    int u = 0;
    while (u < units && !status) {
        if (s.restart > 0 && u > 0 && u % s.restart == 0) {
            if (!jd_restart_ahead(b, (u / s.restart - 1) & 7)) return VSC_JPEG_STATUS_RESTART;
            jd_start(b, b.pos + 2, 0);
            pred[0] = pred[1] = pred[2] = 0, eobrun = 0;
        }
        int left = units - u;
        if (s.restart > 0) {
            const int end = (u / s.restart + 1) * s.restart;
            left = (end < units ? end : units) - u;
        }
        if (!seq && !dcscan && s.ah == 0 && eobrun > 0) {   // AC first: the blocks of an EOBRUN hold nothing of this band (eobrun <= left)
            u += eobrun, eobrun = 0;
            continue;
        }
        const int row = u / per_row, col = u - row * per_row;
        for (int c = 0; c < g.ncomp && !status; ++c) {
            if (!(s.comps >> c & 1)) continue;
            const int sel = s.huff >> (8 * c);
            const JdHuff dc = jd_huff(set, jp_dc_table(sel & 3)), ac = jd_huff(set, jp_ac_table((sel >> 2) & 3));
            const int bw = nc == 1 || c != 0 ? 1 : g.hs, bh = nc == 1 || c != 0 ? 1 : g.vs;
            const int pitch = c == 0 ? g.mx * g.hs : g.mx;                      // blocks per row of the component's plane
            int16_t *plane = coef + (c == 0 ? 0 : g.ybytes + (c - 1) * g.cbytes);
            for (int blk = 0; blk < bw * bh && !status; ++blk) {
                int16_t *at = plane + ((long long)(row * bh + blk / bw) * pitch + col * bw + blk % bw) * 64;
                if (seq) {
                    int v = 0;
                    int sz = jd_symbol(b, dc);
                    if (sz < 0 || sz > 16) status = VSC_JPEG_STATUS_CODE;
                    else {
                        if (sz) pred[c] = (int16_t)(pred[c] + jd_receive(b, sz));
                        if (lane == 0) v = pred[c];
                        int k = 1;
                        while (k < 64) {
                            sz = jd_symbol(b, ac);
                            if (sz < 0) {
                                status = VSC_JPEG_STATUS_CODE;
                                break;
                            }
                            const int r = sz >> 4;
                            sz &= 15;
                            if (sz) {
                                k += r;
                                if (k > 63) {
                                    status = VSC_JPEG_STATUS_RUN;
                                    break;
                                }
                                const int x = jd_receive(b, sz);
                                if (lane == k) v = x;
                                ++k;
                            } else if (r == 15) k += 16;
                            else break;
                        }
                    }
                    if (!status) at[nat] = (int16_t)v;
                } else if (dcscan && s.ah == 0) {
                    const int sz = jd_symbol(b, dc);
                    if (sz < 0 || sz > 16) status = VSC_JPEG_STATUS_CODE;
                    else {
                        if (sz) pred[c] = (int16_t)(pred[c] + jd_receive(b, sz));
                        if (lane == 0) at[0] = (int16_t)((uint32_t)pred[c] << s.al);
                    }
                } else if (dcscan) {
                    if (jp_bits(b, 1) && lane == 0) at[0] = (int16_t)(at[0] | (1 << s.al));
                } else if (s.ah == 0) {
                    int v = 0, k = s.ss;
                    bool any = false;
                    while (k <= s.se) {
                        int sz = jd_symbol(b, ac);
                        if (sz < 0) {
                            status = VSC_JPEG_STATUS_CODE;
                            break;
                        }
                        const int r = sz >> 4;
                        sz &= 15;
                        if (sz) {
                            k += r;
                            if (k > s.se) {
                                status = VSC_JPEG_STATUS_RUN;
                                break;
                            }
                            const int x = jd_receive(b, sz);
                            if (lane == k) v = (int16_t)((uint32_t)x << s.al);
                            any = true, ++k;
                        } else if (r == 15) k += 16;
                        else {
                            eobrun = jp_eobrun(b, r, left);
                            if (eobrun < 0) status = VSC_JPEG_STATUS_RUN, eobrun = 0;
                            break;
                        }
                    }
                    if (!status && any && inband) at[nat] = (int16_t)v;
                    if (eobrun > 0) --eobrun;
                } else {
                    int v = ahead;
                    if (u + 1 < units && inband) {
                        const int nrow = (u + 1) / per_row, ncol = u + 1 - nrow * per_row;
                        ahead = (plane + ((long long)nrow * pitch + ncol) * 64)[nat];
                    }
                    unsigned long long nz = __ballot(v != 0);
                    const int p1 = 1 << s.al;
                    int k = s.ss;
                    if (eobrun == 0) {
                        while (k <= s.se) {
                            int sz = jd_symbol(b, ac);
                            if (sz < 0 || (sz & 15) > 1) {
                                status = VSC_JPEG_STATUS_CODE;
                                break;
                            }
                            int r = sz >> 4;
                            sz &= 15;
                            if (sz == 0 && r < 15) {
                                eobrun = jp_eobrun(b, r, left);
                                if (eobrun < 0) status = VSC_JPEG_STATUS_RUN, eobrun = 0;
                                break;
                            }
                            int fresh = 0;
                            if (sz) fresh = jp_bits(b, 1) ? p1 : -p1;                   // the sign comes first
                            unsigned long long z = ~nz & jp_band(k, s.se);
                            for (; r > 0 && z; --r) z &= z - 1ull;                      // the (r + 1)-th zero coefficient from k on
                            if (!z) {
                                status = VSC_JPEG_STATUS_RUN;
                                break;
                            }
                            const int pos = __ffsll((long long)z) - 1;
                            jp_correct(b, v, lane, nz & jp_band(k, pos - 1), s.al);
                            if (sz) {
                                if (lane == pos) v = fresh;
                                nz |= 1ull << pos;
                            }
                            k = pos + 1;
                        }
                    }
                    if (!status && eobrun > 0) {
                        jp_correct(b, v, lane, nz & jp_band(k, s.se), s.al);
                        --eobrun;
                    }
                    if (!status && inband) at[nat] = (int16_t)v;
                }
                if (!status && b.avail < 0) status = VSC_JPEG_STATUS_DATA;
            }
        }
        ++u;
    }
    return status;
}

__global__ __launch_bounds__(JD_WAVE) void jpeg_scans_kernel(JpArgs a) {
    __shared__ uint32_t jp_set[JP_SET_BYTES / 4];
    __shared__ uint32_t jp_win[JD_WINDOW / 4];
    if ((int)blockIdx.x >= a.jd.n) return;
    const JdFrame f = a.jd.frames[blockIdx.x];
    const JpFrame pf = a.pf[blockIdx.x];
    const JdGeom g = jd_geom(f.h, f.w, f.sampling);
    const int lane = threadIdx.x;
    const int nat = jd_zigzag(lane);
    int16_t *coef = (int16_t *)(a.jd.planes + pf.coef_off);
    {   // zero the coefficient planes: whole blocks of 128 bytes, the frame's own
        const long long n16 = (g.ybytes + 2 * g.cbytes) / 8;
        JpQuad *p = (JpQuad *)coef;
        for (long long i = lane; i < n16; i += JD_WAVE) p[i] = JpQuad{};
    }
    int status = 0, loaded = -1;
    const int nscans = a.limit > 0 && a.limit < pf.nscans ? a.limit : pf.nscans;
    for (int si = 0; si < nscans && !status; ++si) {
        const JpScan s = a.scans[pf.scan0 + si];
        __syncthreads();                                // the zeroes and the last scan's stores, before this scan's loads
        if (s.set != loaded) {
            const uint32_t *gset = a.jd.sets + (size_t)s.set * (JP_SET_BYTES / 4);
            for (int i = lane; i < JP_SET_BYTES / 4; i += JD_WAVE) jp_set[i] = gset[i];
            __syncthreads();
            loaded = s.set;
        }
        JdBits b;
        jd_open(b, a.jd.bytes + s.seg_off, s.seg_len, jp_win);
        jd_start(b, 0, 0);
        status = jp_scan(s, g, f, b, jp_set, coef, nat);
    }
    if (lane == 0) a.jd.status[blockIdx.x] = status;
}

// eight lanes per block: lane l the column l, then the row l
__global__ __launch_bounds__(JP_IDCT_THREADS) void jpeg_scans_idct_kernel(JpArgs a) {
    __shared__ uint32_t ws[JP_IDCT_BLOCKS][JP_IDCT_PITCH];
    const int group = threadIdx.x >> 3, l = threadIdx.x & 7;
    const long long j = (long long)blockIdx.x * JP_IDCT_BLOCKS + group;
    const bool valid = j < a.blocks;
    uint32_t d[8];
    uint8_t *dst = nullptr;
    int pitch = 0;
    if (valid) {
        int lo = 0, hi = a.jd.n - 1;                    // the frame of this block: the last whose first block is not behind it
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (a.pf[mid].blk0 <= j) lo = mid;
            else hi = mid - 1;
        }
        const JdFrame f = a.jd.frames[lo];
        const JpFrame pf = a.pf[lo];
        const JdGeom g = jd_geom(f.h, f.w, f.sampling);
        int jj = (int)(j - pf.blk0);
        const int yblocks = (int)(g.ybytes / 64), cblocks = (int)(g.cbytes / 64);
        int c = 0;
        if (jj >= yblocks) c = 1 + (jj - yblocks) / cblocks, jj -= yblocks + (c - 1) * cblocks;
        const int across = c == 0 ? g.mx * g.hs : g.mx;
        const int by = jj / across, bx = jj - by * across;
        const int16_t *src = (const int16_t *)(a.jd.planes + pf.coef_off) + (c == 0 ? 0 : g.ybytes + (c - 1) * g.cbytes) + (long long)jj * 64;
        const uint16_t *quant = (const uint16_t *)(a.jd.sets + (size_t)f.set * (JP_SET_BYTES / 4)) + ((f.comp >> (8 * c)) & 3) * 64;
        for (int i = 0; i < 8; ++i) d[i] = (uint32_t)(int)src[8 * i + l] * (uint32_t)quant[8 * i + l];
        jd_idct8(d, 11);
        for (int i = 0; i < 8; ++i) ws[group][8 * i + l] = d[i];
        pitch = c == 0 ? g.ypitch : g.cpitch;
        dst = a.jd.planes + f.plane_off + (c == 0 ? 0 : g.ybytes + (c - 1) * g.cbytes) + (long long)(by * 8 + l) * pitch + bx * 8;
    }
    __syncthreads();
    if (valid) {
        for (int i = 0; i < 8; ++i) d[i] = ws[group][8 * l + i];
        jd_idct8(d, 18);
        uint32_t lo = 0, hi = 0;
        for (int i = 0; i < 4; ++i) lo |= jd_range_limit(d[i]) << (8 * i), hi |= jd_range_limit(d[4 + i]) << (8 * i);
        uint32_t *row = (uint32_t *)dst;                // planes and pitches are multiples of 8
        row[0] = lo, row[1] = hi;
    }
}

__global__ __launch_bounds__(JD_COLOR_BLOCK) void jpeg_scans_color_kernel(JdArgs a) { jd_color_tile(a); }

// a caller's table set (VSC_JPEG_SCAN_TABLE_SET_BYTES) -> the kernel's, by jd_build_set on its two halves: tables 0 and 1, tables 2 and 3
bool jp_build_set(const uint8_t *src, uint32_t *dst_words) {
    std::vector<uint32_t> half(JD_SET_BYTES / 4);
    for (int part = 0; part < 2; ++part) {
        uint8_t old[VSC_JPEG_TABLE_SET_BYTES];
        memset(old, 0, sizeof old);
        if (part == 0) memcpy(old, src, 512), old[1600] = src[2688];
        int hmask = 0;
        for (int t = 0; t < 4; ++t) {                   // DC a, DC a + 1, AC a, AC a + 1 with a = 2 * part
            const int from = 4 * (t >> 1) + 2 * part + (t & 1);
            memcpy(old + 512 + 16 * t, src + 512 + 16 * from, 16);
            memcpy(old + 576 + 256 * t, src + 640 + 256 * from, 256);
            hmask |= (src[2689] >> from & 1) << t;
        }
        old[1601] = (uint8_t)hmask;
        if (!jd_build_set(old, half.data())) return false;
        if (part == 0) memcpy(dst_words, half.data(), JD_SET_BYTES);
        else memcpy((uint8_t *)dst_words + JD_SET_BYTES, (const uint8_t *)half.data() + 512, 4 * JD_HUFF_BYTES);
    }
    return true;
}

}  // namespace

extern "C" int vsc_jpeg_decode_scans_u8(vsc_jpeg_decode *h, const uint8_t *bytes_dev, int64_t bytes_len, const int64_t *frames_host, int64_t n_frames,
                                        const int64_t *scans_host, const int64_t *scan_ptr_host, const uint8_t *tables_host, int32_t n_table_sets,
                                        uint8_t *out_dev, int64_t out_len, int32_t *status_dev) {
    VSC_REQUIRE(h, "jpeg_decode_scans: null handle");
    VSC_REQUIRE(n_frames >= 0 && n_frames < (1ll << 31) && bytes_len >= 0 && out_len >= 0 && n_table_sets >= 0,
                "jpeg_decode_scans: bad sizes: %lld frames, %lld bytes, %lld output bytes, %d table sets", (long long)n_frames, (long long)bytes_len,
                (long long)out_len, n_table_sets);
    if (n_frames == 0) {
        h->last_chunks = 0;
        return VSC_OK;
    }
    VSC_REQUIRE(frames_host && scans_host && scan_ptr_host && tables_host && bytes_dev && out_dev && status_dev, "jpeg_decode_scans: null pointer");
    VSC_REQUIRE(scan_ptr_host[0] == 0, "jpeg_decode_scans: the scan rows start at %lld", (long long)scan_ptr_host[0]);
    for (int64_t i = 0; i < n_frames; ++i)
        VSC_REQUIRE(scan_ptr_host[i + 1] > scan_ptr_host[i] && scan_ptr_host[i + 1] < (1ll << 31), "jpeg_decode_scans: frame %lld: scan rows [%lld, %lld)", (long long)i,
                    (long long)scan_ptr_host[i], (long long)scan_ptr_host[i + 1]);
    const int64_t n_scans = scan_ptr_host[n_frames];
    for (int s = 0; s < n_table_sets; ++s)
        VSC_REQUIRE(!(tables_host[(size_t)s * JP_HOST_SET_BYTES + 2688] & ~15), "jpeg_decode_scans: table set %d: bad presence mask", s);

    // every frame and every scan script checked before anything is launched
    std::vector<JdFrame> frames((size_t)n_frames);
    std::vector<JpFrame> pframes((size_t)n_frames);
    std::vector<JpScan> scans((size_t)n_scans);
    std::vector<int64_t> chunk_first;
    std::vector<int> chunk_wgs, chunk_blocks;
    long long used = 0, most = 0;
    for (int64_t i = 0; i < n_frames; ++i) {
        const int64_t *r = frames_host + JD_FRAME_ROW * i;
        JdFrame &f = frames[(size_t)i];
        VSC_REQUIRE(r[0] == 0 && r[1] == 0 && r[5] == 0 && r[9] == 0, "jpeg_decode_scans: frame %lld: columns 0, 1, 5 and 9 of a frame row are 0 in this entry", (long long)i);
        VSC_REQUIRE(r[2] >= 1 && r[2] <= VSC_JPEG_MAX_SIDE && r[3] >= 1 && r[3] <= VSC_JPEG_MAX_SIDE, "jpeg_decode_scans: frame %lld: %lld x %lld pixels (1 .. %d a side)",
                    (long long)i, (long long)r[2], (long long)r[3], VSC_JPEG_MAX_SIDE);
        VSC_REQUIRE(r[4] >= 0 && r[4] <= 3, "jpeg_decode_scans: frame %lld: sampling class %lld", (long long)i, (long long)r[4]);
        VSC_REQUIRE(r[6] >= 0 && r[6] < n_table_sets, "jpeg_decode_scans: frame %lld: table set %lld of %d", (long long)i, (long long)r[6], n_table_sets);
        VSC_REQUIRE(r[7] >= 0 && r[7] <= out_len - r[2] * r[3] * 3, "jpeg_decode_scans: frame %lld: output [%lld, +%lld) outside the %lld bytes", (long long)i,
                    (long long)r[7], (long long)(r[2] * r[3] * 3), (long long)out_len);
        const int ncomp = r[4] == 0 ? 1 : 3;
        VSC_REQUIRE(r[8] >= 0 && r[8] < (1ll << (8 * ncomp)), "jpeg_decode_scans: frame %lld: component word %lld", (long long)i, (long long)r[8]);
        const uint8_t *qset = tables_host + (size_t)r[6] * JP_HOST_SET_BYTES;
        for (int c = 0; c < ncomp; ++c) {
            const int sel = (int)(r[8] >> (8 * c)) & 255;
            VSC_REQUIRE(sel < 4 && (qset[2688] >> sel & 1), "jpeg_decode_scans: frame %lld: component %d uses a quantisation table its set does not hold", (long long)i, c);
        }
        f.seg_off = 0, f.seg_len = 0, f.h = (int)r[2], f.w = (int)r[3], f.sampling = (int)r[4], f.restart = 0, f.set = (int)r[6];
        f.out_off = r[7], f.comp = (int)r[8];

        // the scan script: per coefficient of every component the Al it stands at, -1: not yet coded
        int state[3][64];
        for (auto &row : state)
            for (int &v : row) v = -1;
        for (int64_t si = scan_ptr_host[i]; si < scan_ptr_host[i + 1]; ++si) {
            const int64_t *q = scans_host + JP_SCAN_ROW * si;
            VSC_REQUIRE(q[0] >= 0 && q[1] >= 0 && q[1] < (1ll << 31) && q[0] <= bytes_len - q[1], "jpeg_decode_scans: scan %lld: segment [%lld, +%lld) outside the %lld bytes",
                        (long long)si, (long long)q[0], (long long)q[1], (long long)bytes_len);
            VSC_REQUIRE(q[2] >= 1 && q[2] < (1 << ncomp), "jpeg_decode_scans: scan %lld: component mask %lld", (long long)si, (long long)q[2]);
            VSC_REQUIRE(q[3] >= 0 && q[3] <= q[4] && q[4] <= 63 && q[5] >= 0 && q[5] <= 13 && q[6] >= 0 && q[6] <= 13, "jpeg_decode_scans: scan %lld: Ss %lld, Se %lld, Ah %lld, Al %lld",
                        (long long)si, (long long)q[3], (long long)q[4], (long long)q[5], (long long)q[6]);
            VSC_REQUIRE(q[7] >= 0 && q[7] <= 65535, "jpeg_decode_scans: scan %lld: restart interval %lld", (long long)si, (long long)q[7]);
            VSC_REQUIRE(q[8] >= 0 && q[8] < n_table_sets, "jpeg_decode_scans: scan %lld: table set %lld of %d", (long long)si, (long long)q[8], n_table_sets);
            VSC_REQUIRE(q[9] >= 0 && q[9] < (1ll << (8 * ncomp)), "jpeg_decode_scans: scan %lld: Huffman word %lld", (long long)si, (long long)q[9]);
            const int ss = (int)q[3], se = (int)q[4], ah = (int)q[5], al = (int)q[6];
            const bool seq = ss == 0 && se == 63;
            int nc = 0;
            for (int c = 0; c < ncomp; ++c) nc += (int)(q[2] >> c & 1);
            VSC_REQUIRE(seq ? ah == 0 && al == 0 : (ss > 0 || se == 0) && (ss == 0 || nc == 1) && (ah == 0 || al == ah - 1),
                        "jpeg_decode_scans: scan %lld: no scan of a sequential or progressive script (Ss %d, Se %d, Ah %d, Al %d, %d components)", (long long)si, ss, se, ah, al, nc);
            const uint8_t *set = tables_host + (size_t)q[8] * JP_HOST_SET_BYTES;
            for (int c = 0; c < ncomp; ++c) {
                const int sel = (int)(q[9] >> (8 * c)) & 255;
                if (!(q[2] >> c & 1)) {
                    VSC_REQUIRE(sel == 0, "jpeg_decode_scans: scan %lld: Huffman tables for component %d, which is not in the scan", (long long)si, c);
                    continue;
                }
                const bool need_dc = ss == 0 && ah == 0, need_ac = se > 0;
                VSC_REQUIRE(sel < 16 && (!need_dc || (set[2689] >> (sel & 3) & 1)) && (!need_ac || (set[2689] >> (4 + (sel >> 2)) & 1)),
                            "jpeg_decode_scans: scan %lld: component %d uses a Huffman table its set does not hold", (long long)si, c);
                VSC_REQUIRE(ss == 0 || state[c][0] >= 0, "jpeg_decode_scans: scan %lld: an AC scan of component %d before its first DC scan", (long long)si, c);
                for (int k = ss; k <= se; ++k) {
                    VSC_REQUIRE(state[c][k] == (ah ? ah : -1), "jpeg_decode_scans: scan %lld: component %d, coefficient %d: Ah %d does not continue Al %d", (long long)si, c, k, ah,
                                state[c][k]);
                    state[c][k] = al;
                }
            }
            JpScan &s = scans[(size_t)si];
            s.seg_off = q[0], s.seg_len = (int)q[1], s.comps = (int)q[2], s.ss = ss, s.se = se, s.ah = ah, s.al = al, s.restart = (int)q[7], s.set = (int)q[8];
            s.huff = (int)q[9], s.pad = 0;
        }
        for (int c = 0; c < ncomp; ++c)
            for (int k = 0; k < 64; ++k)
                VSC_REQUIRE(state[c][k] == 0, "jpeg_decode_scans: frame %lld: the scans leave coefficient %d of component %d %s", (long long)i, k, c,
                            state[c][k] < 0 ? "uncoded" : "above Al 0");

        const JdGeom g = jd_geom(f.h, f.w, f.sampling);
        const long long samples = g.ybytes + 2 * g.cbytes;                    // a multiple of 64
        const long long pixels = (samples + 15) & ~15ll, need = pixels + 2 * samples;
        const long long wgs = (long long)((f.h + JD_BAND - 1) / JD_BAND) * ((f.w + JD_TILE - 1) / JD_TILE);
        // a new chunk where the scratch would pass the cap (one frame may exceed it) or a grid 2^30 workgroups
        if (chunk_first.empty() || used + need > h->cap || chunk_wgs.back() + wgs > (1ll << 30) || chunk_blocks.back() + samples / 64 > (1ll << 30))
            chunk_first.push_back(i), chunk_wgs.push_back(0), chunk_blocks.push_back(0), used = 0;
        JpFrame &pf = pframes[(size_t)i];
        f.plane_off = used, f.wg0 = chunk_wgs.back();
        pf.coef_off = used + pixels, pf.scan0 = (int)scan_ptr_host[i], pf.nscans = (int)(scan_ptr_host[i + 1] - scan_ptr_host[i]);
        pf.blk0 = chunk_blocks.back(), pf.nblk = (int)(samples / 64);
        used += need, chunk_wgs.back() += (int)wgs, chunk_blocks.back() += pf.nblk;
        most = used > most ? used : most;
    }

    // the call's tables as the kernels read them: table sets (built once per content and handle), frames, scan frames, scans
    const size_t set_words = JP_SET_BYTES / 4;
    auto words = [](size_t bytes) { return (bytes + 15) / 16 * 4; };
    const size_t at_frames = (size_t)n_table_sets * set_words, at_pf = at_frames + words(frames.size() * sizeof(JdFrame));
    const size_t at_scans = at_pf + words(pframes.size() * sizeof(JpFrame)), total = at_scans + words(scans.size() * sizeof(JpScan));
    std::vector<uint32_t> meta(total);
    for (int s = 0; s < n_table_sets; ++s) {
        const std::string key((const char *)tables_host + (size_t)s * JP_HOST_SET_BYTES, JP_HOST_SET_BYTES);    // (the other entries' keys are shorter)
        auto it = h->built.find(key);
        if (it == h->built.end()) {
            std::vector<uint32_t> built(set_words);
            VSC_REQUIRE(jp_build_set((const uint8_t *)key.data(), built.data()), "jpeg_decode_scans: table set %d: a Huffman table's lengths describe no prefix code", s);
            it = h->built.emplace(key, std::move(built)).first;
        }
        memcpy(meta.data() + (size_t)s * set_words, it->second.data(), JP_SET_BYTES);
    }
    memcpy(meta.data() + at_frames, frames.data(), frames.size() * sizeof(JdFrame));
    memcpy(meta.data() + at_pf, pframes.data(), pframes.size() * sizeof(JpFrame));
    memcpy(meta.data() + at_scans, scans.data(), scans.size() * sizeof(JpScan));
    VSC_TRY(jd_grow(h->meta, meta.size() * 4));
    VSC_TRY(jd_grow(h->planes, (size_t)most));
    VSC_CHECK_HIP(hipMemcpyAsync(h->meta.ptr, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, h->stream));

    // measurement aid (tools/micro/jpeg_scans.py): VSC_JPEG_STAGES bit 1 the scan launch, bit 2 the colour launch, bit 4 the IDCT
    // launch, over what the handle's last call left; bits 8 and up: only that many scans of every frame are walked (0: all)
    const int stages = vsc_opt_int(OPT_JPEG_STAGES, 7);
    JpArgs a;
    a.limit = stages >> 8;
    const uint32_t *m = (const uint32_t *)h->meta.ptr;
    a.jd.bytes = bytes_dev, a.jd.sets = m, a.jd.planes = (uint8_t *)h->planes.ptr, a.jd.out = out_dev;
    a.scans = (const JpScan *)(m + at_scans);
    for (size_t c = 0; c < chunk_first.size(); ++c) {
        const int64_t f0 = chunk_first[c], f1 = c + 1 < chunk_first.size() ? chunk_first[c + 1] : n_frames;
        a.jd.frames = (const JdFrame *)(m + at_frames) + f0, a.pf = (const JpFrame *)(m + at_pf) + f0, a.jd.status = status_dev + f0, a.jd.n = (int)(f1 - f0);
        a.blocks = chunk_blocks[c];
        if (stages & 1) {
            hipLaunchKernelGGL(jpeg_scans_kernel, dim3((unsigned)a.jd.n), dim3(JD_WAVE), 0, h->stream, a);
            VSC_CHECK_LAUNCH();
        }
        if (stages & 4) {
            hipLaunchKernelGGL(jpeg_scans_idct_kernel, dim3((unsigned)((a.blocks + JP_IDCT_BLOCKS - 1) / JP_IDCT_BLOCKS)), dim3(JP_IDCT_THREADS), 0, h->stream, a);
            VSC_CHECK_LAUNCH();
        }
        if (stages & 2) {
            hipLaunchKernelGGL(jpeg_scans_color_kernel, dim3((unsigned)chunk_wgs[c]), dim3(JD_COLOR_BLOCK), 0, h->stream, a.jd);
            VSC_CHECK_LAUNCH();
        }
    }
    h->last_chunks = (long long)chunk_first.size();
    return VSC_OK;
}
