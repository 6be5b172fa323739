// JPEG decoding in parallel inside a frame: vsc_jpeg_decode_split_u8, behind vsc_jpeg_decode_u8's contract (same bytes, same status).
// The unit of work is the ITEM: a run of consecutive blocks of one frame whose start state is known -- the bit position in the
// entropy-coded segment, the index of the first block in scan order, the number of blocks and the three DC predictors.  One wave
// decodes one item with the body of csrc/jpeg_decode.hip (jpeg_decode_dev.h: jd_decode_blocks); the one-wave path is the item
// "the whole frame from bit 0".  Two sources supply items:
//
//   restart intervals: the caller passes the offsets of the frame's RSTn markers (vsc_hip/jpeg.py finds them in the loader workers).
//     The host groups consecutive intervals into items of at least item_bytes entropy bytes.  An item that is not its frame's last
//     ends with the check the one-wave path makes before it crosses a marker, and the marker must stand where the next item says
//     it does: a lying offset or a marker out of sequence is VSC_JPEG_STATUS_RESTART, never a write outside the frame's planes.
//
//   self-synchronising sub-streams (frames without restart intervals): the segment is cut every sub_bytes raw bytes.
//     jpeg_sync_kernel, one wave per sub-stream, decodes symbols only from a state (raw bit position of a block start, slot of
//     that block in its MCU) to the first block start at or behind the sub-stream's end; a code in no table, a run past
//     coefficient 63 or a block that runs out of bytes moves the block start one bit on.  Round 0 starts sub-stream i at
//     (8 i sub_bytes, 0); each of the `rounds` verification rounds (one launch each, two state buffers: a round reads only its
//     predecessor's output) starts it at sub-stream i - 1's exit and records whether its own exit changed; a wave whose start did not
//     change copies its row forward.  A frame has converged iff the last round changed no exit: the exits are then a fixed point of
//     x_i = F_i(x_{i-1}) with x_0 true, hence all true.  jpeg_item_table_kernel, one thread per frame, takes the exclusive prefix sums
//     of block counts and DC differences and writes the item rows; a frame that has not converged, whose counts do not add up to
//     its blocks or whose slots do not fit becomes "item 0: the whole frame from bit 0, the others empty" -- the one-wave path
//     inside the same launch, so a damaged scan reports what it reports there.
//
// Every item writes its own status; jpeg_item_status_kernel, one thread per frame, takes the first non-zero one in item order.
// No workgroup waits on another, every loop is bounded by a bit position or a coefficient index that advances, and all stores are
// plain vector stores.  The colour launch is csrc/jpeg_decode.hip's (the same body, jd_color_tile).
#include "common.h"

#include <cstring>
#include <map>
#include <string>
#include <vector>

#ifndef JD_UNIFORM
#define JD_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#endif
// the handle's statistics come back with a blocking copy (vsc_jpeg_decode_stats)
#ifndef JD_COPY_BACK
#define JD_COPY_BACK(dst, src, bytes) hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)
#endif

#include "jpeg_decode_dev.h"

namespace {

constexpr int JS_TABLE_BLOCK = 64;
constexpr int JS_MAX_ROUNDS = 128;

struct JsItem {                     // 32 bytes
    int frame;                      // of the call
    int byte, bit;                  // where the first block starts in the segment
    int block0, nblocks;            // nblocks == 0: an empty item
    int end_off;                    // the byte of the segment at which the RSTn behind the item stands; -1: none is checked
    int16_t pred[3], pad;
};

struct JsFrame {                    // per frame of the call
    int sub0, nsub;                 // its sub-stream rows (nsub == 0: its items are the host's)
    int item0, nitem;
};

struct JsSync {                     // the state of one sub-stream after a round
    long long pos, start_pos;       // raw bit positions: the exit, and the start it was decoded from
    int slot, start_slot;
    int count, changed;             // blocks started; the exit differs from the previous round's
    uint16_t sum[3], pad;           // DC differences per component, mod 2^16
};

struct JsArgs {
    const uint8_t *bytes;
    const JdFrame *frames;          // the CALL's frames
    const JsFrame *split;
    const uint32_t *sets;
    uint8_t *planes;
    JsItem *items;                  // item kernel: the chunk's; table kernel: the call's
    int32_t *item_status;           // likewise
    const int *sub_frame;           // the frame of every sub-stream row
    const JsSync *prev;
    JsSync *cur;
    int32_t *fell, *status;         // per frame: fell back to one item; the chunk's status entries
    int n, round, sub_bytes, frame0;
};

// one block's symbols from the reader's position: 0, or the VSC_JPEG_STATUS_* of what stops it
__device__ inline int js_skip_block(JdRawBits &b, const JdHuff &dc, const JdHuff &ac, int *diff) {
    int s = jd_symbol(b, dc);
    if (s < 0 || s > 16) return VSC_JPEG_STATUS_CODE;
    *diff = s ? jd_receive(b, s) : 0;
    int k = 1;
    while (k < 64) {
        s = jd_symbol(b, ac);
        if (s < 0) return VSC_JPEG_STATUS_CODE;
        const int r = s >> 4;
        s &= 15;
        if (s) {
            k += r;
            if (k > 63) return VSC_JPEG_STATUS_RUN;
            jd_fill(b);
            jd_skip(b, s);
            ++k;
        } else if (r == 15) k += 16;
        else break;
    }
    return b.avail < 0 ? VSC_JPEG_STATUS_DATA : 0;
}

__global__ __launch_bounds__(JD_WAVE) void jpeg_sync_kernel(JsArgs a) {
    __shared__ uint32_t jd_set[JD_SET_BYTES / 4];
    __shared__ uint32_t jd_win[JD_WINDOW / 4];
    if ((int)blockIdx.x >= a.n) return;
    const int fr = a.sub_frame[blockIdx.x];
    const JsFrame sf = a.split[fr];
    const int i = (int)blockIdx.x - sf.sub0;
    long long pos = 0;
    int slot = 0;
    if (i > 0) {
        if (a.round == 0) pos = 8ll * i * a.sub_bytes;
        else pos = a.prev[blockIdx.x - 1].pos, slot = a.prev[blockIdx.x - 1].slot;
    }
    JsSync out;
    if (a.round > 0) {
        out = a.prev[blockIdx.x];
        if (out.start_pos == pos && out.start_slot == slot) {      // the same start: the same row
            out.changed = 0;
            if (threadIdx.x == 0) a.cur[blockIdx.x] = out;
            return;
        }
    }
    const long long old_pos = a.round > 0 ? out.pos : -1;
    const int old_slot = a.round > 0 ? out.slot : -1;
    const JdFrame f = a.frames[fr];
    jd_load_set(jd_set, a.sets, f.set);
    const JdGeom g = jd_geom(f.h, f.w, f.sampling);
    const int ylum = g.hs * g.vs, bpm = g.ncomp == 3 ? ylum + 2 : 1;
    const long long all = 8ll * f.seg_len, cut = 8ll * (i + 1) * a.sub_bytes, end = cut < all ? cut : all;
    JdRawBits b;
    jd_open(b, a.bytes + f.seg_off, f.seg_len, jd_win);
    out.start_pos = pos, out.start_slot = slot, out.pad = 0;
    int count = 0, sum0 = 0, sum1 = 0, sum2 = 0;                   // (scalars: an array indexed by the component would live in scratch)
    bool fresh = true;
    while (pos < end) {                                            // every turn moves pos on by at least one bit
        if (fresh) jd_start(b, (int)(pos >> 3), (int)(pos & 7));
        const int c = slot < ylum ? 0 : slot - ylum + 1;
        const int sel = f.comp >> (8 * c);
        const JdHuff dc = jd_huff(jd_set, (sel >> 2) & 1), ac = jd_huff(jd_set, 2 + ((sel >> 3) & 1));
        int diff = 0;
        if (js_skip_block(b, dc, ac, &diff)) pos += 1, fresh = true;
        else {
            const long long next = jd_rawpos(b);
            fresh = next <= pos;                                   // (cannot happen: a block takes bits)
            pos = fresh ? pos + 1 : next;
            sum0 += c == 0 ? diff : 0, sum1 += c == 1 ? diff : 0, sum2 += c == 2 ? diff : 0;
            count += 1;
            if (++slot == bpm) slot = 0;
        }
    }
    out.pos = pos, out.slot = slot, out.count = count;
    out.sum[0] = (uint16_t)sum0, out.sum[1] = (uint16_t)sum1, out.sum[2] = (uint16_t)sum2;
    out.changed = i == 0 ? 0 : a.round == 0 ? 1 : (pos != old_pos || slot != old_slot);
    if (threadIdx.x == 0) a.cur[blockIdx.x] = out;
}

__global__ __launch_bounds__(JS_TABLE_BLOCK) void jpeg_item_table_kernel(JsArgs a) {
    const int fr = (int)(blockIdx.x * JS_TABLE_BLOCK + threadIdx.x);
    if (fr >= a.n) return;
    const JsFrame sf = a.split[fr];
    if (sf.nsub == 0) {
        a.fell[fr] = 0;
        return;
    }
    const JdFrame f = a.frames[fr];
    const JdGeom g = jd_geom(f.h, f.w, f.sampling);
    const int bpm = g.ncomp == 3 ? g.hs * g.vs + 2 : 1;
    const long long total = (long long)g.mx * g.my * bpm;
    const JsSync *s = a.prev + sf.sub0;                            // the last round's rows
    JsItem *items = a.items + sf.item0;
    bool ok = true;
    long long blocks = 0;
    for (int i = 0; i < sf.nsub; ++i) {
        const int slot = i ? s[i - 1].slot : 0;
        const long long start = i ? s[i - 1].pos : 0;
        if (s[i].changed || slot != (int)(blocks % bpm) || s[i].start_pos != start || s[i].start_slot != slot || s[i].count < 0) ok = false;
        blocks += s[i].count;
        if (blocks > total) ok = false;
    }
    if (blocks != total) ok = false;
    uint16_t sum[3] = {0, 0, 0};
    blocks = 0;
    for (int i = 0; i < sf.nitem; ++i) {
        JsItem it;
        it.frame = fr, it.end_off = -1, it.pad = 0;
        if (ok) {
            const long long start = i ? s[i - 1].pos : 0;
            it.byte = (int)(start >> 3), it.bit = (int)(start & 7), it.block0 = (int)blocks, it.nblocks = s[i].count;
            for (int c = 0; c < 3; ++c) it.pred[c] = (int16_t)sum[c], sum[c] = (uint16_t)(sum[c] + s[i].sum[c]);
            blocks += s[i].count;
        } else {
            it.byte = it.bit = it.block0 = 0, it.nblocks = i ? 0 : (int)total;
            it.pred[0] = it.pred[1] = it.pred[2] = 0;
        }
        items[i] = it;
    }
    a.fell[fr] = ok ? 0 : 1;
}

__global__ __launch_bounds__(JD_WAVE) void jpeg_item_kernel(JsArgs a) {
    JD_DECODE_LDS;
    if ((int)blockIdx.x >= a.n) return;
    const JsItem it = a.items[blockIdx.x];
    const JdFrame f = a.frames[it.frame];
    const JdGeom g = jd_geom(f.h, f.w, f.sampling);
    const int total = g.mx * g.my * (g.ncomp == 3 ? g.hs * g.vs + 2 : 1);
    // no item writes a block at or beyond the frame's count, and none starts outside the segment
    const bool empty = it.nblocks <= 0 || it.block0 < 0 || it.block0 >= total || it.byte < 0 || it.byte > f.seg_len || it.bit < 0 || it.bit > 7;
    if (empty) {
        if (threadIdx.x == 0) a.item_status[blockIdx.x] = 0;
        return;
    }
    jd_load_set(jd_set, a.sets, f.set);
    JdBits b;
    jd_open(b, a.bytes + f.seg_off, f.seg_len, jd_win);
    jd_start(b, it.byte, it.bit);
    int pred[3] = {it.pred[0], it.pred[1], it.pred[2]};
    const int j1 = it.nblocks < total - it.block0 ? it.block0 + it.nblocks : total;
    const int status = jd_decode_blocks<false>(f, g, b, jd_set, jd_ws, a.planes, it.block0, j1, pred, it.end_off);
    if (threadIdx.x == 0) a.item_status[blockIdx.x] = status;
}

// the frame's status: the first non-zero one of its items, in item order
__global__ __launch_bounds__(JS_TABLE_BLOCK) void jpeg_item_status_kernel(JsArgs a) {
    const int k = (int)(blockIdx.x * JS_TABLE_BLOCK + threadIdx.x);
    if (k >= a.n) return;
    const JsFrame sf = a.split[a.frame0 + k];
    int status = 0;
    for (int i = 0; i < sf.nitem && !status; ++i) status = a.item_status[sf.item0 + i];
    a.status[k] = status;
}

__global__ __launch_bounds__(JD_COLOR_BLOCK) void jpeg_split_color_kernel(JdArgs a) { jd_color_tile(a); }

}  // namespace

extern "C" int vsc_jpeg_decode_split(vsc_jpeg_decode *h, int32_t mode, int32_t sub_bytes, int32_t rounds, int32_t item_bytes) {
    VSC_REQUIRE(h, "jpeg_decode_split: null handle");
    VSC_REQUIRE(mode >= 0 && mode <= 3, "jpeg_decode_split: mode %d (bit 1: restart markers, bit 2: sub-streams)", mode);
    VSC_REQUIRE(sub_bytes == 0 || (sub_bytes >= 32 && sub_bytes % 4 == 0 && sub_bytes <= (1 << 24)), "jpeg_decode_split: %d bytes a sub-stream (a multiple of 4, 32 .. 2^24)",
                sub_bytes);
    VSC_REQUIRE(rounds >= 0 && rounds <= JS_MAX_ROUNDS, "jpeg_decode_split: %d verification rounds (1 .. %d)", rounds, JS_MAX_ROUNDS);
    VSC_REQUIRE(item_bytes >= 0, "jpeg_decode_split: %d bytes an item", item_bytes);
    h->split_mode = mode;
    if (sub_bytes) h->sub_bytes = sub_bytes;
    if (rounds) h->rounds = rounds;
    if (item_bytes) h->item_bytes = item_bytes;
    return VSC_OK;
}

extern "C" int vsc_jpeg_decode_stats(vsc_jpeg_decode *h, int64_t *out) {
    VSC_REQUIRE(h && out, "jpeg_decode_stats: null pointer");
    long long fell = 0;
    if (h->stat_frames > 0) {
        VSC_CHECK_HIP(hipStreamSynchronize(h->stream));
        std::vector<int32_t> flags((size_t)h->stat_frames);
        VSC_CHECK_HIP(JD_COPY_BACK(flags.data(), (const uint8_t *)h->sync.ptr + h->stat_flags_at, flags.size() * 4));
        for (int32_t v : flags) fell += v != 0;
    }
    out[0] = h->stat_markers, out[1] = h->stat_subs - fell, out[2] = h->stat_unsplit + fell, out[3] = h->stat_items;
    return VSC_OK;
}

extern "C" int vsc_jpeg_decode_split_u8(vsc_jpeg_decode *h, const uint8_t *bytes_dev, int64_t bytes_len, const int64_t *frames_host, int64_t n_frames,
                                        const uint8_t *tables_host, int32_t n_table_sets, const int64_t *restart_ptr_host, const int32_t *restart_off_host,
                                        uint8_t *out_dev, int64_t out_len, int32_t *status_dev) {
    VSC_REQUIRE(h, "jpeg_decode_split: null handle");
    VSC_REQUIRE(n_frames >= 0 && n_frames < (1ll << 31) && bytes_len >= 0 && out_len >= 0 && n_table_sets >= 0,
                "jpeg_decode_split: bad sizes: %lld frames, %lld bytes, %lld output bytes, %d table sets", (long long)n_frames, (long long)bytes_len,
                (long long)out_len, n_table_sets);
    h->stat_markers = h->stat_subs = h->stat_unsplit = h->stat_items = h->stat_frames = 0;
    if (n_frames == 0) {
        h->last_chunks = 0;
        return VSC_OK;
    }
    VSC_REQUIRE(frames_host && tables_host && bytes_dev && out_dev && status_dev, "jpeg_decode_split: null pointer");
    JdPlan p;
    VSC_TRY(jd_plan(h, bytes_len, frames_host, n_frames, tables_host, n_table_sets, out_len, p));
    const std::vector<JdFrame> &frames = p.frames;

    // the items of every frame; the marker offsets of every row are checked before anything is launched
    std::vector<JsFrame> split((size_t)n_frames);
    std::vector<JsItem> items;
    std::vector<int> sub_frame;
    long long n_markers = 0, n_subs = 0, n_unsplit = 0;
    if (restart_ptr_host) {
        VSC_REQUIRE(restart_ptr_host[0] == 0, "jpeg_decode_split: the marker rows start at %lld", (long long)restart_ptr_host[0]);
        for (int64_t i = 0; i < n_frames; ++i)
            VSC_REQUIRE(restart_ptr_host[i + 1] >= restart_ptr_host[i] && restart_ptr_host[i + 1] < (1ll << 31), "jpeg_decode_split: frame %lld: marker row [%lld, %lld)",
                        (long long)i, (long long)restart_ptr_host[i], (long long)restart_ptr_host[i + 1]);
        VSC_REQUIRE(restart_ptr_host[n_frames] == 0 || restart_off_host, "jpeg_decode_split: null pointer");
        for (int64_t i = 0; i < n_frames; ++i)
            for (int64_t k = restart_ptr_host[i]; k < restart_ptr_host[i + 1]; ++k) {
                const int32_t off = restart_off_host[k];
                VSC_REQUIRE(off >= 0 && off <= frames[(size_t)i].seg_len - 2 && (k == restart_ptr_host[i] || off >= restart_off_host[k - 1] + 2),
                            "jpeg_decode_split: frame %lld: marker %lld at %d is not behind its predecessor inside the segment of %d bytes", (long long)i,
                            (long long)(k - restart_ptr_host[i]), off, frames[(size_t)i].seg_len);
            }
    }
    for (int64_t i = 0; i < n_frames; ++i) {
        const JdFrame &f = frames[(size_t)i];
        const JdGeom g = jd_geom(f.h, f.w, f.sampling);
        const int bpm = g.ncomp == 3 ? g.hs * g.vs + 2 : 1, mcus = g.mx * g.my;
        JsFrame &sf = split[(size_t)i];
        sf.sub0 = (int)sub_frame.size(), sf.nsub = 0, sf.item0 = (int)items.size(), sf.nitem = 0;
        JsItem it;
        memset(&it, 0, sizeof it);
        it.frame = (int)i, it.end_off = -1;
        const int64_t m0 = restart_ptr_host ? restart_ptr_host[i] : 0, m1 = restart_ptr_host ? restart_ptr_host[i + 1] : 0;
        if (f.restart > 0 && (h->split_mode & 1) && m1 - m0 == (mcus + f.restart - 1) / f.restart - 1) {
            const int32_t *off = restart_off_host + m0;
            const int64_t last = m1 - m0;                          // intervals 0 .. last
            int64_t first = 0;
            long long acc = 0;
            for (int64_t k = 0; k <= last; ++k) {
                acc += (k < last ? off[k] : f.seg_len) - (k ? off[k - 1] + 2 : 0);
                if (acc < h->item_bytes && k < last) continue;
                it.byte = first ? off[first - 1] + 2 : 0;
                it.block0 = (int)(first * f.restart * bpm);
                const long long upto = (k + 1) * f.restart < mcus ? (k + 1) * f.restart : mcus;
                it.nblocks = (int)(upto * bpm) - it.block0;
                it.end_off = k < last ? off[k] : -1;
                items.push_back(it);
                first = k + 1, acc = 0;
            }
            ++n_markers;
        } else if (f.restart == 0 && (h->split_mode & 2) && f.seg_len > 0) {
            sf.nsub = (f.seg_len + h->sub_bytes - 1) / h->sub_bytes;
            VSC_REQUIRE(sub_frame.size() + (size_t)sf.nsub < (1u << 30), "jpeg_decode_split: more than 2^30 sub-streams in one call");
            for (int k = 0; k < sf.nsub; ++k) {
                sub_frame.push_back((int)i);
                it.nblocks = k ? 0 : mcus * bpm;                    // the table kernel writes the rows
                items.push_back(it);
            }
            ++n_subs;
        } else {
            it.nblocks = mcus * bpm;
            items.push_back(it);
            if ((f.restart > 0 && (h->split_mode & 1)) || (f.restart == 0 && (h->split_mode & 2))) ++n_unsplit;
        }
        sf.nitem = (int)items.size() - sf.item0;
        VSC_REQUIRE(items.size() < (1u << 30), "jpeg_decode_split: more than 2^30 items in one call");
    }

    // one upload: table sets, frames, their split rows, the items, the frame of every sub-stream
    const size_t set_words = JD_SET_BYTES / 4;
    const size_t at_frames = (size_t)n_table_sets * set_words, at_split = at_frames + (frames.size() * sizeof(JdFrame) + 7) / 8 * 2;
    const size_t at_items = at_split + split.size() * sizeof(JsFrame) / 4, at_subs = at_items + items.size() * sizeof(JsItem) / 4;
    std::vector<uint32_t> meta(at_subs + sub_frame.size() + 2);
    VSC_TRY(jd_sets(h, tables_host, n_table_sets, meta.data()));
    memcpy(meta.data() + at_frames, frames.data(), frames.size() * sizeof(JdFrame));
    memcpy(meta.data() + at_split, split.data(), split.size() * sizeof(JsFrame));
    memcpy(meta.data() + at_items, items.data(), items.size() * sizeof(JsItem));
    if (!sub_frame.empty()) memcpy(meta.data() + at_subs, sub_frame.data(), sub_frame.size() * 4);
    // device-written state: two buffers of sub-stream rows, item statuses, fallback flags
    const size_t sync_rows = sub_frame.size(), at_status = 2 * sync_rows * sizeof(JsSync), at_fell = at_status + items.size() * 4;
    VSC_TRY(jd_grow(h->meta, meta.size() * 4));
    VSC_TRY(jd_grow(h->planes, (size_t)p.most));
    VSC_TRY(jd_grow(h->sync, at_fell + (size_t)n_frames * 4));
    VSC_CHECK_HIP(hipMemcpyAsync(h->meta.ptr, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, h->stream));

    JsArgs s;
    memset(&s, 0, sizeof s);
    const uint32_t *m = (const uint32_t *)h->meta.ptr;
    s.bytes = bytes_dev, s.sets = m, s.frames = (const JdFrame *)(m + at_frames), s.split = (const JsFrame *)(m + at_split), s.planes = (uint8_t *)h->planes.ptr;
    JsItem *dev_items = (JsItem *)((uint32_t *)h->meta.ptr + at_items);
    int32_t *dev_item_status = (int32_t *)((uint8_t *)h->sync.ptr + at_status);
    s.sub_frame = (const int *)(m + at_subs), s.fell = (int32_t *)((uint8_t *)h->sync.ptr + at_fell), s.sub_bytes = h->sub_bytes;
    s.items = dev_items, s.item_status = dev_item_status;
    JsSync *buf[2] = {(JsSync *)h->sync.ptr, (JsSync *)h->sync.ptr + sync_rows};
    if (sync_rows) {
        for (int r = 0; r <= h->rounds; ++r) {
            s.n = (int)sync_rows, s.round = r, s.cur = buf[r & 1], s.prev = buf[(r & 1) ^ 1];
            hipLaunchKernelGGL(jpeg_sync_kernel, dim3((unsigned)sync_rows), dim3(JD_WAVE), 0, h->stream, s);
            VSC_CHECK_LAUNCH();
        }
        s.prev = buf[h->rounds & 1];
    }
    s.n = (int)n_frames;
    hipLaunchKernelGGL(jpeg_item_table_kernel, dim3((unsigned)((n_frames + JS_TABLE_BLOCK - 1) / JS_TABLE_BLOCK)), dim3(JS_TABLE_BLOCK), 0, h->stream, s);
    VSC_CHECK_LAUNCH();

    JdArgs a;
    a.bytes = bytes_dev, a.sets = m, a.planes = (uint8_t *)h->planes.ptr, a.out = out_dev;
    for (size_t c = 0; c < p.chunk_first.size(); ++c) {
        const int64_t f0 = p.chunk_first[c], f1 = c + 1 < p.chunk_first.size() ? p.chunk_first[c + 1] : n_frames;
        const int i0 = split[(size_t)f0].item0, i1 = split[(size_t)f1 - 1].item0 + split[(size_t)f1 - 1].nitem;
        s.items = dev_items + i0, s.item_status = dev_item_status + i0, s.n = i1 - i0;
        hipLaunchKernelGGL(jpeg_item_kernel, dim3((unsigned)s.n), dim3(JD_WAVE), 0, h->stream, s);
        VSC_CHECK_LAUNCH();
        s.item_status = dev_item_status, s.status = status_dev + f0, s.frame0 = (int)f0, s.n = (int)(f1 - f0);
        hipLaunchKernelGGL(jpeg_item_status_kernel, dim3((unsigned)((s.n + JS_TABLE_BLOCK - 1) / JS_TABLE_BLOCK)), dim3(JS_TABLE_BLOCK), 0, h->stream, s);
        VSC_CHECK_LAUNCH();
        a.frames = s.frames + f0, a.status = status_dev + f0, a.n = (int)(f1 - f0);
        hipLaunchKernelGGL(jpeg_split_color_kernel, dim3((unsigned)p.chunk_wgs[c]), dim3(JD_COLOR_BLOCK), 0, h->stream, a);
        VSC_CHECK_LAUNCH();
    }
    h->last_chunks = (long long)p.chunk_first.size();
    h->stat_markers = n_markers, h->stat_subs = n_subs, h->stat_unsplit = n_unsplit, h->stat_items = (long long)items.size(), h->stat_frames = n_frames;
    h->stat_flags_at = at_fell;
    return VSC_OK;
}
