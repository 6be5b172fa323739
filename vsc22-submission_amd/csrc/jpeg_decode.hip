// Baseline JPEG frames to uint8 [H, W, 3] on the device: vsc_jpeg_decode_u8.  The contract -- libjpeg's default decode path as
// Pillow drives it, bit for bit -- is stated with that entry in include/vsc_hip.h (executable form: tests/jpeg_decode_contract.py).
//
// Two launches per chunk of frames, both with one argument structure and a 1-D grid (which is also what lets the file run on the
// CPU against tests/hip_emu/common.h):
//
// jpeg_scan_idct_kernel, one wave (a workgroup of 64 threads) per frame: the scan of a frame is sequential, so the frame is the
//   unit of parallelism.  The bit buffer, the byte un-stuffing, the Huffman lookups and the restart logic are wave-uniform: every
//   lane holds the same values, and what comes out of LDS goes through JD_UNIFORM (v_readfirstlane) so that the arithmetic behind
//   it runs on the scalar side.  The 64 lanes are the 64 coefficients of the current block in natural order: a decoded
//   coefficient is dropped into the register of the lane at its de-zigzagged position.  At the end of a block all lanes
//   dequantise into LDS, lanes 0..7 run jpeg_idct_islow's column pass and then its row pass through LDS, range-limit and store
//   the block's 8 rows of 8 bytes into the component's plane (uint8, MCU-padded, in the handle's scratch).  No coefficient goes
//   to HBM.  The bitstream is staged into a 256-byte LDS window with aligned dword loads that never leave the frame's segment;
//   the frame's table set (quantisation tables in natural order, per Huffman table a 9-bit lookup table plus libjpeg's maxcode /
//   valoffset arrays for longer codes) is copied to LDS once.  A code that is in no table, a run past coefficient 63, a missing
//   or wrong RSTn and a scan that runs out of bytes set the frame's status (VSC_JPEG_STATUS_*) and end the frame; nothing is read
//   outside the segment or written outside the frame's own planes.
//
// jpeg_color_kernel, one workgroup per (frame, band of JD_BAND rows, tile of JD_TILE columns): Y, Cb, Cr from the planes with
//   libjpeg's "fancy" triangle upsampling (edges replicated at the component's real down-sampled size; plain replication when
//   the down-sampled width is 2 or less), the 16-bit fixed-point YCbCr -> RGB, packed RGB out.  A thread owns one ALIGNED dword
//   of global memory inside a row's segment of the tile and stores it whole; only the partial dwords at the two ends of a segment
//   are byte stores, each byte by its owner, so neighbouring tiles, rows and frames never write the same byte (frame_inputs.hip's
//   rule).
//
// Integer arithmetic throughout; the IDCT runs in wrapping 32-bit arithmetic, which equals libjpeg's for every stream an encoder
// writes and stays defined for corrupt ones.
//
// The reader, the Huffman lookups, the IDCT, the decode body of a run of blocks and the colour body are in jpeg_decode_dev.h, which
// csrc/jpeg_split.hip (vsc_jpeg_decode_split_u8: one wave per ITEM of a frame) shares: the kernel here is the run "the whole frame".
#include "common.h"
#include <cstring>
#include <map>
#include <string>
#include <vector>

// a value every lane of the wave holds: kept in a scalar register
#ifndef JD_UNIFORM
#define JD_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#endif

#include "jpeg_decode_dev.h"

namespace {

__global__ __launch_bounds__(JD_WAVE) void jpeg_scan_idct_kernel(JdArgs a) {
    JD_DECODE_LDS;
    if ((int)blockIdx.x >= a.n) return;
    const JdFrame f = a.frames[blockIdx.x];
    jd_load_set(jd_set, a.sets, f.set);
    const JdGeom g = jd_geom(f.h, f.w, f.sampling);
    JdBits b;
    jd_open(b, a.bytes + f.seg_off, f.seg_len, jd_win);
    jd_start(b, 0, 0);
    int pred[3] = {0, 0, 0};
    const int status = jd_decode_blocks<true>(f, g, b, jd_set, jd_ws, a.planes, 0, g.mx * g.my * (g.ncomp == 3 ? g.hs * g.vs + 2 : 1), pred, -1);
    if (threadIdx.x == 0) a.status[blockIdx.x] = status;
}

__global__ __launch_bounds__(JD_COLOR_BLOCK) void jpeg_color_kernel(JdArgs a) { jd_color_tile(a); }

}  // namespace

extern "C" int vsc_jpeg_decode_create(void *stream, vsc_jpeg_decode **out) {
    VSC_REQUIRE(out, "jpeg_decode_create: null pointer");
    *out = new vsc_jpeg_decode;
    (*out)->stream = (hipStream_t)stream;
    return VSC_OK;
}

extern "C" void vsc_jpeg_decode_destroy(vsc_jpeg_decode *h) {
    if (!h) return;
    if (h->planes.ptr) (void)hipFree(h->planes.ptr);
    if (h->meta.ptr) (void)hipFree(h->meta.ptr);
    if (h->sync.ptr) (void)hipFree(h->sync.ptr);
    delete h;
}

extern "C" int vsc_jpeg_decode_scratch(vsc_jpeg_decode *h, int64_t cap_bytes, int64_t *last_chunks, int64_t *scratch_bytes) {
    VSC_REQUIRE(h, "jpeg_decode_scratch: null handle");
    VSC_REQUIRE(cap_bytes >= 0, "jpeg_decode_scratch: cap %lld", (long long)cap_bytes);
    if (cap_bytes) h->cap = cap_bytes;
    if (last_chunks) *last_chunks = h->last_chunks;
    if (scratch_bytes) *scratch_bytes = (int64_t)h->planes.bytes;
    return VSC_OK;
}

extern "C" int vsc_jpeg_decode_u8(vsc_jpeg_decode *h, const uint8_t *bytes_dev, int64_t bytes_len, const int64_t *frames_host, int64_t n_frames,
                                  const uint8_t *tables_host, int32_t n_table_sets, uint8_t *out_dev, int64_t out_len, int32_t *status_dev) {
    VSC_REQUIRE(h, "jpeg_decode: null handle");
    VSC_REQUIRE(n_frames >= 0 && n_frames < (1ll << 31) && bytes_len >= 0 && out_len >= 0 && n_table_sets >= 0,
                "jpeg_decode: bad sizes: %lld frames, %lld bytes, %lld output bytes, %d table sets", (long long)n_frames, (long long)bytes_len,
                (long long)out_len, n_table_sets);
    if (n_frames == 0) {
        h->last_chunks = 0;
        return VSC_OK;
    }
    VSC_REQUIRE(frames_host && tables_host && bytes_dev && out_dev && status_dev, "jpeg_decode: null pointer");
    JdPlan p;
    VSC_TRY(jd_plan(h, bytes_len, frames_host, n_frames, tables_host, n_table_sets, out_len, p));
    const std::vector<JdFrame> &frames = p.frames;
    const std::vector<int64_t> &chunk_first = p.chunk_first;
    const std::vector<int> &chunk_wgs = p.chunk_wgs;
    const size_t set_words = JD_SET_BYTES / 4;
    std::vector<uint32_t> meta((size_t)n_table_sets * set_words + (frames.size() * sizeof(JdFrame) + 3) / 4);
    VSC_TRY(jd_sets(h, tables_host, n_table_sets, meta.data()));
    memcpy(meta.data() + (size_t)n_table_sets * set_words, frames.data(), frames.size() * sizeof(JdFrame));
    VSC_TRY(jd_grow(h->meta, meta.size() * 4));
    VSC_TRY(jd_grow(h->planes, (size_t)p.most));
    VSC_CHECK_HIP(hipMemcpyAsync(h->meta.ptr, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, h->stream));

    // measurement aid (tools/micro/jpeg_decode_bench.py times the two launches apart): VSC_JPEG_STAGES=1 the scan launch only, 2 the
    // colour launch only, over the planes the handle's last call left
    const int stages = vsc_opt_int(OPT_JPEG_STAGES, 3);
    JdArgs a;
    a.bytes = bytes_dev, a.sets = (const uint32_t *)h->meta.ptr, a.planes = (uint8_t *)h->planes.ptr, a.out = out_dev;
    const JdFrame *dev_frames = (const JdFrame *)((const uint32_t *)h->meta.ptr + (size_t)n_table_sets * set_words);
    for (size_t c = 0; c < chunk_first.size(); ++c) {
        const int64_t f0 = chunk_first[c], f1 = c + 1 < chunk_first.size() ? chunk_first[c + 1] : n_frames;
        a.frames = dev_frames + f0, a.status = status_dev + f0, a.n = (int)(f1 - f0);
        if (stages & 1) {
            hipLaunchKernelGGL(jpeg_scan_idct_kernel, dim3((unsigned)a.n), dim3(JD_WAVE), 0, h->stream, a);
            VSC_CHECK_LAUNCH();
        }
        if (stages & 2) {
            hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)chunk_wgs[c]), dim3(JD_COLOR_BLOCK), 0, h->stream, a);
            VSC_CHECK_LAUNCH();
        }
    }
    h->last_chunks = (long long)chunk_first.size();
    return VSC_OK;
}
