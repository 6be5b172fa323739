// Matching-track network inputs built on the device (VSC22-Matching-Track-1st/infer/src/utils.py:18-73 and src/dataset.py:103-144):
// per candidate the query view whose ten best row maxima have the largest mean, and that view's similarity map cropped / zero-padded
// into an R x R canvas on three identical channels -- plus, for the classifier, the transposed map.  The maps are the matrices of
// vsc_pair_similarity_f32 and never leave the device.  The contract is stated with vsc_match_maps_f32 in include/vsc_hip.h
// (executable form: tests/match_maps_contract.py).
//
// Two kernels per chunk of MM_CHUNK items, each with one argument structure and a 1-D grid (which is also what lets the file run
// on the CPU against tests/hip_emu/common.h).  The chunk's item table travels in that structure, so the entry uploads nothing, owns
// no scratch and never waits for the stream:
//  (a) match_view_kernel, one workgroup per item.  A single-view item writes view_start = 0 and reads nothing.  Otherwise wave w
//      scores the views w, w + 4, ...: per row a coalesced sweep of the r_rows columns and a wave maximum; the ten largest row
//      maxima of the view stay sorted in lanes 0 .. 9 (one ballot + one shuffle per row); the mean is summed in numpy's pairwise
//      order.  Maxima are exact and the sum's order is fixed, so the score has no freedom; the first view with the largest score
//      wins.  HBM bound: one read of the multi-view items' matrices.
//  (b) match_canvas_kernel, one workgroup per 64 x 64 canvas tile of an item.  The tile of the chosen view (zero outside the valid
//      h x w) goes through LDS with 65-float rows; the map's slice reads it by rows and the transposed slice by columns, so every
//      global read and write is a run of consecutive floats, and the column reads fall on distinct banks.  Every element of both
//      slices is written.  HBM bound: 12 R^2 bytes written per slice.
#include "common.h"

// the view score is contract arithmetic: every sum rounded on its own, then one correctly rounded division
#pragma clang fp contract(off)

namespace {

constexpr int MM_BLOCK = 256;
constexpr int MM_WAVES = MM_BLOCK / 64;
constexpr int MM_TILE = 64;
constexpr int MM_CHUNK = 128;                 // items per launch: 128 x 24 bytes of kernel arguments (limit 4 KiB)
constexpr int MM_MAX_RES = 1024;
constexpr int MM_TOP = 10;                    // the pairwise summation below is written out for ten values
#ifdef VSC_MATCH_TOP_ROWS
static_assert(MM_TOP == VSC_MATCH_TOP_ROWS, "include/vsc_hip.h states another number of rows");
#endif

struct MmItem {
    long long off;
    int q_rows, r_rows, frames;
};

struct MmArgs {
    const float *sims;
    int32_t *view_start;                      // [n], of this chunk
    float *out;                               // [n * (1 + with_transpose)][R][R][3], of this chunk
    int n, R, tiles, with_transpose;
    MmItem it[MM_CHUNK];
};

__device__ inline float wave_max_f32(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// mean of a[0 .. c-1] (ascending, a[k] held by lane c-1-k of `t`) as np.float32 computes it: numpy's pairwise sum, then one division
__device__ inline float view_score(float t, int c) {
    float a[MM_TOP];
#pragma unroll
    for (int k = 0; k < MM_TOP; ++k) a[k] = __shfl(t, c - 1 - k >= 0 ? c - 1 - k : 0, 64);
    float s;
    if (c < 8) {
        s = a[0];
#pragma unroll
        for (int k = 1; k < 7; ++k)
            if (k < c) s = s + a[k];
    } else {
        s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
        if (c > 8) s = s + a[8];
        if (c > 9) s = s + a[9];
    }
    return s / (float)c;
}

__global__ __launch_bounds__(MM_BLOCK) void match_view_kernel(MmArgs a) {
    __shared__ float s_score[MM_WAVES];
    __shared__ int s_view[MM_WAVES];
    const MmItem it = a.it[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (it.q_rows <= it.frames) {              // one view: nothing to choose, nothing read
        if (tid == 0) a.view_start[blockIdx.x] = 0;
        return;
    }
    const int views = it.q_rows / it.frames;   // whole views: checked by the launcher
    const int c = it.frames < MM_TOP ? it.frames : MM_TOP;
    const float *S = a.sims + it.off;
    float best = -INFINITY;
    int best_v = -1;
    for (int v = wave; v < views; v += MM_WAVES) {
        float t = -INFINITY;                   // lanes 0 .. 9: the largest row maxima so far, descending
        for (int i = 0; i < it.frames; ++i) {
            const float *row = S + ((long long)v * it.frames + i) * it.r_rows;
            float m = -INFINITY;
            for (int x = lane; x < it.r_rows; x += 64) m = fmaxf(m, row[x]);
            m = wave_max_f32(m);
            const int pos = __popcll(__ballot(lane < MM_TOP && t >= m));   // values that stay in front of m
            const float up = __shfl_up(t, 1, 64);
            if (lane < MM_TOP && lane >= pos) t = lane == pos ? m : up;
        }
        const float score = view_score(t, c);
        if (best_v < 0 || score > best) best = score, best_v = v;
    }
    if (lane == 0) s_score[wave] = best, s_view[wave] = best_v;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < MM_WAVES; ++w) {
            const int vw = s_view[w];
            if (vw < 0) continue;
            const float sw = s_score[w];
            if (sw > best || (sw == best && vw < best_v)) best = sw, best_v = vw;
        }
        a.view_start[blockIdx.x] = best_v * it.frames;
    }
}

__global__ __launch_bounds__(MM_BLOCK) void match_canvas_kernel(MmArgs a) {
    __shared__ float tile[MM_TILE][MM_TILE + 1];
    const int R = a.R, item = (int)blockIdx.x / (a.tiles * a.tiles), t = (int)blockIdx.x % (a.tiles * a.tiles);
    const MmItem it = a.it[item];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int y0 = (t / a.tiles) * MM_TILE, x0 = (t % a.tiles) * MM_TILE;
    const int th = min(MM_TILE, R - y0), tw = min(MM_TILE, R - x0);       // the tile's part of the canvas
    const int h = min(min(it.frames, it.q_rows), R), w = min(it.r_rows, R);   // the valid part of the canvas
    int vs = it.q_rows > it.frames ? a.view_start[item] : 0;
    if (vs < 0 || vs + h > it.q_rows) vs = 0;                              // never read outside the item, whatever the buffer holds
    const float *S = a.sims + it.off + (long long)vs * it.r_rows;
    for (int yy = wave; yy < th; yy += MM_WAVES) {
        const int y = y0 + yy, x = x0 + lane;
        tile[yy][lane] = (y < h && x < w) ? S[(long long)y * it.r_rows + x] : 0.f;
    }
    __syncthreads();
    const size_t slice = (size_t)R * R * 3;
    float *o = a.out + (size_t)item * (a.with_transpose ? 2 : 1) * slice;
    for (int yy = wave; yy < th; yy += MM_WAVES) {                         // out[y, x, c] = s[vs + y, x]
        float *dst = o + ((size_t)(y0 + yy) * R + x0) * 3;
        for (int j = lane; j < 3 * tw; j += 64) dst[j] = tile[yy][j / 3];
    }
    if (!a.with_transpose) return;
    o += slice;
    for (int xx = wave; xx < tw; xx += MM_WAVES) {                         // out[x, y, c] = s[vs + y, x]
        float *dst = o + ((size_t)(x0 + xx) * R + y0) * 3;
        for (int j = lane; j < 3 * th; j += 64) dst[j] = tile[j / 3][xx];
    }
}

}  // namespace

int launch_match_maps(const float *sims_dev, int64_t sims_len, const int64_t *items_host, int64_t n_items, int resolution, int with_transpose,
                      int32_t *view_start_dev, float *out_dev, hipStream_t stream) {
    VSC_REQUIRE(n_items >= 0 && n_items < (1ll << 31), "match_maps: %lld items", (long long)n_items);
    VSC_REQUIRE(resolution >= 1 && resolution <= MM_MAX_RES, "match_maps: resolution %d outside [1, %d]", resolution, MM_MAX_RES);
    VSC_REQUIRE(with_transpose == 0 || with_transpose == 1, "match_maps: with_transpose %d is neither 0 nor 1", with_transpose);
    if (n_items == 0) return VSC_OK;
    VSC_REQUIRE(items_host && view_start_dev && out_dev, "match_maps: null pointer");
    for (int64_t i = 0; i < n_items; ++i) {
        const int64_t off = items_host[4 * i], q = items_host[4 * i + 1], r = items_host[4 * i + 2], f = items_host[4 * i + 3];
        VSC_REQUIRE(f >= 1 && f < (1ll << 31), "match_maps: item %lld has %lld frames per view (at least 1)", (long long)i, (long long)f);
        VSC_REQUIRE(q >= 0 && q < (1ll << 31) && r >= 0 && r < (1ll << 31), "match_maps: item %lld is %lld x %lld", (long long)i, (long long)q,
                    (long long)r);
        VSC_REQUIRE(off >= 0 && off <= sims_len && q * r <= sims_len - off && (q * r == 0 || sims_dev),
                    "match_maps: item %lld = (%lld, %lld, %lld) outside the %lld similarities", (long long)i, (long long)off, (long long)q,
                    (long long)r, (long long)sims_len);
        if (q > f) {
            VSC_REQUIRE(r >= 1, "match_maps: item %lld has %lld rows in views of %lld and no columns", (long long)i, (long long)q, (long long)f);
            VSC_REQUIRE(q % f == 0, "match_maps: item %lld has ragged views: %lld rows are not whole views of %lld frames", (long long)i,
                        (long long)q, (long long)f);
        }
    }
    const size_t slice = (size_t)resolution * resolution * 3;
    MmArgs a;
    a.sims = sims_dev;
    a.R = resolution, a.tiles = (resolution + MM_TILE - 1) / MM_TILE, a.with_transpose = with_transpose;   // tiles <= 16
    for (int64_t base = 0; base < n_items; base += MM_CHUNK) {
        a.n = (int)(n_items - base < MM_CHUNK ? n_items - base : MM_CHUNK);
        for (int i = 0; i < MM_CHUNK; ++i) {
            const int64_t *p = items_host + 4 * (base + (i < a.n ? i : 0));
            a.it[i] = MmItem{(long long)p[0], (int)p[1], (int)p[2], (int)p[3]};
        }
        a.view_start = view_start_dev + base;
        a.out = out_dev + (size_t)base * (with_transpose ? 2 : 1) * slice;
        hipLaunchKernelGGL(match_view_kernel, dim3((unsigned)a.n), dim3(MM_BLOCK), 0, stream, a);
        VSC_CHECK_LAUNCH();
        hipLaunchKernelGGL(match_canvas_kernel, dim3((unsigned)(a.n * a.tiles * a.tiles)), dim3(MM_BLOCK), 0, stream, a);
        VSC_CHECK_LAUNCH();
    }
    return VSC_OK;
}

extern "C" int vsc_match_maps_f32(const float *sims_dev, int64_t sims_len, const int64_t *items_host, int64_t n_items, int32_t resolution,
                                  int32_t with_transpose, int32_t *view_start_dev, float *out_dev, void *stream) {
    return launch_match_maps(sims_dev, sims_len, items_host, n_items, resolution, with_transpose, view_start_dev, out_dev, (hipStream_t)stream);
}
