// Greedy near-duplicate frame filter of the query ensemble (VSC22-Descriptor-Track-1st/infer/extract_query_feats.py:190-199) over the
// frame x frame matrices of vsc_pair_similarity_f32, which never leave the device.  The contract is stated with vsc_frame_filter_f32
// in include/vsc_hip.h (executable form: tests/frame_filter_contract.py).
//
// One kernel, one workgroup per video, one argument structure and a 1-D grid (which is also what lets the file run on the CPU
// against tests/hip_emu/common.h).  A chunk's item table travels in that structure, so the entry uploads nothing and never waits
// for the stream.  Four phases, separated by workgroup barriers:
//  (1) columns: thread = column j, rows ascending.  One coalesced read of the matrix; the column's fp32 add chain in the stated
//      order (the first row is copied, not added to zero); per row one ballot of v > thr, stored as word j / 64 of row i of the
//      adjacency bit matrix.  The bit matrix lives in LDS while it fits beside mean[] and order[], otherwise in a slice of the
//      search path's grow-only scratch; the kernel reaches either through one generic pointer.
//  (2) rank: position of i in the visit order = number of j with mean[j] > mean[i], or equal and j > i.  A count, not a sort.
//  (3) walk, one wave: lane w holds word w of the `removed` set (rows <= 4096 = 64 lanes x 64 bits).  Per visited i one LDS read,
//      one shuffle, one bit test; row i's words are ORed in only when i survives.
//  (4) compaction: popcount prefix over the 64 words, then every thread places its own column (or the -1 of the tail).
// The bound is latency: phase 3 is a chain of `rows` dependent steps on one wave (an LDS or L2 read each), and phase 1 reads
// 4 rows^2 bytes once -- 13 MB for 1 800 rows, microseconds of HBM time.  No atomics: the output is a pure function of the input.
#include "common.h"

// contract arithmetic: a pure add chain and one correctly rounded division; nothing may be contracted or reassociated
#pragma clang fp contract(off)

namespace {

constexpr int FF_BLOCK = 512;
constexpr int FF_MAX_ROWS = VSC_FRAME_FILTER_MAX_ROWS;   // one 64-bit word of the removed set per lane
constexpr int FF_CHUNK = VSC_FRAME_FILTER_CHUNK;         // items per launch: 128 x 24 bytes of kernel arguments (limit 4 KiB)
constexpr int FF_LDS_MAX = VSC_FRAME_FILTER_LDS_BYTES;   // dynamic LDS a workgroup may ask for (1 KiB left to the static arrays below)
static_assert(FF_MAX_ROWS <= 64 * 64 && FF_CHUNK * 24 + 64 <= 4096 && FF_LDS_MAX <= 160 * 1024 - 1024 && 8 * FF_MAX_ROWS <= 160 * 1024 - 1024,
              "include/vsc_hip.h states limits the kernel cannot hold");

struct FfItem {
    long long off;                            // element offset of the matrix
    long long bits;                           // offset of the bit matrix in the scratch, in 64-bit words; -1: LDS
    int rows, out;                            // rows; prefix sum of rows = start of the item's output slices
};

struct FfArgs {
    const float *sims;
    unsigned long long *scratch;
    float thr;
    int32_t *kept, *counts;                   // kept: whole call; counts: of this chunk
    float *means;                             // whole call, or null
    int32_t *order;                           // whole call, or null
    FfItem it[FF_CHUNK];
};

__host__ __device__ inline long long ff_words(long long rows) { return (rows + 63) >> 6; }
// bytes of dynamic LDS of an item whose bit matrix is in LDS (mean[], order[], bits[][]), and without it
__host__ __device__ inline long long ff_lds_bytes(long long rows, bool bits_in_lds) {
    return 8 * rows + (bits_in_lds ? 8 * rows * ff_words(rows) : 0);
}

__global__ __launch_bounds__(FF_BLOCK) void frame_filter_kernel(FfArgs a) {
    extern __shared__ __align__(16) unsigned char ff_smem[];
    __shared__ unsigned long long s_keep[64];
    __shared__ int s_prefix[65];

    const FfItem it = a.it[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = it.rows, W = (L + 63) >> 6;
    if (L == 0) {
        if (tid == 0) a.counts[blockIdx.x] = 0;
        return;
    }
    float *mean = (float *)ff_smem;                                   // [L]
    int *order = (int *)(ff_smem + (size_t)L * 4);                    // [L]
    unsigned long long *bits = it.bits < 0 ? (unsigned long long *)(ff_smem + (size_t)L * 8) : a.scratch + it.bits;   // [L][W]
    const float *s = a.sims + it.off;
    const float thr = a.thr;

    // (1) column chains and the adjacency bits.  A wave owns 64 consecutive columns = one word of every row.
    for (int j0 = wave * 64; j0 < L; j0 += FF_BLOCK) {
        const int j = j0 + lane;
        const bool valid = j < L;
        const float *col = s + (valid ? j : 0);
        float acc = 0.f;
        for (int i = 0; i < L; ++i) {
            float v = col[(size_t)i * L];
            if (i == j) v = v - 1.0f;
            acc = i == 0 ? v : acc + v;
            const unsigned long long b = __ballot(valid && v > thr);
            if (lane == 0) bits[(size_t)i * W + (j0 >> 6)] = b;
        }
        if (valid) {
            mean[j] = acc / (float)L;
            order[j] = 0;            // every slot holds a row number even if NaN means (outside the contract) leave ranks unused
        }
    }
    __threadfence_block();
    __syncthreads();

    // (2) visit position by counting
    for (int i = tid; i < L; i += FF_BLOCK) {
        const float mi = mean[i];
        int r = 0;
        for (int j = 0; j < L; ++j) {
            const float mj = mean[j];
            r += (mj > mi || (mj == mi && j > i)) ? 1 : 0;
        }
        order[r] = i;
        if (a.means) a.means[it.out + i] = mi;
    }
    __syncthreads();
    if (a.order)
        for (int t = tid; t < L; t += FF_BLOCK) a.order[it.out + t] = order[t];

    // (3) the greedy walk on one wave
    if (wave == 0) {
        unsigned long long removed = 0ull;
        for (int t = 0; t < L; ++t) {
            const int i = order[t];
            const unsigned long long word = __shfl(removed, i >> 6, 64);
            if (!((word >> (i & 63)) & 1ull) && lane < W) removed |= bits[(size_t)i * W + lane];
        }
        unsigned long long keep = 0ull;
        if (lane < W) {
            const int left = L - lane * 64;
            keep = ~removed & (left >= 64 ? ~0ull : (1ull << left) - 1ull);
        }
        int incl = __popcll(keep);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        s_keep[lane] = keep;
        s_prefix[lane + 1] = incl;
        if (lane == 0) s_prefix[0] = 0;
    }
    __syncthreads();

    // (4) kept rows ascending, then the -1 tail
    const int total = s_prefix[64];
    int32_t *out = a.kept + it.out;
    for (int j = tid; j < L; j += FF_BLOCK) {
        const unsigned long long keep = s_keep[j >> 6];
        if ((keep >> (j & 63)) & 1ull) out[s_prefix[j >> 6] + __popcll(keep & ((1ull << (j & 63)) - 1ull))] = j;
        if (j >= total) out[j] = -1;
    }
    if (tid == 0) a.counts[blockIdx.x] = total;
}

}  // namespace

int launch_frame_filter(const float *sims_dev, int64_t sims_len, const int64_t *items_host, int64_t n_items, float threshold,
                        int32_t *kept_dev, int32_t *counts_dev, float *means_dev, int32_t *order_dev, hipStream_t stream) {
    VSC_REQUIRE(n_items >= 0 && n_items < (1ll << 31) && sims_len >= 0, "frame_filter: %lld items, %lld similarities", (long long)n_items,
                (long long)sims_len);
    VSC_REQUIRE(threshold - threshold == 0.f, "frame_filter: the threshold is not finite");
    if (n_items == 0) return VSC_OK;
    VSC_REQUIRE(items_host && counts_dev, "frame_filter: null pointer");
    long long total_rows = 0, scratch_words = 0;
    for (int64_t i = 0; i < n_items; ++i) {
        const int64_t off = items_host[2 * i], rows = items_host[2 * i + 1];
        VSC_REQUIRE(rows >= 0 && rows <= FF_MAX_ROWS, "frame_filter: item %lld has %lld rows (limit %d)", (long long)i, (long long)rows, FF_MAX_ROWS);
        VSC_REQUIRE(off >= 0 && off <= sims_len && rows * rows <= sims_len - off && (rows == 0 || sims_dev),
                    "frame_filter: item %lld = (%lld, %lld) outside the %lld similarities", (long long)i, (long long)off, (long long)rows,
                    (long long)sims_len);
        total_rows += rows;
        if (ff_lds_bytes(rows, true) > FF_LDS_MAX) scratch_words += (rows * ff_words(rows) + 15) & ~15ll;   // 128-byte slices
    }
    VSC_REQUIRE(total_rows < (1ll << 31), "frame_filter: %lld rows in one call (limit 2^31 - 1)", total_rows);
    VSC_REQUIRE(total_rows == 0 || kept_dev, "frame_filter: null pointer");
    void *scratch = nullptr;
    if (scratch_words) VSC_TRY(search_scratch_get(SCRATCH_FRAME_FILTER_BITS, (size_t)scratch_words * 8, &scratch));
    FfArgs a;
    a.sims = sims_dev, a.scratch = (unsigned long long *)scratch, a.thr = threshold;
    a.kept = kept_dev, a.means = means_dev, a.order = order_dev;
    long long out = 0, word = 0;
    for (int64_t base = 0; base < n_items; base += FF_CHUNK) {
        const int n = (int)(n_items - base < FF_CHUNK ? n_items - base : FF_CHUNK);
        long long lds = 0;
        for (int i = 0; i < FF_CHUNK; ++i) {
            if (i >= n) {
                a.it[i] = FfItem{0, -1, 0, 0};
                continue;
            }
            const long long rows = items_host[2 * (base + i) + 1];
            const bool in_lds = ff_lds_bytes(rows, true) <= FF_LDS_MAX;
            a.it[i] = FfItem{(long long)items_host[2 * (base + i)], in_lds ? -1 : word, (int)rows, (int)out};
            out += rows;
            if (!in_lds) word += (rows * ff_words(rows) + 15) & ~15ll;
            const long long need = ff_lds_bytes(rows, in_lds);
            lds = need > lds ? need : lds;
        }
        a.counts = counts_dev + base;
        VSC_TRY(vsc_allow_dynamic_lds(frame_filter_kernel, (int)lds));
        hipLaunchKernelGGL(frame_filter_kernel, dim3((unsigned)n), dim3(FF_BLOCK), (size_t)lds, stream, a);
        VSC_CHECK_LAUNCH();
    }
    return VSC_OK;
}

struct vsc_frame_filter {
    hipStream_t stream;
};

extern "C" int vsc_frame_filter_create(void *stream, vsc_frame_filter **out) {
    VSC_REQUIRE(out, "frame_filter_create: null pointer");
    *out = new vsc_frame_filter{(hipStream_t)stream};
    return VSC_OK;
}

extern "C" void vsc_frame_filter_destroy(vsc_frame_filter *h) { delete h; }

extern "C" int vsc_frame_filter_f32(vsc_frame_filter *h, const float *sims_dev, int64_t sims_len, const int64_t *items_host, int64_t n_items,
                                    float threshold, int32_t *kept_dev, int32_t *counts_dev, float *means_dev, int32_t *order_dev) {
    VSC_REQUIRE(h, "frame_filter: null handle");
    return launch_frame_filter(sims_dev, sims_len, items_host, n_items, threshold, kept_dev, counts_dev, means_dev, order_dev, h->stream);
}
