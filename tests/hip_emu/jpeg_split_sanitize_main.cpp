// A stand-alone program around the emulated csrc/jpeg_decode.hip + csrc/jpeg_split.hip for a host sanitizer run;
// tests/test_jpeg_split_emulated.py builds it with -fsanitize=address,undefined (tests/hip_emu_build.py: build_sanitized) and runs
// it as a child process (no sanitizer runtime is loaded into Python).  jpeg_split_emu.inc is the two emulated sources, one behind
// the other.  By hand, with the test's calls file: python tests/hip_emu_build.py jpeg_split calls.bin
// calls.bin is written by the test, int64 little endian throughout: the number of calls, then per call {n_frames, bytes_len,
// n_table_sets, out_len, scratch cap or 0, mode, sub_bytes, rounds, item_bytes, number of marker offsets, the four statistics
// expected}, the frame table [n_frames][10], per frame what is expected (0: status 0 and the expected bytes; 1: a damaged scan, the
// status vsc_jpeg_decode_u8 gives for it, which is not 0; 2: VSC_JPEG_STATUS_RESTART; 3: a flipped byte, the status
// vsc_jpeg_decode_u8 gives for it, which may be 0), the marker rows' ptr [n_frames + 1], the
// offsets (int32, padded), the table sets, the bytes and the expected output (padded to whole int64s each).  Every operand sits in
// an allocation of exactly its size, so does the kernels' scratch (common.h's hipMalloc): an access one byte outside any of them is an
// error.  Every call runs twice on one handle, over outputs pre-filled with 0x00 and with 0xFF: a frame that decodes is written
// completely and from the inputs alone, and the bytes between and around the frames' outputs keep their fill.
#include "jpeg_split_emu.inc"

static std::vector<int64_t> g_file;
static size_t g_at = 0;
static const int64_t *take(size_t bytes) {
    const int64_t *p = g_file.data() + g_at;
    g_at += (bytes + 7) / 8;
    if (g_at > g_file.size()) {
        fprintf(stderr, "calls file too short\n");
        exit(20);
    }
    return p;
}
template <class T> static T *exact(const void *src, size_t n) {      // an allocation of exactly n elements
    T *p = new T[n ? n : 1];
    if (n) memcpy(p, src, n * sizeof(T));
    return p;
}

int main(int argc, char **argv) {
    if (argc != 2) return 21;
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) return 22;
    fseek(fp, 0, SEEK_END);
    const long size = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    g_file.resize((size_t)size / 8);
    if (fread(g_file.data(), 8, g_file.size(), fp) != g_file.size()) return 23;
    fclose(fp);

    const int64_t n_calls = *take(8);
    size_t frames_run = 0, damaged = 0;
    for (int64_t c = 0; c < n_calls; ++c) {
        const int64_t *hd = take(14 * 8);
        const int64_t n = hd[0], bytes_len = hd[1], n_sets = hd[2], out_len = hd[3], cap = hd[4], n_off = hd[9];
        const int64_t *rows = take((size_t)n * 80), *expect = take((size_t)n * 8), *ptr_f = take((size_t)(n + 1) * 8);
        const int32_t *off_f = (const int32_t *)take((size_t)n_off * 4);
        const uint8_t *tables = (const uint8_t *)take((size_t)n_sets * VSC_JPEG_TABLE_SET_BYTES), *bytes = (const uint8_t *)take((size_t)bytes_len);
        const uint8_t *want = (const uint8_t *)take((size_t)out_len);
        uint8_t *b = exact<uint8_t>(bytes, (size_t)bytes_len), *t = exact<uint8_t>(tables, (size_t)n_sets * VSC_JPEG_TABLE_SET_BYTES);
        int64_t *r = exact<int64_t>(rows, (size_t)n * 10), *ptr = exact<int64_t>(ptr_f, (size_t)n + 1);
        int32_t *off = exact<int32_t>(off_f, (size_t)n_off);
        vsc_jpeg_decode *h = nullptr;
        if (vsc_jpeg_decode_create(nullptr, &h) != 0) return 1;
        if (cap && vsc_jpeg_decode_scratch(h, cap, nullptr, nullptr) != 0) return 2;
        if (vsc_jpeg_decode_split(h, (int32_t)hd[5], (int32_t)hd[6], (int32_t)hd[7], (int32_t)hd[8]) != 0) return 2;
        std::vector<uint8_t> covered((size_t)out_len, 0);
        for (int64_t i = 0; i < n; ++i)
            for (int64_t k = 0; k < rows[10 * i + 2] * rows[10 * i + 3] * 3; ++k) covered[(size_t)(rows[10 * i + 7] + k)] = expect[i] ? 2 : 1;   // 2: unspecified
        // what the one-wave entry says about these frames
        int32_t *one = new int32_t[(size_t)n];
        {
            uint8_t *out = new uint8_t[(size_t)out_len];
            if (vsc_jpeg_decode_u8(h, b, bytes_len, r, n, t, (int32_t)n_sets, out, out_len, one) != 0) return 3;
            delete[] out;
        }
        for (int fill = 0; fill < 2; ++fill) {
            uint8_t *out = new uint8_t[(size_t)out_len];
            int32_t *status = new int32_t[(size_t)n];
            memset(out, fill ? 0xFF : 0x00, (size_t)out_len);
            for (int64_t i = 0; i < n; ++i) status[i] = -1;
            if (vsc_jpeg_decode_split_u8(h, b, bytes_len, r, n, t, (int32_t)n_sets, ptr, off, out, out_len, status) != 0) return 3;
            int64_t st[4] = {-1, -1, -1, -1};
            if (vsc_jpeg_decode_stats(h, st) != 0 || st[0] != hd[10] || st[1] != hd[11] || st[2] != hd[12] || st[3] != hd[13]) {
                fprintf(stderr, "call %lld: statistics %lld %lld %lld %lld\n", (long long)c, (long long)st[0], (long long)st[1], (long long)st[2], (long long)st[3]);
                return 4;
            }
            for (int64_t i = 0; i < n; ++i) {
                const int32_t must = expect[i] == 2 ? VSC_JPEG_STATUS_RESTART : one[i];
                if (status[i] != must || (expect[i] != 3 && (expect[i] != 0) != (status[i] != 0))) {
                    fprintf(stderr, "call %lld frame %lld: status %d, one wave per frame %d\n", (long long)c, (long long)i, status[i], one[i]);
                    return 5;
                }
                if (!fill) ++frames_run, damaged += expect[i] != 0;
            }
            for (int64_t k = 0; k < out_len; ++k) {
                if (covered[(size_t)k] == 1 ? out[k] != want[k] : covered[(size_t)k] == 0 && out[k] != (fill ? 0xFF : 0x00)) {
                    fprintf(stderr, "call %lld: output byte %lld is %d\n", (long long)c, (long long)k, out[k]);
                    return 6;
                }
            }
            delete[] out;
            delete[] status;
        }
        vsc_jpeg_decode_destroy(h);
        delete[] one;
        delete[] b;
        delete[] t;
        delete[] r;
        delete[] ptr;
        delete[] off;
    }
    // the refusals: nothing is launched
    vsc_jpeg_decode *h = nullptr;
    if (vsc_jpeg_decode_create(nullptr, &h) != 0) return 7;
    const size_t launches = emu_launches();
    uint8_t bytes[16] = {0}, tables[VSC_JPEG_TABLE_SET_BYTES] = {0}, out[3] = {0x5A, 0x5A, 0x5A};
    int32_t status = 77;
    tables[1600] = 1, tables[1601] = 5, tables[512] = 1, tables[512 + 32] = 1;     // one code of length 1 in DC0 and in AC0
    const int64_t good[10] = {0, 16, 1, 1, 0, 1, 0, 0, 0, 0};                      // a 1 x 1 one-component frame, restart interval 1
    const int64_t ptr0[2] = {0, 0}, ptr1[2] = {0, 1}, ptr2[2] = {0, 2}, ptr_bad[2] = {1, 1}, ptr_back[2] = {0, -1};
    const int32_t in[2] = {3, 5}, outside[1] = {15}, negative[1] = {-1}, close[2] = {3, 4}, back[2] = {5, 3};
    if (vsc_jpeg_decode_split(nullptr, 3, 0, 0, 0) == 0 || vsc_jpeg_decode_split(h, 4, 0, 0, 0) == 0 || vsc_jpeg_decode_split(h, -1, 0, 0, 0) == 0 ||
        vsc_jpeg_decode_split(h, 3, 16, 0, 0) == 0 || vsc_jpeg_decode_split(h, 3, 66, 0, 0) == 0 || vsc_jpeg_decode_split(h, 3, 0, 129, 0) == 0 ||
        vsc_jpeg_decode_split(h, 3, 0, -1, 0) == 0 || vsc_jpeg_decode_split(h, 3, 0, 0, -1) == 0)
        return 8;
    if (vsc_jpeg_decode_split(h, 3, 64, 3, 1) != 0) return 8;
    if (vsc_jpeg_decode_split_u8(nullptr, bytes, 16, good, 1, tables, 1, ptr0, nullptr, out, 3, &status) == 0 ||
        vsc_jpeg_decode_split_u8(h, nullptr, 16, good, 1, tables, 1, ptr0, nullptr, out, 3, &status) == 0 ||
        vsc_jpeg_decode_split_u8(h, bytes, 16, good, 1, tables, 1, ptr0, nullptr, nullptr, 3, &status) == 0 ||
        vsc_jpeg_decode_split_u8(h, bytes, 16, good, 1, tables, 1, ptr0, nullptr, out, 3, nullptr) == 0 ||
        vsc_jpeg_decode_split_u8(h, bytes, 16, good, 1, tables, 1, ptr1, nullptr, out, 3, &status) == 0 ||
        vsc_jpeg_decode_split_u8(h, bytes, 16, good, 1, tables, 1, ptr_bad, in, out, 3, &status) == 0 ||
        vsc_jpeg_decode_split_u8(h, bytes, 16, good, 1, tables, 1, ptr_back, in, out, 3, &status) == 0 ||
        vsc_jpeg_decode_split_u8(h, bytes, 16, good, 1, tables, 1, ptr1, outside, out, 3, &status) == 0 ||
        vsc_jpeg_decode_split_u8(h, bytes, 16, good, 1, tables, 1, ptr1, negative, out, 3, &status) == 0 ||
        vsc_jpeg_decode_split_u8(h, bytes, 16, good, 1, tables, 1, ptr2, close, out, 3, &status) == 0 ||
        vsc_jpeg_decode_split_u8(h, bytes, 16, good, 1, tables, 1, ptr2, back, out, 3, &status) == 0 ||
        vsc_jpeg_decode_split_u8(h, bytes, 16, good, -1, tables, 1, ptr0, nullptr, out, 3, &status) == 0)
        return 9;
    int64_t st[4];
    if (vsc_jpeg_decode_stats(h, nullptr) == 0 || vsc_jpeg_decode_stats(nullptr, st) == 0) return 10;
    if (vsc_jpeg_decode_split_u8(h, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr) != 0) return 12;
    if (vsc_jpeg_decode_stats(h, st) != 0 || st[0] || st[1] || st[2] || st[3]) return 12;
    if (emu_launches() != launches || status != 77 || out[0] != 0x5A || out[1] != 0x5A || out[2] != 0x5A) return 13;
    // sixteen zero bytes: a 1 x 1 frame; two offsets where none are expected: taken as unsplit
    if (vsc_jpeg_decode_split_u8(h, bytes, 16, good, 1, tables, 1, ptr2, in, out, 3, &status) != 0 || status != 0) return 14;
    if (vsc_jpeg_decode_stats(h, st) != 0 || st[0] != 0 || st[1] != 0 || st[2] != 1 || st[3] != 1) return 15;
    if (vsc_jpeg_decode_split_u8(h, bytes, 16, good, 1, tables, 1, nullptr, nullptr, out, 3, &status) != 0 || status != 0) return 16;
    if (vsc_jpeg_decode_stats(h, st) != 0 || st[0] != 1 || st[3] != 1) return 17;
    vsc_jpeg_decode_destroy(h);
    printf("jpeg_split emulated under the sanitizers: ok (%lld calls, %zu frames, %zu of them damaged, %zu launches)\n", (long long)n_calls, frames_run, damaged,
           emu_launches());
    return 0;
}
