// A stand-alone program around the emulated csrc/jpeg_decode.hip + csrc/jpeg_scans.hip for a host sanitizer run;
// tests/test_jpeg_scans_emulated.py builds it with -fsanitize=address,undefined (tests/hip_emu_build.py: build_sanitized;
// jpeg_scans_emu.inc is the emulated source) and runs it as a child process: no sanitizer runtime is loaded into Python.
// calls.bin is written by the test from tests/jpeg_scans_cases.py, int64 little endian throughout: the number of calls, then per
// call {n_frames, bytes_len, n_table_sets, out_len, scratch cap or 0, chunks expected or 0, n_scans}, the frame table
// [n_frames][10], the scan table [n_scans][10], the scan pointers [n_frames + 1], per frame the status expected (0: must decode
// to the expected bytes), the table sets, the bytes and the expected output (padded to whole int64s each).  Every operand sits in
// an allocation of exactly its size, so does the kernels' scratch -- pixel planes and coefficient planes -- (common.h's hipMalloc):
// an access one byte outside any of them is an error.  Every call runs over outputs pre-filled with 0x00 and with 0xFF: a frame
// that decodes is written completely and from the inputs alone, and the bytes between and around the frames' outputs keep their
// fill (a damaged frame's own output is unspecified).
#include "jpeg_scans_emu.inc"

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

template <class T> static T *exact(const void *src, size_t count) {
    T *p = new T[count ? count : 1];
    memcpy(p, src, count * sizeof(T));
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
        const int64_t *hd = take(56);
        const int64_t n = hd[0], bytes_len = hd[1], n_sets = hd[2], out_len = hd[3], cap = hd[4], chunks = hd[5], n_scans = hd[6];
        const int64_t *rows = take((size_t)n * 80), *srows = take((size_t)n_scans * 80), *ptr = take((size_t)(n + 1) * 8), *expect = take((size_t)n * 8);
        const uint8_t *tables = (const uint8_t *)take((size_t)n_sets * VSC_JPEG_SCAN_TABLE_SET_BYTES), *bytes = (const uint8_t *)take((size_t)bytes_len);
        const uint8_t *want = (const uint8_t *)take((size_t)out_len);
        // exactly sized copies: the file's arrays have neighbours
        uint8_t *b = exact<uint8_t>(bytes, (size_t)bytes_len), *t = exact<uint8_t>(tables, (size_t)n_sets * VSC_JPEG_SCAN_TABLE_SET_BYTES);
        int64_t *r = exact<int64_t>(rows, (size_t)n * 10), *s = exact<int64_t>(srows, (size_t)n_scans * 10), *p = exact<int64_t>(ptr, (size_t)n + 1);
        vsc_jpeg_decode *h = nullptr;
        if (vsc_jpeg_decode_create(nullptr, &h) != 0) return 1;
        if (cap && vsc_jpeg_decode_scratch(h, cap, nullptr, nullptr) != 0) return 2;
        std::vector<uint8_t> covered((size_t)out_len, 0);
        for (int64_t i = 0; i < n; ++i)
            for (int64_t k = 0; k < rows[10 * i + 2] * rows[10 * i + 3] * 3; ++k) covered[(size_t)(rows[10 * i + 7] + k)] = expect[i] ? 2 : 1;   // 2: unspecified
        for (int fill = 0; fill < 2; ++fill) {
            uint8_t *out = new uint8_t[(size_t)out_len];
            int32_t *status = new int32_t[(size_t)n];
            memset(out, fill ? 0xFF : 0x00, (size_t)out_len);
            for (int64_t i = 0; i < n; ++i) status[i] = -1;
            if (vsc_jpeg_decode_scans_u8(h, b, bytes_len, r, n, s, p, t, (int32_t)n_sets, out, out_len, status) != 0) return 3;
            int64_t got_chunks = -1;
            if (vsc_jpeg_decode_scratch(h, 0, &got_chunks, nullptr) != 0 || (chunks && got_chunks != chunks)) return 4;
            for (int64_t i = 0; i < n; ++i) {
                if (status[i] != expect[i]) {
                    fprintf(stderr, "call %lld frame %lld: status %d, expected %lld\n", (long long)c, (long long)i, status[i], (long long)expect[i]);
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
        delete[] b;
        delete[] t;
        delete[] r;
        delete[] s;
        delete[] p;
    }
    // the refusals: nothing is launched
    vsc_jpeg_decode *h = nullptr;
    if (vsc_jpeg_decode_create(nullptr, &h) != 0) return 7;
    const size_t launches = emu_launches();
    uint8_t bytes[16] = {0}, tables[VSC_JPEG_SCAN_TABLE_SET_BYTES] = {0}, out[3] = {0x5A, 0x5A, 0x5A};
    int32_t status = 77;
    tables[2688] = 1, tables[2689] = 0x11, tables[512] = 1, tables[512 + 64] = 1;     // one code of length 1 in DC0 and in AC0
    const int64_t frame[10] = {0, 0, 1, 1, 0, 0, 0, 0, 0, 0}, ptr[2] = {0, 1}, ptr2[3] = {0, 2};
    const int64_t good[10] = {0, 16, 1, 0, 63, 0, 0, 0, 0, 0};
    const int64_t bad[][10] = {{1, 16, 1, 0, 63, 0, 0, 0, 0, 0},  {0, 16, 2, 0, 63, 0, 0, 0, 0, 0}, {0, 16, 1, 0, 62, 0, 0, 0, 0, 0}, {0, 16, 1, 0, 63, 0, 1, 0, 0, 0},
                               {0, 16, 1, 0, 63, 0, 0, -1, 0, 0}, {0, 16, 1, 0, 63, 0, 0, 0, 1, 0}, {0, 16, 1, 0, 63, 0, 0, 0, 0, 1}, {0, 16, 1, 0, 63, 0, 0, 0, 0, 4},
                               {0, 16, 1, 1, 63, 0, 0, 0, 0, 0},  {0, 16, 1, 0, 0, 0, 0, 0, 0, 0},  {0, 16, 1, 0, 0, 1, 0, 0, 0, 0},  {-1, 16, 1, 0, 63, 0, 0, 0, 0, 0}};
    for (const auto &r : bad)
        if (vsc_jpeg_decode_scans_u8(h, bytes, 16, frame, 1, r, ptr, tables, 1, out, 3, &status) == 0) return 8;
    int64_t twice[20];
    memcpy(twice, good, 80), memcpy(twice + 10, good, 80);                             // the same scan sent twice
    if (vsc_jpeg_decode_scans_u8(h, bytes, 16, frame, 1, twice, ptr2, tables, 1, out, 3, &status) == 0) return 9;
    if (vsc_jpeg_decode_scans_u8(nullptr, bytes, 16, frame, 1, good, ptr, tables, 1, out, 3, &status) == 0 ||
        vsc_jpeg_decode_scans_u8(h, nullptr, 16, frame, 1, good, ptr, tables, 1, out, 3, &status) == 0 ||
        vsc_jpeg_decode_scans_u8(h, bytes, 16, frame, 1, nullptr, ptr, tables, 1, out, 3, &status) == 0 ||
        vsc_jpeg_decode_scans_u8(h, bytes, 16, frame, 1, good, nullptr, tables, 1, out, 3, &status) == 0 ||
        vsc_jpeg_decode_scans_u8(h, bytes, 16, frame, 1, good, ptr, tables, 1, out, 3, nullptr) == 0 ||
        vsc_jpeg_decode_scans_u8(h, bytes, 16, frame, -1, good, ptr, tables, 1, out, 3, &status) == 0 ||
        vsc_jpeg_decode_scans_u8(h, bytes, 16, frame, 1, good, ptr, tables, 1, out, 2, &status) == 0)
        return 10;
    tables[512] = 3;                                                                   // three codes of length 1: no prefix code
    if (vsc_jpeg_decode_scans_u8(h, bytes, 16, frame, 1, good, ptr, tables, 1, out, 3, &status) == 0) return 11;
    if (vsc_jpeg_decode_scans_u8(h, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr) != 0) return 12;
    if (emu_launches() != launches || status != 77 || out[0] != 0x5A || out[1] != 0x5A || out[2] != 0x5A) return 13;
    tables[512] = 1;
    if (vsc_jpeg_decode_scans_u8(h, bytes, 16, frame, 1, good, ptr, tables, 1, out, 3, &status) != 0 || status != 0) return 14;     // sixteen zero bytes: a 1 x 1 gray frame
    vsc_jpeg_decode_destroy(h);
    printf("jpeg_scans emulated under the sanitizers: ok (%lld calls, %zu frames, %zu of them damaged, %zu launches)\n", (long long)n_calls, frames_run, damaged,
           emu_launches());
    return 0;
}
