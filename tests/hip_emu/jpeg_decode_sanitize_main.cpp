// A stand-alone program around the emulated csrc/jpeg_decode.hip for a host sanitizer run; tests/test_jpeg_decode_emulated.py builds
// it with -fsanitize=address,undefined (tests/hip_emu_build.py: build_sanitized; jpeg_decode_emu.inc is the emulated source) and
// runs it as a child process: no sanitizer runtime is loaded into Python.  By hand, with the test's calls file:
//   python tests/hip_emu_build.py jpeg_decode calls.bin
// calls.bin is written by the test from tests/jpeg_decode_cases.py (the files are made by Pillow's encoder at test time), int64
// little endian throughout: the number of calls, then per call {n_frames, bytes_len, n_table_sets, out_len, scratch cap or 0,
// chunks expected or 0}, the frame table [n_frames][10], per frame 0 (must decode: status 0 and the expected bytes) or 1 (a damaged
// scan: status not 0), the table sets, the bytes and the expected output (padded to whole int64s each).  Every operand sits in an
// allocation of exactly its size, so does the kernels' scratch (common.h's hipMalloc): an access one byte outside any of them is an error.
// Every call runs over outputs pre-filled with 0x00 and with 0xFF: a frame that decodes is written completely and from the inputs
// alone, and the bytes between and around the frames' outputs keep their fill (a damaged frame's own output is unspecified).
#include "jpeg_decode_emu.inc"

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
        const int64_t *hd = take(48);
        const int64_t n = hd[0], bytes_len = hd[1], n_sets = hd[2], out_len = hd[3], cap = hd[4], chunks = hd[5];
        const int64_t *rows = take((size_t)n * 80), *expect = take((size_t)n * 8);
        const uint8_t *tables = (const uint8_t *)take((size_t)n_sets * VSC_JPEG_TABLE_SET_BYTES), *bytes = (const uint8_t *)take((size_t)bytes_len);
        const uint8_t *want = (const uint8_t *)take((size_t)out_len);
        // exactly sized copies: the file's arrays have neighbours
        uint8_t *b = new uint8_t[(size_t)bytes_len], *t = new uint8_t[(size_t)n_sets * VSC_JPEG_TABLE_SET_BYTES];
        int64_t *r = new int64_t[(size_t)n * 10];
        memcpy(b, bytes, (size_t)bytes_len), memcpy(t, tables, (size_t)n_sets * VSC_JPEG_TABLE_SET_BYTES), memcpy(r, rows, (size_t)n * 80);
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
            if (vsc_jpeg_decode_u8(h, b, bytes_len, r, n, t, (int32_t)n_sets, out, out_len, status) != 0) return 3;
            int64_t got_chunks = -1;
            if (vsc_jpeg_decode_scratch(h, 0, &got_chunks, nullptr) != 0 || (chunks && got_chunks != chunks)) return 4;
            for (int64_t i = 0; i < n; ++i) {
                if (expect[i] ? status[i] == 0 || status[i] == -1 : status[i] != 0) {
                    fprintf(stderr, "call %lld frame %lld: status %d\n", (long long)c, (long long)i, status[i]);
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
    }
    // the refusals: nothing is launched
    vsc_jpeg_decode *h = nullptr;
    if (vsc_jpeg_decode_create(nullptr, &h) != 0 || vsc_jpeg_decode_create(nullptr, nullptr) == 0) return 7;
    const size_t launches = emu_launches();
    uint8_t bytes[16] = {0}, tables[VSC_JPEG_TABLE_SET_BYTES] = {0}, out[3] = {0x5A, 0x5A, 0x5A};
    int32_t status = 77;
    tables[1600] = 1, tables[1601] = 5, tables[512] = 1, tables[512 + 32] = 1;     // one code of length 1 in DC0 and in AC0
    const int64_t good[10] = {0, 16, 1, 1, 0, 0, 0, 0, 0, 0};
    const int64_t bad[][10] = {{1, 16, 1, 1, 0, 0, 0, 0, 0, 0}, {0, 16, 0, 1, 0, 0, 0, 0, 0, 0},     {0, 16, 1, 16385, 0, 0, 0, 0, 0, 0}, {0, 16, 1, 1, 4, 0, 0, 0, 0, 0},
                               {0, 16, 1, 1, 0, 0, 1, 0, 0, 0}, {0, 16, 1, 1, 0, 0, 0, 1, 0, 0},     {0, 16, 1, 1, 0, 0, 0, 0, 1, 0},     {0, 16, 1, 1, 0, 0, 0, 0, 4, 0},
                               {0, 16, 1, 1, 0, 0, 0, 0, 8, 0}, {-1, 16, 1, 1, 0, 0, 0, 0, 0, 0},    {0, 16, 1, 1, 0, -1, 0, 0, 0, 0}};
    for (const auto &r : bad)
        if (vsc_jpeg_decode_u8(h, bytes, 16, r, 1, tables, 1, out, 3, &status) == 0) return 8;
    if (vsc_jpeg_decode_u8(nullptr, bytes, 16, good, 1, tables, 1, out, 3, &status) == 0) return 9;
    if (vsc_jpeg_decode_u8(h, nullptr, 16, good, 1, tables, 1, out, 3, &status) == 0 || vsc_jpeg_decode_u8(h, bytes, 16, good, 1, tables, 1, nullptr, 3, &status) == 0 ||
        vsc_jpeg_decode_u8(h, bytes, 16, good, 1, tables, 1, out, 3, nullptr) == 0 || vsc_jpeg_decode_u8(h, bytes, 16, good, -1, tables, 1, out, 3, &status) == 0)
        return 10;
    tables[512] = 3;                                                                // three codes of length 1: no prefix code
    if (vsc_jpeg_decode_u8(h, bytes, 16, good, 1, tables, 1, out, 3, &status) == 0) return 11;
    if (vsc_jpeg_decode_u8(h, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr) != 0) return 12;
    if (emu_launches() != launches || status != 77 || out[0] != 0x5A || out[1] != 0x5A || out[2] != 0x5A) return 13;
    tables[512] = 1;
    if (vsc_jpeg_decode_u8(h, bytes, 16, good, 1, tables, 1, out, 3, &status) != 0 || status != 0) return 14;     // sixteen zero bytes: a 1 x 1 gray frame
    vsc_jpeg_decode_destroy(h);
    printf("jpeg_decode emulated under the sanitizers: ok (%lld calls, %zu frames, %zu of them damaged, %zu launches)\n", (long long)n_calls, frames_run, damaged,
           emu_launches());
    return 0;
}
