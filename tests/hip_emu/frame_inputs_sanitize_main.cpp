// A stand-alone program around the emulated csrc/frame_inputs.hip for a host sanitizer run (it is no part of the test suite):
//   python tests/hip_emu_build.py frame_inputs [-DFI_EMU_LDS_BYTES=4096 | -DFI_EMU_LDS_BYTES=8]
// builds it with -fsanitize=address,undefined (frame_inputs_emu.inc is the emulated source) and runs it.
// Seeded frames and every output in exactly sized allocations (an access one byte outside any operand is an error; the staging
// loads round down to dwords, so the frames' first and last bytes are what they must not step over), downscales, upscales, an
// identity, windows at odd byte offsets, more than one tile of output columns, the vertical-first shape, then the refusals.  It
// checks only what needs no second implementation: an identity resize returns its input, and every call gives the same bytes over
// outputs pre-filled with 0x00 and with 0xFF (every byte is written, from the inputs alone).
#include "frame_inputs_emu.inc"

static uint32_t g_seed = 12345u;
static uint8_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return (uint8_t)(g_seed >> 24); }

struct Shape { int n, h, w; std::vector<int32_t> targets; };

int main() {
    const Shape shapes[] = {
        {2, 37, 53, {0, 37, 0, 53, 17, 17, 0, 0, 17, 17, 0, 37, 0, 53, 24, 34, 0, 5, 24, 24, 3, 30, 5, 40, 17, 17, 0, 0, 17, 17}},
        {3, 9, 31, {0, 9, 0, 31, 24, 82, 0, 29, 24, 24}},
        {1, 24, 24, {0, 24, 0, 24, 24, 24, 0, 0, 24, 24}},
        {2, 1, 1, {0, 1, 0, 1, 4, 4, 0, 0, 4, 4}},
        {1, 1, 5, {0, 1, 0, 5, 3, 15, 0, 6, 3, 3}},
        {2, 200, 7, {0, 200, 0, 7, 16, 16, 0, 0, 16, 16}},
        {2, 203, 2, {0, 203, 0, 2, 8, 8, 0, 0, 8, 8}},
        {2, 64, 48, {0, 64, 0, 48, 31, 29, 3, 2, 23, 19}},
        {2, 20, 150, {0, 20, 0, 150, 12, 99, 0, 0, 12, 99, 0, 20, 0, 150, 12, 140, 1, 3, 10, 131}},
    };
    vsc_frame_inputs *h = nullptr;
    if (vsc_frame_inputs_create(nullptr, &h) != 0) return 1;
    size_t calls = 0;
    for (const Shape &s : shapes) {
        const size_t fbytes = (size_t)s.n * s.h * s.w * 3;
        uint8_t *frames = new uint8_t[fbytes];
        for (size_t i = 0; i < fbytes; ++i) frames[i] = rnd();
        const int nt = (int)s.targets.size() / 10;
        std::vector<uint8_t *> outs[2];
        for (int fill = 0; fill < 2; ++fill) {
            for (int t = 0; t < nt; ++t) {
                const size_t bytes = (size_t)s.n * s.targets[10 * t + 8] * s.targets[10 * t + 9] * 3;
                outs[fill].push_back(new uint8_t[bytes]);
                memset(outs[fill].back(), fill ? 0xFF : 0x00, bytes);
            }
            if (vsc_frame_inputs_u8(h, frames, s.n, s.h, s.w, s.targets.data(), nt, outs[fill].data()) != 0) return 2;
            ++calls;
        }
        for (int t = 0; t < nt; ++t) {
            const int32_t *g = s.targets.data() + 10 * t;
            const size_t bytes = (size_t)s.n * g[8] * g[9] * 3;
            if (memcmp(outs[0][t], outs[1][t], bytes) != 0) return 3;
            if (g[4] == s.h && g[5] == s.w && g[8] == s.h && g[9] == s.w && g[1] - g[0] == s.h && g[3] - g[2] == s.w && memcmp(outs[0][t], frames, bytes) != 0) return 4;
            delete[] outs[0][t];
            delete[] outs[1][t];
        }
        delete[] frames;
    }
    uint8_t frame[37 * 53 * 3] = {0}, out[17 * 17 * 3];
    memset(out, 0x5A, sizeof out);
    uint8_t *outp[1] = {out}, *nullp[1] = {nullptr};
    const int32_t good[10] = {0, 37, 0, 53, 17, 17, 0, 0, 17, 17};
    const int32_t bad[][10] = {{0, 38, 0, 53, 17, 17, 0, 0, 17, 17}, {0, 37, 5, 5, 17, 17, 0, 0, 17, 17}, {0, 37, 0, 53, 4097, 17, 0, 0, 17, 17},
                               {0, 37, 0, 53, 17, 0, 0, 0, 17, 0}, {0, 37, 0, 53, 17, 17, 1, 0, 17, 17}, {0, 37, 0, 53, 17, 17, 0, -1, 17, 17}};
    for (const auto &b : bad)
        if (vsc_frame_inputs_u8(h, frame, 1, 37, 53, b, 1, outp) == 0) return 5;
    if (vsc_frame_inputs_u8(nullptr, frame, 1, 37, 53, good, 1, outp) == 0) return 6;
    if (vsc_frame_inputs_u8(h, frame, -1, 37, 53, good, 1, outp) == 0) return 7;
    if (vsc_frame_inputs_u8(h, frame, 1, 37, 53, good, 1, nullp) == 0) return 8;
    if (vsc_frame_inputs_u8(h, nullptr, 1, 37, 53, good, 1, outp) == 0) return 9;
    for (size_t i = 0; i < sizeof out; ++i)
        if (out[i] != 0x5A) return 10;
    if (vsc_frame_inputs_u8(h, frame, 0, 37, 53, good, 1, outp) != 0 || vsc_frame_inputs_u8(h, frame, 1, 37, 53, nullptr, 0, nullptr) != 0) return 11;
    if (vsc_frame_inputs_u8(h, frame, 1, 37, 53, good, 1, outp) != 0) return 12;
    vsc_frame_inputs_destroy(h);
    printf("frame_inputs emulated under the sanitizers: ok (%zu calls, %zu launches, LDS budget %d)\n", calls, emu_launches(), (int)VSC_FRAME_INPUTS_LDS_BYTES);
    return 0;
}
