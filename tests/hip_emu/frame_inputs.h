// What csrc/frame_inputs.hip needs beyond tests/hip_emu/common.h (which stays as it is), for tests/test_frame_inputs_emulated.py and
// frame_inputs_sanitize_main.cpp only: the header's constants, the kernel's dynamic LDS as a static buffer of the device's size, the
// two-pass path's scratch slot as a buffer of its own that is filled with 0xFF when fresh, and the coefficient cache of
// csrc/resample_coeffs.h (the same builder, compiled here for the host; "device" tables are host memory).  A test build may lower
// the LDS budget (-DFI_EMU_LDS_BYTES) so that every target takes the two-pass path.  Build with -I <csrc>.
#pragma once
#include "common.h"

#include <map>
#include <utility>

#include "resample_coeffs.h"
#define VSC_FRAME_INPUTS_MAX_SIDE 4096
#ifndef FI_EMU_LDS_BYTES
#define FI_EMU_LDS_BYTES (160 * 1024)
#endif
#define VSC_FRAME_INPUTS_LDS_BYTES FI_EMU_LDS_BYTES
enum { SCRATCH_VIEW_RESIZE = 0 };
alignas(16) static unsigned char fi_smem[163840];
static size_t g_fi_scratch_bytes = 0, g_fi_launches = 0, g_fi_blocks = 0, g_fi_tables = 0;
static inline int fi_emu_scratch_get(int, size_t bytes, void **out) {
    static void *p = nullptr;
    if (bytes > g_fi_scratch_bytes) {
        free(p);
        p = malloc(bytes);
        memset(p, 0xFF, bytes);
        g_fi_scratch_bytes = bytes;
    }
    *out = p;
    return 0;
}
#define search_scratch_get fi_emu_scratch_get
int resample_coeffs_get(const char *, int in, int out, ResampleCoeffs *res) {
    static std::map<std::pair<int, int>, std::pair<std::vector<int32_t>, int>> cache;     // (table, ksize); a map's nodes do not move
    auto key = std::make_pair(in, out);
    auto it = cache.find(key);
    if (it == cache.end()) {
        int ksize = 0;
        std::vector<int32_t> table = resample_coeffs(in, out, &ksize);
        it = cache.emplace(key, std::make_pair(std::move(table), ksize)).first;
        ++g_fi_tables;
    }
    res->dev = it->second.first.data(), res->host = it->second.first.data(), res->ksize = it->second.second;
    return 0;
}
// launches and workgroups are counted: the tests tell the fused path from the two-pass path, and one band from several, by them
template <class K, class A> static inline void fi_emu_launch(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t s, A a) {
    ++g_fi_launches;
    g_fi_blocks += grid.x;
    if (lds > (size_t)FI_EMU_LDS_BYTES || block.x > (unsigned)EMU_BLOCK) {
        fprintf(stderr, "frame_inputs emulation: a launch asks for %zu bytes of LDS, %u threads\n", lds, block.x);
        abort();
    }
    memset(fi_smem, 0xA5, sizeof fi_smem);      // a kernel that relied on what LDS held would not reproduce the contract
    hipLaunchKernelGGL(kernel, grid, block, lds, s, a);
}
#define hipLaunchKernelGGL fi_emu_launch
extern "C" size_t fi_emu_scratch_bytes() { return g_fi_scratch_bytes; }
extern "C" size_t fi_emu_launches() { return g_fi_launches; }
extern "C" size_t fi_emu_blocks() { return g_fi_blocks; }
extern "C" size_t fi_emu_tables() { return g_fi_tables; }
