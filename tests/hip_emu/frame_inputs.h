// csrc/frame_inputs.hip's own beside tests/hip_emu/common.h: the coefficient cache of csrc/resample_coeffs.h (the same builder,
// compiled here for the host; "device" tables are host memory), and an LDS budget that a test build may lower
// (-DFI_EMU_LDS_BYTES) so that every target takes the two-pass path or splits into small bands; no launch may ask for more.
#pragma once
#ifdef FI_EMU_LDS_BYTES
#define EMU_LDS_BUDGET FI_EMU_LDS_BYTES
#endif
#include "common.h"
#ifdef FI_EMU_LDS_BYTES
#undef VSC_FRAME_INPUTS_LDS_BYTES
#define VSC_FRAME_INPUTS_LDS_BYTES FI_EMU_LDS_BYTES
#endif

#include <map>
#include <utility>

#include "resample_coeffs.h"
static size_t g_emu_coeff_tables = 0;
int resample_coeffs_get(const char *, int in, int out, ResampleCoeffs *res) {
    static std::map<std::pair<int, int>, std::pair<std::vector<int32_t>, int>> cache;     // (table, ksize); a map's nodes do not move
    auto key = std::make_pair(in, out);
    auto it = cache.find(key);
    if (it == cache.end()) {
        int ksize = 0;
        std::vector<int32_t> table = resample_coeffs(in, out, &ksize);
        it = cache.emplace(key, std::make_pair(std::move(table), ksize)).first;
        ++g_emu_coeff_tables;
    }
    res->dev = it->second.first.data(), res->host = it->second.first.data(), res->ksize = it->second.second;
    return 0;
}
extern "C" size_t emu_coeff_tables() { return g_emu_coeff_tables; }
