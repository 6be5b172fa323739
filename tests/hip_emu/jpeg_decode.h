// csrc/jpeg_decode.hip's and csrc/jpeg_split.hip's own beside tests/hip_emu/common.h: the wave-uniform marker as the identity, the
// measurement switch of the launches unset, and the blocking copy behind vsc_jpeg_decode_stats as a memcpy.
#pragma once
#include "common.h"
#define JD_UNIFORM(x) (x)
enum { OPT_JPEG_STAGES = 0 };
static inline int vsc_opt_int(int, int dflt) { return dflt; }
static inline int jd_emu_copy_back(void *dst, const void *src, size_t bytes) {
    memcpy(dst, src, bytes);
    return 0;
}
#define JD_COPY_BACK(dst, src, bytes) jd_emu_copy_back(dst, src, bytes)
