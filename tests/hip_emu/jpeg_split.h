// What csrc/jpeg_split.hip needs beyond tests/hip_emu/jpeg_decode.h (which stays as it is), for tests/test_jpeg_split_emulated.py
// and jpeg_split_sanitize_main.cpp only: the blocking copy behind vsc_jpeg_decode_stats as a memcpy.  The emulated source is
// csrc/jpeg_decode.hip followed by csrc/jpeg_split.hip in one translation unit (both entries, one handle type), each with its
// `#include "common.h"` replaced by this header.  Build with -I <csrc>.
#pragma once
#include "jpeg_decode.h"
static inline int jd_emu_copy_back(void *dst, const void *src, size_t bytes) {
    memcpy(dst, src, bytes);
    return 0;
}
#define JD_COPY_BACK(dst, src, bytes) jd_emu_copy_back(dst, src, bytes)
