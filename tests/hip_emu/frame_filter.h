// What csrc/frame_filter.hip needs beyond tests/hip_emu/common.h (which stays as it is), for tests/test_frame_filter_emulated.py
// only: the header's constants, the kernel's dynamic LDS as a static buffer of the device's size, its scratch slot as a buffer of its
// own that is filled with 0xFF when fresh (a kernel that relied on what its scratch held would not reproduce the contract), and the
// fence, which the emulation's barriers already imply.  ff_emu_lds_bytes(): a test build may lower the LDS budget (-DFF_EMU_LDS_BYTES)
// so that small matrices take the scratch path too.
#pragma once
#include "common.h"
#define VSC_FRAME_FILTER_MAX_ROWS 4096
#define VSC_FRAME_FILTER_CHUNK 128
#ifndef FF_EMU_LDS_BYTES
#define FF_EMU_LDS_BYTES (160 * 1024 - 1024)
#endif
#define VSC_FRAME_FILTER_LDS_BYTES FF_EMU_LDS_BYTES
enum { SCRATCH_FRAME_FILTER_BITS = 0 };
alignas(16) static unsigned char ff_smem[163840];
static size_t g_ff_scratch_allocs = 0, g_ff_scratch_bytes = 0;
static inline int ff_emu_scratch_get(int, size_t bytes, void **out) {
    static void *p = nullptr;
    if (bytes > g_ff_scratch_bytes) {
        free(p);
        p = malloc(bytes);
        memset(p, 0xFF, bytes);
        g_ff_scratch_bytes = bytes;
        ++g_ff_scratch_allocs;
    }
    *out = p;
    return 0;
}
#define search_scratch_get ff_emu_scratch_get
extern "C" size_t ff_emu_scratch_allocs() { return g_ff_scratch_allocs; }
extern "C" size_t ff_emu_scratch_bytes() { return g_ff_scratch_bytes; }
static inline void __threadfence_block() {}
