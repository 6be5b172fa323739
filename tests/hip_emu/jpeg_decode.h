// What csrc/jpeg_decode.hip needs beyond tests/hip_emu/common.h (which stays as it is), for tests/test_jpeg_decode_emulated.py and
// jpeg_decode_sanitize_main.cpp only: the header's constants, device allocations as host allocations of exactly the size asked for
// and filled with 0xFF (the plane scratch and the uploaded tables: an access one byte outside either is a sanitizer error), the
// wave-uniform marker as the identity, and counters of launches and workgroups.  Build with -I <csrc>.
#pragma once
#include "common.h"

#define VSC_JPEG_FRAME_ROW 10
#define VSC_JPEG_TABLE_SET_BYTES 1608
#define VSC_JPEG_MAX_SIDE 16384
#define VSC_JPEG_STATUS_DATA 1
#define VSC_JPEG_STATUS_CODE 2
#define VSC_JPEG_STATUS_RUN 3
#define VSC_JPEG_STATUS_RESTART 4
#define JD_UNIFORM(x) (x)
enum { OPT_JPEG_STAGES = 0 };
static inline int vsc_opt_int(int, int dflt) { return dflt; }      // the measurement switch of the launches: unset
static size_t g_jd_launches = 0, g_jd_blocks = 0, g_jd_allocs = 0;
static inline int jd_emu_malloc(void **p, size_t bytes) {
    *p = malloc(bytes);
    memset(*p, 0xFF, bytes);
    ++g_jd_allocs;
    return 0;
}
static inline int jd_emu_free(void *p) {
    free(p);
    return 0;
}
#define hipMalloc jd_emu_malloc
#define hipFree jd_emu_free
template <class K, class A> static inline void jd_emu_launch(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t s, A a) {
    ++g_jd_launches;
    g_jd_blocks += grid.x;
    if (block.x > (unsigned)EMU_BLOCK || block.x % 64) {
        fprintf(stderr, "jpeg_decode emulation: a launch asks for %u threads\n", block.x);
        abort();
    }
    hipLaunchKernelGGL(kernel, grid, block, lds, s, a);
}
#define hipLaunchKernelGGL jd_emu_launch
extern "C" size_t jd_emu_launches() { return g_jd_launches; }
extern "C" size_t jd_emu_blocks() { return g_jd_blocks; }
extern "C" size_t jd_emu_allocs() { return g_jd_allocs; }
