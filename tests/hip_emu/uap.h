// What csrc/uap.hip needs beyond tests/hip_emu/common.h (which stays as it is), for tests/test_uap_emulated.py only: the header's
// tile constant, the scratch slots of csrc/common.h with one buffer PER SLOT (common.h's stand-in hands every slot the same buffer,
// which is enough for a kernel with one slot), and hipMemsetAsync.  Fresh "device" memory is filled with 0xFF, so a kernel that
// relied on what its scratch held would not reproduce the contract.
#pragma once
#include "common.h"
#define VSC_UAP_TILE 2048
enum { SCRATCH_UAP_STATE = 0, SCRATCH_UAP_KEYS, SCRATCH_UAP_PAY, SCRATCH_UAP_HIST, SCRATCH_UAP_TREE, UAP_EMU_SLOTS };
static size_t g_uap_scratch_allocs = 0;          // how often a slot had to grow
static inline int uap_emu_scratch_get(int slot, size_t bytes, void **out) {
    static void *p[UAP_EMU_SLOTS];
    static size_t n[UAP_EMU_SLOTS];
    if (bytes < 16) bytes = 16;
    if (bytes > n[slot]) {
        free(p[slot]);
        p[slot] = malloc(bytes);
        memset(p[slot], 0xFF, bytes);
        n[slot] = bytes;
        ++g_uap_scratch_allocs;
    }
    *out = p[slot];
    return 0;
}
#define search_scratch_get uap_emu_scratch_get
extern "C" size_t uap_emu_scratch_allocs() { return g_uap_scratch_allocs; }
static inline int hipMemsetAsync(void *d, int v, size_t n, hipStream_t) { memset(d, v, n); return 0; }
