// Host stand-in for csrc/common.h, for every kernel the suite checks without a GPU (tests/hip_emu/README.md): a .hip source is
// compiled as plain C++ against this header and run on the CPU -- one workgroup at a time, one OS thread per GPU thread,
// std::barrier for __syncthreads and (per 64 threads) for the wave intrinsics, which whole waves call.  Device memory is host memory.
// The public limits and status codes are those of include/vsc_hip.h, the scratch slots those of csrc/scratch_slots.h.  What a
// kernel must not rely on is poisoned: LDS before every launch, scratch and device allocations when fresh.
// tests/hip_emu_build.py builds against it; a kernel's own additions sit in a header of its name beside this one.
#pragma once
#include <barrier>
#include <thread>
#include <vector>
#include <cstring>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <algorithm>
#include <atomic>

#include "../../include/vsc_hip.h"
#include "../../vsc22-submission_amd/csrc/scratch_slots.h"
using std::min; using std::max;
#define __global__
#define __device__
#define __host__
#define __launch_bounds__(x)
#define __shared__ static
#define __constant__ static const
#define __align__(x)
#define __restrict__
typedef void* hipStream_t;
struct dim3 { unsigned x; dim3(unsigned a):x(a){} };
struct Idx { int x; };
static thread_local Idx threadIdx, blockIdx;
constexpr int EMU_BLOCK = 1024;     // the device's own limit
static std::barrier<> *g_block_bar;
static std::barrier<> *g_wave_bar[EMU_BLOCK/64];
static uint64_t g_xch[EMU_BLOCK/64][64];
static std::atomic<int> g_or;
static inline void __syncthreads() { g_block_bar->arrive_and_wait(); }
static inline int __syncthreads_or(int p) { if (p) g_or.store(1); g_block_bar->arrive_and_wait(); int r = g_or.load(); g_block_bar->arrive_and_wait(); if (threadIdx.x==0) g_or.store(0); g_block_bar->arrive_and_wait(); return r; }
static inline void __threadfence_block() {}     // the barriers already order memory
template<class T> static inline T emu_read(T v, int src) {
    int w = threadIdx.x >> 6, l = threadIdx.x & 63; uint64_t raw = 0; memcpy(&raw, &v, sizeof v); g_xch[w][l] = raw;
    g_wave_bar[w]->arrive_and_wait(); T r; memcpy(&r, &g_xch[w][src & 63], sizeof r); g_wave_bar[w]->arrive_and_wait(); return r; }
template<class T> static inline T __shfl(T v, int src, int) { return emu_read(v, src); }
template<class T> static inline T __shfl_xor(T v, int o, int) { return emu_read(v, (threadIdx.x & 63) ^ o); }
template<class T> static inline T __shfl_up(T v, int o, int) { int l = threadIdx.x & 63; T r = emu_read(v, l >= o ? l - o : l); return l >= o ? r : v; }
static inline unsigned long long __ballot(bool p) {
    int w = threadIdx.x >> 6, l = threadIdx.x & 63; g_xch[w][l] = p; g_wave_bar[w]->arrive_and_wait();
    unsigned long long m = 0; for (int i = 0; i < 64; ++i) m |= (unsigned long long)(g_xch[w][i] & 1) << i; g_wave_bar[w]->arrive_and_wait(); return m; }
static inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
static inline int __ffsll(long long v) { return __builtin_ffsll(v); }
static inline uint32_t atomicAdd(uint32_t *p, uint32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline unsigned atomicMin(unsigned *p, unsigned v) {     // (g++ has no __atomic_fetch_min)
    unsigned old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < old && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old; }
static inline unsigned long long atomicCAS(unsigned long long *p, unsigned long long expect, unsigned long long v) {
    __atomic_compare_exchange_n(p, &expect, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED); return expect; }     // -> what *p held
static inline unsigned __float_as_uint(float x) { unsigned u; memcpy(&u, &x, sizeof u); return u; }
static char g_err[512];
#define VSC_REQUIRE(cond, ...) do { if (!(cond)) { snprintf(g_err, sizeof g_err, __VA_ARGS__); fprintf(stderr, "%s\n", g_err); return VSC_ERR_INVALID; } } while (0)
#define VSC_TRY(expr) do { if (int _rc = (expr)) return _rc; } while (0)
#define VSC_CHECK_HIP(expr) do { (expr); } while (0)
#define VSC_CHECK_LAUNCH()

// ---- device memory: host allocations of exactly the size asked for (an access one byte outside is a sanitizer error), 0xFF when fresh
enum { hipMemcpyHostToDevice = 1 };
static size_t g_emu_allocs = 0;
static inline int hipMalloc(void **p, size_t bytes) { *p = malloc(bytes ? bytes : 1); memset(*p, 0xFF, bytes); ++g_emu_allocs; return 0; }
static inline int hipFree(void *p) { free(p); return 0; }
static inline int hipMemcpyAsync(void *d, const void *s, size_t n, int, hipStream_t) { memcpy(d, s, n); return 0; }
static inline int hipMemsetAsync(void *d, int v, size_t n, hipStream_t) { memset(d, v, n); return 0; }
static inline int hipStreamSynchronize(hipStream_t) { return 0; }
// the grow-only scratch of csrc/common.h: one buffer per slot, 0xFF when fresh and the last call's leftovers afterwards
static void *g_emu_scratch[SCRATCH_SLOTS];
static size_t g_emu_scratch_bytes[SCRATCH_SLOTS], g_emu_scratch_allocs = 0;      // allocs: how often a slot had to grow
static inline int search_scratch_get(int slot, size_t bytes, void **out) {
    if (bytes < 16) bytes = 16;
    if (bytes > g_emu_scratch_bytes[slot]) {
        free(g_emu_scratch[slot]);
        g_emu_scratch[slot] = malloc(bytes);
        memset(g_emu_scratch[slot], 0xFF, bytes);
        g_emu_scratch_bytes[slot] = bytes;
        ++g_emu_scratch_allocs;
    }
    *out = g_emu_scratch[slot];
    return 0;
}

// ---- launches: every kernel's dynamic LDS (`extern __shared__ ... xx_smem[]`) is this one buffer of the device's size, filled with
// a pattern before each launch.  EMU_LDS_BUDGET: what a launch may ask for; a kernel's header lowers it together with its
// VSC_*_LDS_BYTES.  Launches and workgroups are counted: the tests tell one path of a launcher from another by them.
#ifndef EMU_LDS_BUDGET
#define EMU_LDS_BUDGET (160 * 1024)
#endif
// #define EMU_NO_LDS_POISON       // (a kernel whose results depend on what LDS held: none so far)
alignas(16) static unsigned char emu_lds[160 * 1024];
static size_t g_emu_launches = 0, g_emu_blocks = 0;
template<class K> static inline int vsc_allow_dynamic_lds(K, int) { return 0; }
template<class K, class A> static inline void hipLaunchKernelGGL(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t, A a) {
    ++g_emu_launches;
    g_emu_blocks += grid.x;
    if (block.x > (unsigned)EMU_BLOCK || block.x % 64 || lds > (size_t)(EMU_LDS_BUDGET)) {
        fprintf(stderr, "hip_emu: a launch asks for %u threads, %zu bytes of LDS\n", block.x, lds);
        abort();
    }
#ifndef EMU_NO_LDS_POISON
    memset(emu_lds, 0xA5, sizeof emu_lds);
#endif
    for (unsigned b = 0; b < grid.x; ++b) {
        std::barrier<> bb(block.x); g_block_bar = &bb;
        std::vector<std::barrier<>*> wb; for (unsigned w = 0; w < block.x / 64; ++w) { wb.push_back(new std::barrier<>(64)); g_wave_bar[w] = wb.back(); }
        std::vector<std::thread> ts;
        for (unsigned t = 0; t < block.x; ++t) ts.emplace_back([=] { threadIdx.x = t; blockIdx.x = b; kernel(a); });
        for (auto &t : ts) t.join();
        for (auto *w : wb) delete w;
    }
}
extern "C" size_t emu_launches() { return g_emu_launches; }
extern "C" size_t emu_blocks() { return g_emu_blocks; }
extern "C" size_t emu_allocs() { return g_emu_allocs; }
extern "C" size_t emu_scratch_allocs() { return g_emu_scratch_allocs; }
extern "C" size_t emu_scratch_bytes(int slot) {      // of one slot; below 0: of all slots together
    size_t n = 0;
    for (int s = 0; s < SCRATCH_SLOTS; ++s) n += slot < 0 || slot == s ? g_emu_scratch_bytes[s] : 0;
    return n;
}
