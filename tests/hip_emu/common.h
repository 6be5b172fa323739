// Host stand-in for csrc/common.h, for tests/test_match_segments_emulated.py only: csrc/match_segments.hip is compiled as plain C++
// against this header and run on the CPU -- one workgroup at a time, one OS thread per GPU thread, std::barrier for __syncthreads
// and (per 64 threads) for the wave intrinsics, which are only ever called by whole waves in that kernel.  It checks the kernel's
// phases (labels, sizes, ranks, point lookup, the MT19937 stream, trial loop, final fit) against the executable contract without
// a GPU; it says nothing about LDS limits, the device's float64 library or speed.  Device memory is host memory here.
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
using std::min; using std::max;
#define __global__
#define __device__
#define __host__
#define __launch_bounds__(x)
#define __shared__ static
#define __constant__ static const
#define __align__(x)
#define __restrict__
#define VSC_OK 0
#define VSC_ERR_INVALID 2
typedef void* hipStream_t;
struct dim3 { unsigned x; dim3(unsigned a):x(a){} };
struct Idx { int x; };
static thread_local Idx threadIdx, blockIdx;
constexpr int EMU_BLOCK = 512;
static std::barrier<> *g_block_bar;
static std::barrier<> *g_wave_bar[EMU_BLOCK/64];
static uint64_t g_xch[EMU_BLOCK/64][64];
static std::atomic<int> g_or;
alignas(16) static unsigned char ms_smem[163840];
static inline void __syncthreads() { g_block_bar->arrive_and_wait(); }
static inline int __syncthreads_or(int p) { if (p) g_or.store(1); g_block_bar->arrive_and_wait(); int r = g_or.load(); g_block_bar->arrive_and_wait(); if (threadIdx.x==0) g_or.store(0); g_block_bar->arrive_and_wait(); return r; }
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
static char g_err[512];
#define VSC_REQUIRE(cond, ...) do { if (!(cond)) { snprintf(g_err, sizeof g_err, __VA_ARGS__); fprintf(stderr, "%s\n", g_err); return VSC_ERR_INVALID; } } while (0)
#define VSC_TRY(expr) do { if (int _rc = (expr)) return _rc; } while (0)
#define VSC_CHECK_HIP(expr) do { (expr); } while (0)
#define VSC_CHECK_LAUNCH()
enum { SCRATCH_MS_TABLE = 23 };
enum { hipMemcpyHostToDevice = 1 };
static inline int search_scratch_get(int, size_t bytes, void **out) { static void *p = nullptr; static size_t n = 0; if (bytes > n) { free(p); p = malloc(bytes); n = bytes; } *out = p; return 0; }
static inline int hipMemcpyAsync(void *d, const void *s, size_t n, int, hipStream_t) { memcpy(d, s, n); return 0; }
static inline int hipStreamSynchronize(hipStream_t) { return 0; }
template<class K> static inline int vsc_allow_dynamic_lds(K, int) { return 0; }
template<class K, class A> static inline void hipLaunchKernelGGL(K kernel, dim3 grid, dim3 block, size_t, hipStream_t, A a) {
    for (unsigned b = 0; b < grid.x; ++b) {
        std::barrier<> bb(block.x); g_block_bar = &bb;
        std::vector<std::barrier<>*> wb; for (unsigned w = 0; w < block.x / 64; ++w) { wb.push_back(new std::barrier<>(64)); g_wave_bar[w] = wb.back(); }
        std::vector<std::thread> ts;
        for (unsigned t = 0; t < block.x; ++t) ts.emplace_back([=] { threadIdx.x = t; blockIdx.x = b; kernel(a); });
        for (auto &t : ts) t.join();
        for (auto *w : wb) delete w;
    }
}
