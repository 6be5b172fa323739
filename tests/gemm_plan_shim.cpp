// csrc/gemm_plan.h behind a C interface for tests/test_gemm_plan_cpu.py, and the sweep of the tail form's invariant that
// tests/hip_emu/gemm_plan_sanitize_main.cpp runs under the sanitizers.  sw: the members of GemmSwitches in their order.
// out: kernel, tiles_m, tiles_n, group_n, grid, block, lds_bytes, skew, merge_first, kernel_slices, ln_tail.
#include "gemm_plan.h"
using namespace gemmplan;

static GemmSwitches switches(const int *s) {
    return GemmSwitches{s[0] != 0, s[1] != 0, (char)s[2], s[3] != 0, s[4] != 0, s[5] != 0, s[6], s[7] != 0, s[8], s[9], s[10] != 0, (char)s[11]};
}
static void put(const GemmPlan &p, long long *out) {
    const long long v[11] = {p.kernel, p.tiles_m, p.tiles_n, p.group_n, p.grid, p.block, p.lds_bytes, p.skew, p.merge_first, p.kernel_slices, p.ln_tail};
    for (int i = 0; i < 11; ++i) out[i] = v[i];
}
extern "C" void plan_gemm(long long m, int n, int k, int epilogue, int has_slices, int nslices, int cus, const int *sw, long long *out) {
    put(gemm_plan(m, n, k, epilogue, has_slices != 0, nslices, cus, switches(sw)), out);
}
extern "C" void plan_resadd_ln(long long m, int n, int k, int cus, const int *sw, long long *out) { put(gemm_resadd_ln_plan(m, n, k, cus, switches(sw)), out); }
extern "C" void plan_gemm_ln(long long m, int n, int k, int merge_res, int cus, int device_in_range, const int *sw, long long *out) {
    put(gemm_ln_plan(m, n, k, merge_res, cus, device_in_range != 0, switches(sw)), out);
}
extern "C" int plan_v4_shape_ok(long long tiles_m, int tiles_n, int n, int k, int cus, int bf16_out) { return v4_shape_ok(tiles_m, tiles_n, n, k, cus, bf16_out != 0); }

// m = 256, 512, .. 2^20 and k = 64, 128, .. 4096 with no diagnostic switch set: wherever gemm_resadd_ln_plan says tail, gemm_plan of
// the RESADD GEMM must say V4 with the whole row of tiles as one N-group, on the same grid.  -> tails seen, or -1 - (violations)
extern "C" long long plan_tail_sweep(int cus) {
    GemmSwitches sw;
    sw.ln_tail = true;
    long long tails = 0, bad = 0;
    for (long long m = 256; m <= (1ll << 20); m += 256)
        for (int k = 64; k <= 4096; k += 64) {
            const GemmPlan t = gemm_resadd_ln_plan(m, 768, k, cus, sw);
            if (!t.ln_tail) continue;
            ++tails;
            const GemmPlan g = gemm_plan(m, 768, k, EPI_RESADD_F32, false, 0, cus, sw);
            if (!(t.kernel == V4 && g.kernel == V4 && g.group_n == g.tiles_n && t.group_n == g.group_n && t.tiles_m == g.tiles_m &&
                  t.tiles_n == g.tiles_n && t.grid == g.grid && t.tiles_m % 8 == 0))
                ++bad;
        }
    return bad ? -1 - bad : tails;
}
