// Which GEMM kernel runs, and with what grid, N-group and LDS size: the whole choice of gemm_bf16.hip as pure functions of the
// shape, the epilogue, the CU count and the diagnostic switches.  It includes nothing, of HIP or of the library (as
// scratch_slots.h), so that tests/test_gemm_plan_cpu.py compiles it for the host.  The launchers of gemm_bf16.hip execute a plan and
// recompute none of its numbers; the refusals (VSC_REQUIRE) stay with them.
#pragma once

namespace gemmplan {

// the epilogue kinds by number (include/vsc_hip.h: vsc_epilogue; common.h: the LayerNorm-folding kinds) -- gemm_bf16.hip asserts
// that the two agree
enum { EPI_BF16 = 0, EPI_GELU_BF16 = 1, EPI_QGELU_BF16 = 2, EPI_RESADD_F32 = 3, EPI_PATCH_F32 = 4, EPI_F32 = 5, EPI_LNF_BF16 = 6,
       EPI_LNF_GELU_BF16 = 7, EPI_LNF_QGELU_BF16 = 8, EPI_RESADD_STATS_F32 = 9, EPI_LN_RES_F32 = 10, EPI_RESADD_LN_F32 = 11 };

constexpr bool epi_bf16_out(int e) {
    return e == EPI_BF16 || e == EPI_GELU_BF16 || e == EPI_QGELU_BF16 || e == EPI_LNF_BF16 || e == EPI_LNF_GELU_BF16 ||
           e == EPI_LNF_QGELU_BF16;
}
constexpr bool epi_lnf(int e) { return e >= EPI_LNF_BF16 && e <= EPI_LNF_QGELU_BF16; }
// the epilogues the persistent kernel serves (every kind but PATCH)
constexpr bool epi_v4(int e) {
    return e == EPI_BF16 || e == EPI_GELU_BF16 || e == EPI_QGELU_BF16 || e == EPI_RESADD_F32 || e == EPI_F32 || e == EPI_LN_RES_F32 ||
           epi_lnf(e) || e == EPI_RESADD_STATS_F32 || e == EPI_RESADD_LN_F32;
}

// The kernels.  V1: 128 x 128, 4 waves.  V2_*: the 256-row tile configurations of gemm_bf16_v2_kernel,
//   A: 8 waves 256x256 (1 block/CU)   B: 8 waves 256x128
//   C: 4 waves 128x256 (2 blocks/CU)  D: 4 waves 256x128 (2 blocks/CU)
// V3: A's tile on the mainloop64 K loop, one tile per workgroup.  V4: V3 as a persistent kernel.  LN_ROW_<N>: the row-owning
// gemm_ln_kernel at width N.
enum GemmKernel { NONE = -1, V1 = 0, V2_A, V2_B, V2_C, V2_D, V3, V4, LN_ROW_128, LN_ROW_256, LN_ROW_512 };

// <WAVES_M, WAVES_N, TM, TN, STAGES> of a v2 configuration and what follows from them
struct V2Config {
    int waves_m, waves_n, tm, tn, stages;
    constexpr int bm() const { return waves_m * tm * 16; }
    constexpr int bn() const { return waves_n * tn * 16; }
    constexpr int waves() const { return waves_m * waves_n; }
    // the operand ring, or the waves' 16 KiB of write-out staging where that is larger
    constexpr int lds_bytes() const {
        return stages * (bm() + bn()) * 64 > waves() * 16384 ? stages * (bm() + bn()) * 64 : waves() * 16384;
    }
};
constexpr V2Config v2_config(int kernel) {
    return kernel == V2_A ? V2Config{2, 4, 8, 4, 4} : kernel == V2_B ? V2Config{4, 2, 4, 4, 4} : kernel == V2_C ? V2Config{1, 4, 8, 4, 3}
                                                                                                                : V2Config{2, 2, 8, 4, 3};
}
// <WAVES_M, WAVES_N, STAGES> of the row-owning kernel: 512x128 (N=128), 256x256 (N=256), 128x512 (N=512)
struct LnRowConfig {
    int waves_m, waves_n, stages;
    constexpr int rows() const { return waves_m * 64; }
    // the write-out regions + row-statistic partials alias the ring once the K loop is done
    constexpr int lds_bytes() const {
        return stages * (waves_m * 64 + waves_n * 128) * 64 > 8 * 16384 + 8192 ? stages * (waves_m * 64 + waves_n * 128) * 64 : 8 * 16384 + 8192;
    }
};
constexpr LnRowConfig ln_row_config(int kernel) {
    // N = 128: 4 x 40 KiB = the whole 160 KiB: two tiles stay in flight across a barrier
    return kernel == LN_ROW_128 ? LnRowConfig{8, 1, 4} : kernel == LN_ROW_256 ? LnRowConfig{4, 2, 4} : LnRowConfig{2, 4, 4};
}
constexpr int RING_BYTES = 8 * 16384;   // mainloop64.h ml64::RING_BYTES (asserted equal in gemm_bf16.hip)
// dynamic LDS of v3: ring (== 8 waves x 16 KiB of write-out staging) + the epilogue constants
constexpr int V3_LDS_BYTES = RING_BYTES + 4096;
// ... and of v4: behind the ring the two bias rows; LayerNorm-folding kinds: bias | colsum rows, the tile's row statistics and 2 KiB
// per slice merged in the kernel; RESADD_LN: the claim word and gamma | beta behind the bias rows
constexpr int V4_MAX_SLICES = 12;
constexpr int v4_lds_bytes(int epilogue, int kernel_slices) {
    return RING_BYTES + (epi_lnf(epilogue) ? 2 * 2048 + 2048 + kernel_slices * 2048 : 2048 + (epilogue == EPI_RESADD_LN_F32 ? 64 + 2 * 768 * 4 : 0));
}

// The switches that steer the choice (common.h VSC_OPT_LIST; values as vsc_opt* reads them), filled per launch by gemm_switches()
// in gemm_bf16.hip.  All unset: the defaults.
struct GemmSwitches {
    bool v1 = false;             // VSC_GEMM_V1 set: the 128 x 128 kernel wherever it exists
    bool cfg_set = false;        // VSC_GEMM_CFG set: the 256-row family whatever the tile count, and ...
    char cfg = 0;                // ... its first character as the configuration ('A'..'D'; anything else runs D)
    bool v3_off = false;         // VSC_GEMM_V3=0: configuration A on the v2 kernel
    bool v4_off = false;         // VSC_GEMM_V4=0: v3 where v4 would run
    bool v4_grid_set = false;    // VSC_GEMM_V4_GRID set, and ...
    int v4_grid = 0;             // ... its value: persistent workgroups per launch
    bool group_n_set = false;    // VSC_GEMM_GROUP_N set, and ...
    int group_n = 0;             // ... its value: N-tiles per group, clamped to [1, tiles_n]
    int skew_ns_per_k = 0;       // VSC_GEMM_SKEW_NS_PER_K: first-round start skew of the v2 kernel
    bool ln_tail = false;        // VSC_GEMM_LN_TAIL=1: the residual GEMM with the LayerNorm as its tail (opt-in)
    char ln_v4 = 0;              // VSC_GEMM_LN_V4 first character: '1' forces the persistent LN_RES kernel, '0' switches it off
};

struct GemmPlan {
    int kernel = NONE;
    int tiles_m = 0, tiles_n = 0;   // in the kernel's own tile (V1 128 x 128, V2_* the configuration's, V3 / V4 256 x 256; LN_ROW: row blocks x 1)
    int group_n = 1;                // N-tiles per group of the tile order
    long long grid = 0;             // workgroups (the launchers refuse 2^31 and more)
    int block = 0;                  // threads per workgroup
    int lds_bytes = 0;              // dynamic LDS
    int skew = 0;                   // first-round start skew in shader cycles (v2 only)
    bool merge_first = false;       // LayerNorm-folding kinds: the slice statistics are merged into rowstats by a launch of their own first
    int kernel_slices = 0;          // ... or this many are merged per tile inside the kernel
    bool ln_tail = false;           // gemm_resadd_ln_plan: the one-launch form (V4 with the RESADD_LN write-out); false: GEMM + LayerNorm launches
};

// 256 x 256 tiles of an [m, n] output
constexpr long long tiles256_m(long long m) { return (m + 255) / 256; }
constexpr int tiles256_n(int n) { return (n + 255) / 256; }

// N-group width (tile order) of v3 and v4: groups of 4 N-tiles whatever K is.  Swept on the ViT shapes with this loop (G = 1..12,
// profiles/r02_gemm_ab_groups.txt): 4 is fastest for qkv / fc1, equal for the
// N = 768 GEMMs (3 N-tiles: one group), and the L2-capacity rule of v2 picked 1 at K = 8192 (1186 vs 1561 TF/s).
// groups of 4 N-tiles; of 3 where that divides the row of tiles and 4 does not (qkv: 9 = 3 + 3 + 3 instead of 4 + 4 + 1:
// 204 -> 199.5 us on the persistent kernel, tools/micro/gemm_v4_groups.py)
constexpr int group_n_clamped(int g, int tiles_n, const GemmSwitches &sw) {
    if (sw.group_n_set) g = sw.group_n;
    return g < 1 ? 1 : (g > tiles_n ? tiles_n : g);
}
constexpr int group_n_v34(int tiles_n, const GemmSwitches &sw) {
    return group_n_clamped((tiles_n % 4 != 0 && tiles_n % 3 == 0) ? 3 : 4, tiles_n, sw);
}

// the shapes the persistent kernel takes (tiles_m / tiles_n: 256 x 256 tiles)
constexpr bool v4_shape_ok(long long tiles_m, int tiles_n, int n, int k, int cus, bool bf16_out) {
    const long long a_span = tiles_m * 256 * k * 2, w_span = (long long)tiles_n * 256 * k * 2;
    // (K > 3072: the per-tile costs v4 removes are < 1 % of a tile and its lockstep costs ~3 % -- 8192^3 680 vs 701 us)
    // fp32 write-outs address [m, n] by 32-bit byte offsets from the matrix origin, rows of the last (ragged) tile included
    const bool out_span_ok = tiles_m * 256 * n * (bf16_out ? 2 : 4) < (1ll << 32);
    return k % 128 == 0 && k >= 128 && k <= 3072 && cus % 8 == 0 && tiles_m * tiles_n > cus && a_span < (1ll << 32) &&
           w_span < (1ll << 32) && out_span_ok;
}

inline GemmPlan plan_v1(long long m, int n) {
    GemmPlan pl;
    pl.kernel = V1;
    pl.tiles_m = (int)((m + 127) / 128);
    pl.tiles_n = (n + 127) / 128;
    pl.grid = (long long)pl.tiles_m * pl.tiles_n;
    pl.block = 256;   // (64 KiB of static LDS, none dynamic)
    return pl;
}

inline GemmPlan plan_v2(int kernel, long long m, int n, int k, const GemmSwitches &sw) {
    const V2Config c = v2_config(kernel);
    GemmPlan pl;
    pl.kernel = kernel;
    pl.tiles_m = (int)((m + c.bm() - 1) / c.bm());
    pl.tiles_n = (n + c.bn() - 1) / c.bn();
    // W panel of one N-group (G tiles x K) should sit in a 4 MiB XCD L2 next to the A panels: every N-group is one
    // more pass over A.  With few N tiles the whole width is one group whatever K is -- fc2 (N = 768, K = 3072) ran
    // 3 passes over its 402 MB A (larger than the Infinity Cache) under the L2 rule: 395 -> 330 us with one.
    int g = (int)((long long)(3 << 19) / ((long long)c.bn() * k * 2));
    if (pl.tiles_n <= 4) g = pl.tiles_n;
    pl.group_n = group_n_clamped(g, pl.tiles_n, sw);
    // first-round start skew (diagnostic, off by default): VSC_GEMM_SKEW_NS_PER_K * K / 10 shader cycles spread over the
    // first 256 workgroups.  Re-measured in the ViT step with skews from 0.6 us to a whole tile time: 0 is as fast as any
    // (19.7 k frames/s), a tile time costs 6 % -- the start-up delay is never recovered.
    pl.skew = (int)((long long)sw.skew_ns_per_k * k / 10);
    pl.grid = (long long)pl.tiles_m * pl.tiles_n;
    pl.block = c.waves() * 64;
    pl.lds_bytes = c.lds_bytes();
    return pl;
}

// the persistent kernel on `grid` workgroups; whole_row: one N-group spanning the row of tiles, no diagnostic regrouping
inline GemmPlan plan_v4(long long tiles_m, int tiles_n, int epilogue, int grid, int kernel_slices, bool whole_row, const GemmSwitches &sw) {
    GemmPlan pl;
    pl.kernel = V4;
    pl.tiles_m = (int)tiles_m;
    pl.tiles_n = tiles_n;
    pl.group_n = whole_row ? tiles_n : group_n_v34(tiles_n, sw);
    pl.grid = grid;
    pl.block = 512;
    pl.kernel_slices = kernel_slices;
    pl.lds_bytes = v4_lds_bytes(epilogue, kernel_slices);
    return pl;
}

// v3 or its persistent form: v4 wherever a workgroup gets more than one tile and the 32-bit source offsets hold
inline GemmPlan plan_v34(long long m, int n, int k, int epilogue, bool has_slices, int nslices, int cus, const GemmSwitches &sw) {
    const long long tiles_m = tiles256_m(m);
    const int tiles_n = tiles256_n(n);
    if (epi_v4(epilogue) && !sw.v4_off && v4_shape_ok(tiles_m, tiles_n, n, k, cus, epi_bf16_out(epilogue)) &&
        (!epi_lnf(epilogue) || m * 8 < (1ll << 32)))
    {
        int grid = cus;
        // diagnostic: persistent workgroups per launch (a multiple of 8).  Measured with two lanes, so that the two chunks' GEMMs run
        // side by side on half the chip each instead of one after the other: 128 -> 23.4 k, 192 -> 23.4 k, 256 -> 23.9 k frames/s
        const int g = sw.v4_grid_set ? sw.v4_grid : 0;
        if (g >= 8 && g <= cus && g % 8 == 0) grid = g;
        // statistics given as slice partials: merged per tile inside the kernel when they fit behind the ring (<= 12 slices)
        const bool merge_first = epi_lnf(epilogue) && has_slices && nslices > V4_MAX_SLICES;
        GemmPlan pl = plan_v4(tiles_m, tiles_n, epilogue, grid, epi_lnf(epilogue) && has_slices && !merge_first ? nslices : 0, false, sw);
        pl.merge_first = merge_first;
        return pl;
    }
    GemmPlan pl;
    pl.kernel = V3;
    pl.tiles_m = (int)tiles_m;
    pl.tiles_n = tiles_n;
    pl.group_n = group_n_v34(tiles_n, sw);
    pl.grid = tiles_m * tiles_n;
    pl.block = 512;
    pl.lds_bytes = V3_LDS_BYTES;
    pl.merge_first = epi_lnf(epilogue) && has_slices;
    return pl;
}

// One of the 256-row kernels, or the 128 x 128 one?  (Whose plan does not depend on the CU count: the launcher asks the device for
// it only past this test -- the small launches that end here are the ones exposed to host time.)
constexpr bool gemm_256_row_family(long long m, int n, int k, int epilogue, const GemmSwitches &sw) {
    // A launch that cannot put a 256-row tile on at least half the CUs runs the 128 x 128 kernel instead (four times
    // the workgroups, two per CU): at 8 frames (M = 1576) fc2 takes 44 instead of 74 us and proj 16 instead of 27,
    // at 32 frames the N = 768 GEMMs 26 / 57 instead of 35 / 77 us; from ~130 tiles up the big tile wins.
    const long long big_tiles = tiles256_m(m) * tiles256_n(n);
    const bool fills = big_tiles > (k <= 512 ? 64 : 128);
    const bool fused = epilogue >= EPI_LNF_BF16;  // LayerNorm-folding kinds exist in the 256-row kernels only
    return fused || (!sw.v1 && m >= 1024 && k % 32 == 0 && n % 8 == 0 && (fills || sw.cfg_set));
}

// launch_gemm_bf16_ex: epilogues BF16 .. RESADD_STATS_F32.  has_slices / nslices: GemmExtra::slices given, and their number
// (LayerNorm-folding kinds).  cus: CUs of the device.
inline GemmPlan gemm_plan(long long m, int n, int k, int epilogue, bool has_slices, int nslices, int cus, const GemmSwitches &sw) {
    if (!gemm_256_row_family(m, n, k, epilogue, sw)) return plan_v1(m, n);
    if (epilogue >= EPI_LNF_BF16) {
        // (K % 64 != 0 is refused by the entry: the v2 branch is unreachable and kept for its kernels)
        if (k % 64 == 0) return plan_v34(m, n, k, epilogue, has_slices, nslices, cus, sw);
        GemmPlan pl = plan_v2(V2_A, m, n, k, sw);
        pl.kernel_slices = nslices;
        return pl;
    }
    // wide N: 256x256 tile; N <= 1024 (proj / fc2 / patch): 256x128 so the grid still fills 256 CUs
    // Tried and dropped: 64-k stages with full 128-B line fetches (+0.6 %),
    // a 5-deep ring (+0.4 %), register staging instead of LDS-DMA (0.47x, spills), issuing the
    // LDS-DMA between the MFMA rows of the C phase (-1 %), hybrid staging with A by LDS-DMA and W
    // through registers (-3 %), an intra-wave software pipeline (A fragments refilled from the next stage right
    // after their MFMA group, W fragments double-buffered, one barrier per K-step: equal with DMA, 0.79x with DMA
    // off -- anything issued between back-to-back MFMAs costs more than the phase barriers it removes), a
    // persistent workgroup per CU with a 3-stage ring and the write-out staged behind it so the next tile's first
    // stages fly during the write-out (+-1 %: launch, fill and drain were already hidden; 3 stages are as fast
    // as 4).  tools/micro/fill_bench.hip: LDS-DMA alone delivers 21.6 B/clk/CU with 64-B row pieces (34-40 with
    // full 128-B lines), VGPR staging no more; the K loop is issue/phase-bound, not delivery-bound.
    // measured: A wins on every ViT shape (K >= 768).  With K <= 512 (Swin) the K loop is only 4-16 stages long and
    // the epilogue is a large share of a tile: the 4-wave tiles run two workgroups per CU, so one's write-out
    // overlaps the other's K loop (stage-3 qkv 765 -> 875 TF/s); D when N is a multiple of 128 but not of 256.
    char cfg = n > 128 ? 'A' : 'B';
    if (k <= 512 && n > 128) {
        cfg = (n % 256 != 0 && n % 128 == 0) ? 'D' : 'C';
        // ... unless the persistent kernel takes it (v4: K = 256 / 384 / 512, more 256 x 256 tiles than CUs): without the per-tile
        // launch / prologue / drain the big tile wins here too (Swin-V2-B batch 256: 12.15 k -> 12.95 k frames/s)
        if (epi_v4(epilogue) && k % 128 == 0 && k >= 128 && n % 256 == 0 && ((m + 255) / 256) * (n / 256) > 256) cfg = 'A';
    }
    if (sw.cfg_set) cfg = sw.cfg;   // diagnostic
    if (cfg == 'A' && k % 64 == 0 && !sw.v3_off) return plan_v34(m, n, k, epilogue, has_slices, nslices, cus, sw);
    return plan_v2(cfg == 'A' ? V2_A : cfg == 'B' ? V2_B : cfg == 'C' ? V2_C : V2_D, m, n, k, sw);
}

// ---- residual GEMM + LayerNorm: one persistent launch with the LayerNorm as its tail, or two launches ------------------------------
// The tail form needs what makes gemm_plan pick the persistent kernel for this shape (no diagnostic switch that routes it
// elsewhere), N = 768 as one N-group, and whole row blocks per XCD range: total % 8 == 0 and (total / 8) % tiles_n == 0, i.e.
// tiles_m % 8 == 0 (see ln_tail_arrive).  Otherwise: the plan of the RESADD_F32 GEMM that a LayerNorm launch follows.
inline GemmPlan gemm_resadd_ln_plan(long long m, int n, int k, int cus, const GemmSwitches &sw) {
    // OPT-IN (VSC_GEMM_LN_TAIL=1): measured on the MI355X the tail costs ~98 us a launch where the LayerNorm launch it replaces takes
    // 55 -- one lane -6 %, two lanes inside the run-to-run spread
    const bool routed = !sw.ln_tail || sw.v4_off || sw.v3_off || sw.v1 || sw.cfg_set || sw.v4_grid_set;
    const long long tiles_m = tiles256_m(m);
    // (the RESADD GEMM's own plan is V4, asked last: the listed conditions imply it on 128 CUs and more.  With fewer they do not -- 72 tiles on 64
    // CUs pass v4_shape_ok and still run the 128 x 128 kernel, because 64 / 128 tiles fill the chip whatever its size -- and the tail
    // form used to be taken there; asked of the plan itself, the invariant holds for every CU count.)
    if (!routed && n == 768 && k > 512 && k % 128 == 0 && m >= 1024 && tiles_m % 8 == 0 && v4_shape_ok(tiles_m, n / 256, n, k, cus, false) &&
        gemm_plan(m, n, k, EPI_RESADD_F32, false, 0, cus, sw).kernel == V4)
    {
        // a row block's tiles are consecutive tile indices (no diagnostic regrouping)
        GemmPlan pl = plan_v4(tiles_m, n / 256, EPI_RESADD_LN_F32, cus, 0, true, sw);
        pl.ln_tail = true;
        return pl;
    }
    return gemm_plan(m, n, k, EPI_RESADD_F32, false, 0, cus, sw);
}

// ---- launch_gemm_ln_bf16: Swin-V2's res-post-norm GEMMs ----------------------------------------------------------------------------
// Widths 256 / 512 with more 256 x 256 tiles than CUs: the persistent kernel (v4 K loop, ring streaming across tiles)
// with the LN_RES write-out -- the row-owning 128 x 512 tile stages 25 % more operand bytes per MFMA on the
// BK = 32 loop and pays a prologue per tile.  N = 512 needs whole tile pairs per XCD range (tiles_m % 8 == 0).
// merge_res > 0: the PatchMerging gather on the A operand, which only the row-owning kernel has.  device_in_range: the device
// ordinal indexes the launcher's per-device workspaces.  Widths without a row-owning tile: kernel NONE (the launcher refuses).
inline GemmPlan gemm_ln_plan(long long m, int n, int k, int merge_res, int cus, bool device_in_range, const GemmSwitches &sw) {
    const long long tiles_m = tiles256_m(m);
    const int tiles_n = n / 256;
    // cus == 256 HERE, where v4_shape_ok asks for cus % 8 == 0: the pair exchange of N = 512 pairs workgroups (b, b ^ 8) and its slots
    // are sized for 256 workgroups, and the path was measured on 256 CUs only.  The two tests are deliberately not reconciled.
    const bool shape_ok = (n == 256 || (n == 512 && tiles_m % 8 == 0)) && cus == 256 && v4_shape_ok(tiles_m, tiles_n, n, k, cus, false) &&
                          device_in_range;
    // Where it pays (tools/micro/gemm_ln_ab.py, 256 Swin-V2-B frames; round 4, with the write-out on buffer operations and no
    // spill left): N = 512 from K = 512 on -- s2 proj 96 vs 100 us, s2 fc2 166 vs 195, the un-gathered merge shape 114 vs
    // 128; at N = 256 the short-K launch ties (s1 proj 168 vs 168: bound by its bytes whichever kernel runs it) and stays
    // on the row-owning tile.  VSC_GEMM_LN_V4=1 forces the persistent kernel on every shape it supports (tests), 0
    // switches it off.
    const bool pays = n == 512 && k >= 512;
    if (shape_ok && merge_res == 0 && sw.ln_v4 != '0' && (pays || sw.ln_v4 == '1')) {
        int grid = cus;
        const int g = sw.v4_grid_set ? sw.v4_grid : 0;   // diagnostic, as in plan_v34; whole pairs: a multiple of 16
        if (g >= 16 && g <= cus && g % 16 == 0 && tiles_m * tiles_n >= g) grid = g;
        // the row's two tiles (t, t ^ 1) must land on workgroups (b, b ^ 8) of the same round: N-groups spanning the whole row
        // of tiles, no diagnostic regrouping
        return plan_v4(tiles_m, tiles_n, EPI_LN_RES_F32, grid, 0, true, sw);
    }
    GemmPlan pl;
    pl.kernel = n == 128 ? LN_ROW_128 : n == 256 ? LN_ROW_256 : n == 512 ? LN_ROW_512 : NONE;
    if (pl.kernel == NONE) return pl;
    const LnRowConfig c = ln_row_config(pl.kernel);
    pl.grid = (m + c.rows() - 1) / c.rows();
    pl.tiles_m = (int)pl.grid;
    pl.tiles_n = 1;
    pl.block = 512;
    pl.lds_bytes = c.lds_bytes();
    return pl;
}

}  // namespace gemmplan
