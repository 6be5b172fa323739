"""csrc/gemm_plan.h, compiled for the host: the choice of GEMM kernel as a pure function (no GPU).

The expectations are the recorded table of tests/gemm_plan_cases.py and its transcription of the rules gemm_bf16.hip had before the
plan existed (old_gemm, old_tail_eligible, old_gemm_ln) -- never the plan's own answers.  The shim is an ordinary shared library;
the sweep runs a second time in a stand-alone program under -fsanitize=address,undefined, started as a child process."""
import ctypes
import os
import subprocess

import pytest

import gemm_plan_cases as C
import hip_emu_build

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gemm_plan") / "libgemm_plan_shim.so")
    subprocess.check_call([hip_emu_build.compiler(), "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Werror", "-I", hip_emu_build.CSRC,
                           "-o", out, os.path.join(HERE, "gemm_plan_shim.cpp")])
    lib = ctypes.CDLL(out)
    lib.plan_tail_sweep.restype = ctypes.c_longlong
    return lib


def _call(fn, *args, **options):
    sw, out = (ctypes.c_int * 12)(*C.switches(**options)), (ctypes.c_longlong * 11)()
    fn(*[ctypes.c_longlong(a) if i == 0 else ctypes.c_int(int(a)) for i, a in enumerate(args)], sw, out)
    plan = dict(zip(C.PLAN_FIELDS, out))
    plan["kernel"] = C.KERNELS[plan["kernel"]] if plan["kernel"] >= 0 else None
    return plan


def gemm(shim, m, n, k, e, has_slices=False, nslices=0, cus=256, **o):
    return _call(shim.plan_gemm, m, n, k, C.EPI[e] if isinstance(e, str) else e, has_slices, nslices, cus, **o)


def resadd_ln(shim, m, n, k, cus=256, **o):
    return _call(shim.plan_resadd_ln, m, n, k, cus, **o)


def gemm_ln(shim, m, n, k, merge_res=0, cus=256, device_in_range=True, **o):
    return _call(shim.plan_gemm_ln, m, n, k, merge_res, cus, device_in_range, **o)


def _same_as_old(shim, m, n, k, e, has_slices=False, nslices=0, cus=256, **o):
    e = C.EPI[e] if isinstance(e, str) else e
    new, old = gemm(shim, m, n, k, e, has_slices, nslices, cus, **o), C.old_gemm(m, n, k, e, has_slices, nslices, cus, **o)
    assert new == old, (m, n, k, e, o, new, old)
    return new


def test_model_gemms_have_their_recorded_plans(shim):
    cases = C.model_gemms()
    assert len({name for name, _, _ in cases}) == len(cases) and {name for name, _, _ in cases} == set(C.PINNED)
    for name, entry, args in cases:
        if entry == "gemm":
            plan, old = gemm(shim, *args), C.old_gemm(*args)
        elif entry == "resadd_ln":
            plan = resadd_ln(shim, *args, GEMM_LN_TAIL=1)
            old = dict(C.old_gemm(*args, C.EPI["RESADD_F32"]), ln_tail=0)
            if C.old_tail_eligible(*args, GEMM_LN_TAIL=1):
                tiles_m = (args[0] + 255) // 256
                old = C._plan("V4", tiles_m, 3, 3, 256, 512, C.RING + 2048 + 64 + 2 * 768 * 4, ln_tail=1)
        else:
            plan, old = gemm_ln(shim, *args), C.old_gemm_ln(*args)
        assert tuple(plan[f] for f in C.PINNED_FIELDS) == C.PINNED[name], (name, plan)
        assert plan == old, (name, plan, old)


def test_the_flagship_shapes_run_the_kernels_the_design_names(shim):
    """a few rows of the table, spelled out: the benchmark's ViT chunk is persistent throughout, 8 frames are 128 x 128 tiles"""
    for name in ("qkv", "proj", "fc1", "fc2"):
        assert C.PINNED[f"vit_b16_224/b332/{name}"][0] == "V4" and C.PINNED[f"vit_b16_224/b8/{name}"][0] == "V1"
    assert C.PINNED["vit_b16_224/b332/patch"][0] == "V3"   # (the persistent kernel has no PATCH write-out)
    assert C.PINNED["vit_b16_224/b332/qkv"][1:5] == (256, 9, 3, 256)
    assert C.PINNED["swinv2_base_256/b256/s2.proj"][0] == "V4" and C.PINNED["swinv2_base_256/b256/s1.proj"][0] == "LN_ROW_256"


@pytest.mark.parametrize("e", ["BF16", "GELU_BF16", "QGELU_BF16", "RESADD_F32", "PATCH_F32", "F32"])
def test_boundaries_of_the_tile_family(shim, e):
    # 1024 rows (at N = 33280 either side has more than 128 tiles)
    assert _same_as_old(shim, 1023, 33280, 768, e)["kernel"] == "V1"
    assert _same_as_old(shim, 1024, 33280, 768, e)["kernel"] != "V1"
    # 64 / 65 tiles at K <= 512, 128 / 129 tiles above
    assert _same_as_old(shim, 64 * 256, 256, 512, e)["kernel"] == "V1"
    assert _same_as_old(shim, 64 * 256 + 1, 256, 512, e)["kernel"] == "V2_C"
    assert _same_as_old(shim, 65 * 256, 128, 256, e)["kernel"] == "V2_B"
    assert _same_as_old(shim, 65 * 256, 384, 256, e)["kernel"] == "V2_D"
    assert _same_as_old(shim, 128 * 256, 256, 768, e)["kernel"] == "V1"
    assert _same_as_old(shim, 128 * 256 + 1, 256, 768, e)["kernel"] == "V3"
    # K 512 / 576: 100 tiles fill the chip at 512 only
    assert _same_as_old(shim, 100 * 256, 256, 512, e)["kernel"] == "V2_C"
    assert _same_as_old(shim, 100 * 256, 256, 576, e)["kernel"] == "V1"
    # 256 / 257 tiles against 256 CUs; K 3072 / 3200; K % 128 != 0
    v4 = "V3" if e == "PATCH_F32" else "V4"
    assert _same_as_old(shim, 256 * 256, 256, 768, e)["kernel"] == "V3"
    assert _same_as_old(shim, 256 * 256 + 1, 256, 768, e)["kernel"] == v4
    assert _same_as_old(shim, 257 * 256, 256, 3072, e)["kernel"] == v4
    assert _same_as_old(shim, 257 * 256, 256, 3200, e)["kernel"] == "V3"
    assert _same_as_old(shim, 257 * 256, 256, 832, e)["kernel"] == "V3"
    # short K: C unless the persistent kernel takes it (more than 256 tiles, K % 128 == 0)
    assert _same_as_old(shim, 257 * 256, 256, 512, e)["kernel"] == ("V2_C" if e == "PATCH_F32" else "V4")
    assert _same_as_old(shim, 257 * 256, 256, 448, e)["kernel"] == "V2_C"
    # other CU counts: the tile counts 64 / 128 and the short-K exception's 256 are fixed numbers, "more tiles than CUs" is not
    for cus in (64, 304):
        for tiles in (64, 65, 128, 129, 256, 257, 304, 305):
            for k in (256, 512, 576, 768):
                _same_as_old(shim, tiles * 256, 256, k, e, cus=cus)
    assert _same_as_old(shim, 65 * 256, 256, 768, "BF16", cus=64)["kernel"] == "V1"
    assert _same_as_old(shim, 305 * 256, 256, 768, "BF16", cus=304)["kernel"] == "V4"
    assert _same_as_old(shim, 304 * 256, 256, 768, "BF16", cus=304)["kernel"] == "V3"
    assert _same_as_old(shim, 305 * 256, 256, 768, "BF16", cus=300)["kernel"] == "V3"     # cus % 8 != 0


def test_the_32_bit_spans(shim):
    """v4 addresses A, W and the output by 32-bit byte offsets: one tile row either side of each 2^32 span"""
    # A: tiles_m * 256 * k * 2 < 2^32 -> at K = 3072 tiles_m <= 2730
    assert _same_as_old(shim, 2730 * 256, 512, 3072, "BF16")["kernel"] == "V4"
    assert _same_as_old(shim, 2731 * 256, 512, 3072, "BF16")["kernel"] == "V3"
    # W: tiles_n * 256 * k * 2 < 2^32 -> at K = 3072 tiles_n <= 2730
    assert _same_as_old(shim, 1024, 2730 * 256, 3072, "BF16")["kernel"] == "V4"
    assert _same_as_old(shim, 1024, 2731 * 256, 3072, "BF16")["kernel"] == "V3"
    # output: tiles_m * 256 * n * (2 | 4) < 2^32 -> at N = 4096 tiles_m <= 2047 (bf16) / 1023 (fp32)
    assert _same_as_old(shim, 2047 * 256, 4096, 256, "BF16")["kernel"] == "V4"
    assert _same_as_old(shim, 2048 * 256, 4096, 256, "BF16")["kernel"] == "V3"
    assert _same_as_old(shim, 1023 * 256, 4096, 256, "F32")["kernel"] == "V4"
    assert _same_as_old(shim, 1024 * 256, 4096, 256, "F32")["kernel"] == "V3"
    assert _same_as_old(shim, 1023 * 256, 4096, 256, "RESADD_F32")["kernel"] == "V4"
    assert _same_as_old(shim, 1024 * 256, 4096, 256, "RESADD_F32")["kernel"] == "V3"
    # the row statistics of the LayerNorm-folding kinds, m * 8 < 2^32: the A span (m * K * 2, K >= 128) ends 32 times sooner
    assert _same_as_old(shim, 2 ** 29 - 1, 256, 128, "LNF_BF16")["kernel"] == "V3"
    assert _same_as_old(shim, 2 ** 29, 256, 128, "LNF_BF16")["kernel"] == "V3"
    for args in ((2730, 2, 512, 3072, 256, 1), (2731, 2, 512, 3072, 256, 1), (4, 2731, 2731 * 256, 3072, 256, 1), (1023, 16, 4096, 256, 256, 0),
                 (1024, 16, 4096, 256, 256, 0), (2047, 16, 4096, 256, 256, 1), (2048, 16, 4096, 256, 256, 1)):
        assert bool(shim.plan_v4_shape_ok(ctypes.c_longlong(args[0]), *args[1:])) == C.old_v4_shape_ok(*args[:5], bool(args[5]))


def test_layernorm_folding_kinds(shim):
    """always in the 256-row family; 12 / 13 slices: merged per tile in the kernel, or by a launch of their own first"""
    for e in ("LNF_BF16", "LNF_GELU_BF16", "LNF_QGELU_BF16"):
        assert _same_as_old(shim, 197, 768, 768, e, True, 12)["kernel"] == "V3"            # (never the 128 x 128 kernel)
        p12 = _same_as_old(shim, 332 * 197, 2304, 768, e, True, 12)
        assert (p12["kernel"], p12["merge_first"], p12["kernel_slices"], p12["lds_bytes"]) == ("V4", 0, 12, C.RING + 6144 + 12 * 2048)
        p13 = _same_as_old(shim, 332 * 197, 2304, 832, e, True, 13)                          # K % 128 != 0: v3, merged first
        assert (p13["kernel"], p13["merge_first"], p13["kernel_slices"]) == ("V3", 1, 0)
        p16 = _same_as_old(shim, 332 * 257, 3072, 1024, e, True, 16)
        assert (p16["kernel"], p16["merge_first"], p16["kernel_slices"], p16["lds_bytes"]) == ("V4", 1, 0, C.RING + 6144)
        none = _same_as_old(shim, 332 * 197, 2304, 768, e, False, 12)                        # rowstats given whole
        assert (none["kernel"], none["merge_first"], none["kernel_slices"]) == ("V4", 0, 0)
        off = _same_as_old(shim, 332 * 197, 2304, 768, e, True, 12, GEMM_V4="0")
        assert (off["kernel"], off["merge_first"], off["kernel_slices"]) == ("V3", 1, 0)
    assert _same_as_old(shim, 197, 768, 768, "RESADD_STATS_F32")["kernel"] == "V3"
    assert _same_as_old(shim, 332 * 197, 768, 3072, "RESADD_STATS_F32")["lds_bytes"] == C.RING + 2048


def test_tail_form_boundaries_and_invariant(shim):
    on = dict(GEMM_LN_TAIL=1)
    for m, n, k, cus in ((2048 * 256, 768, 768, 256), (2048 * 256 - 256, 768, 768, 256), (2040 * 256 + 1, 768, 768, 256),   # tiles_m % 8
                         (88 * 256, 768, 768, 256), (80 * 256, 768, 768, 256), (88 * 256, 768, 768, 264),                    # tiles > CUs
                         (88 * 256, 768, 512, 256), (88 * 256, 768, 640, 256), (88 * 256, 768, 704, 256), (88 * 256, 768, 3072, 256),
                         (88 * 256, 768, 3200, 256), (88 * 256, 512, 768, 256), (88 * 256, 1024, 768, 256), (1023, 768, 768, 8),
                         (1024, 768, 768, 8), (2728 * 256, 768, 3072, 256), (2736 * 256, 768, 3072, 256),
                         (5456 * 256, 768, 768, 256), (5464 * 256, 768, 768, 256)):                                        # fp32 output span
        assert bool(resadd_ln(shim, m, n, k, cus, **on)["ln_tail"]) == C.old_tail_eligible(m, n, k, cus, **on), (m, n, k, cus)
    assert resadd_ln(shim, 88 * 256, 768, 768, **on)["ln_tail"] == 1 and resadd_ln(shim, 87 * 256, 768, 768, **on)["ln_tail"] == 0
    assert resadd_ln(shim, 5456 * 256, 768, 768, **on)["ln_tail"] == 1 and resadd_ln(shim, 5464 * 256, 768, 768, **on)["ln_tail"] == 0
    assert resadd_ln(shim, 88 * 256, 768, 768)["ln_tail"] == 0                       # opt-in
    tail = resadd_ln(shim, 88 * 256, 768, 768, **on)
    assert tail == C._plan("V4", 88, 3, 3, 256, 512, C.RING + 2048 + 64 + 2 * 768 * 4, ln_tail=1)
    # every switch that routes the RESADD GEMM elsewhere switches the tail off, and the plan is then that GEMM's
    for o in (dict(GEMM_V4="0"), dict(GEMM_V3="0"), dict(GEMM_V1="1"), dict(GEMM_CFG="A"), dict(GEMM_V4_GRID="128")):
        assert not C.old_tail_eligible(88 * 256, 768, 768, **on, **o)
        assert resadd_ln(shim, 88 * 256, 768, 768, **on, **o) == gemm(shim, 88 * 256, 768, 768, "RESADD_F32", **on, **o)
    # the invariant of the tail's comment over m = 256 .. 2^20, k = 64 .. 4096: it exists only where the RESADD GEMM is the
    # persistent kernel with the row of tiles as one N-group
    for cus in (256, 64, 304):
        assert shim.plan_tail_sweep(cus) > 0
    # On 64 CUs the conditions gemm_resadd_ln_tail_eligible listed broke that invariant: 72 tiles are more than the CUs, yet fewer than
    # the 128 that leave the 128 x 128 kernel.  The plan asks the GEMM's own plan as well, so the tail is not taken there any more;
    # from 128 CUs up the listed conditions imply it, and the two agree on every shape of the sweep's range.
    assert C.old_tail_eligible(24 * 256, 768, 768, 64, **on) and gemm(shim, 24 * 256, 768, 768, "RESADD_F32", cus=64)["kernel"] == "V1"
    assert resadd_ln(shim, 24 * 256, 768, 768, 64, **on)["ln_tail"] == 0 and resadd_ln(shim, 48 * 256, 768, 768, 64, **on)["ln_tail"] == 1
    for cus in (128, 256, 304):
        for tiles_m in range(8, 4097, 8):
            for k in range(512, 3329, 128):
                assert bool(resadd_ln(shim, tiles_m * 256, 768, k, cus, **on)["ln_tail"]) == C.old_tail_eligible(tiles_m * 256, 768, k, cus, **on)


def test_gemm_ln_boundaries(shim):
    def same(m, n, k, merge_res=0, cus=256, device_in_range=True, **o):
        new, old = gemm_ln(shim, m, n, k, merge_res, cus, device_in_range, **o), C.old_gemm_ln(m, n, k, merge_res, cus, device_in_range, **o)
        assert new == old or (old is None and new["kernel"] is None), (m, n, k, merge_res, cus, o, new, old)
        return new["kernel"]
    assert same(264 * 256, 512, 512) == "V4" and same(263 * 256, 512, 512) == "LN_ROW_512"      # tiles_m % 8 at N = 512
    assert same(264 * 256, 512, 384) == "LN_ROW_512" and same(264 * 256, 512, 384, GEMM_LN_V4="1") == "V4"   # pays from K = 512 on
    assert same(264 * 256, 512, 512, GEMM_LN_V4="0") == "LN_ROW_512"
    assert same(128 * 256, 512, 2048) == "LN_ROW_512" and same(136 * 256, 512, 2048) == "V4"    # 256 / 272 tiles against 256 CUs
    assert same(257 * 256, 256, 256) == "LN_ROW_256" and same(257 * 256, 256, 256, GEMM_LN_V4="1") == "V4"
    assert same(256 * 256, 256, 256, GEMM_LN_V4="1") == "LN_ROW_256"
    assert same(264 * 256, 512, 2048, merge_res=32) == "LN_ROW_512"                              # the gather exists in the row kernel only
    assert same(264 * 256, 512, 512, device_in_range=False) == "LN_ROW_512"
    # cus == 256 here, not cus % 8 == 0 as in v4_shape_ok: the pair exchange is sized for 256 workgroups
    assert same(312 * 256, 512, 512, cus=304) == "LN_ROW_512" and same(312 * 256, 512, 512, cus=248) == "LN_ROW_512"
    assert same(264 * 256, 512, 3072) == "V4" and same(264 * 256, 512, 3200) == "LN_ROW_512" and same(264 * 256, 512, 576) == "LN_ROW_512"
    assert same(2728 * 256, 512, 3072) == "V4" and same(2736 * 256, 512, 3072) == "LN_ROW_512"   # the A span
    assert same(8184 * 256, 512, 512) == "V4" and same(8192 * 256, 512, 512) == "LN_ROW_512"     # the fp32 output span
    assert same(1000, 128, 128) == "LN_ROW_128" and same(1000, 384, 128) is None
    for g, grid in ((128, 128), (120, 256), (8, 256), (272, 256)):                                # whole pairs: multiples of 16
        assert gemm_ln(shim, 264 * 256, 512, 512, GEMM_V4_GRID=g)["grid"] == grid
        same(264 * 256, 512, 512, GEMM_V4_GRID=g)


SHAPES = [(332 * 197, 2304, 768, "BF16"), (332 * 197, 768, 3072, "RESADD_F32"), (8 * 197, 768, 768, "RESADD_F32"), (8448, 512, 256, "BF16"),
          (8448, 384, 256, "GELU_BF16"), (16640, 128, 512, "F32"), (8193, 1024, 768, "PATCH_F32"), (256 * 1024, 1536, 512, "BF16"),
          (332 * 197, 2304, 768, "LNF_BF16")]


def test_each_switch_alone_changes_only_what_its_comment_says(shim):
    for m, n, k, e in SHAPES:
        slices = (True, k // 64) if e.startswith("LNF") else (False, 0)
        base = _same_as_old(shim, m, n, k, e, *slices)
        fused = e.startswith("LNF")

        def differs(**o):
            new = _same_as_old(shim, m, n, k, e, *slices, **o)
            return {f for f in C.PLAN_FIELDS if new[f] != base[f]}, new
        # VSC_GEMM_V1: the 128 x 128 kernel wherever it exists
        d, new = differs(GEMM_V1="1")
        assert new["kernel"] == ("V1" if not fused else base["kernel"]) and (fused or base["kernel"] == "V1" or "kernel" in d)
        # VSC_GEMM_CFG: the named configuration of the 256-row family (from 1024 rows on); A is v3 / v4 unless VSC_GEMM_V3=0
        for cfg in "BCD":
            d, new = differs(GEMM_CFG=cfg)
            assert new["kernel"] == (base["kernel"] if fused else "V2_" + cfg)
        assert differs(GEMM_CFG="A")[1]["kernel"] in ("V3", "V4")
        assert differs(GEMM_CFG="A", GEMM_V3="0")[1]["kernel"] == ("V2_A" if not fused else base["kernel"])
        # VSC_GEMM_V3=0 alone: only configuration A changes, to the v2 kernel
        d, new = differs(GEMM_V3="0")
        assert (new["kernel"] == "V2_A" and not fused) if base["kernel"] in ("V3", "V4") and not fused else not d
        # VSC_GEMM_V4=0: v3 where v4 ran (one tile per workgroup; slice statistics merged first), nothing else
        d, new = differs(GEMM_V4="0")
        if base["kernel"] == "V4":
            assert new["kernel"] == "V3" and new["grid"] == new["tiles_m"] * new["tiles_n"] and d <= {"kernel", "grid", "lds_bytes", "merge_first", "kernel_slices"}
        else:
            assert not d
        # VSC_GEMM_V4_GRID: the grid of v4, in multiples of 8 up to the CUs
        for g, ok in ((128, True), (192, True), (100, False), (264, False), (0, False)):
            d, new = differs(GEMM_V4_GRID=g)
            assert d == ({"grid"} if ok and base["kernel"] == "V4" else set()) and (not d or new["grid"] == g)
        # VSC_GEMM_GROUP_N: N-tiles per group of the 256-row kernels, clamped to [1, tiles_n]
        for g in (0, 1, 2, 100):
            d, new = differs(GEMM_GROUP_N=g)
            want = base["group_n"] if base["kernel"] == "V1" else max(1, min(g, base["tiles_n"]))
            assert new["group_n"] == want and d <= {"group_n"}
        # VSC_GEMM_SKEW_NS_PER_K: the start skew of the v2 kernel
        d, new = differs(GEMM_SKEW_NS_PER_K=5)
        assert d == ({"skew"} if base["kernel"].startswith("V2") else set()) and new["skew"] == (5 * k // 10 if d else 0)
        # the switches of the other entries do not touch this one
        assert not differs(GEMM_LN_TAIL="1")[0] and not differs(GEMM_LN_V4="1")[0] and not differs(GEMM_LN_V4="0")[0]
    # ... nor do this entry's switches, beside VSC_GEMM_V4_GRID, touch launch_gemm_ln_bf16
    base = gemm_ln(shim, 264 * 256, 512, 512)
    for o in (dict(GEMM_V1="1"), dict(GEMM_CFG="C"), dict(GEMM_V3="0"), dict(GEMM_V4="0"), dict(GEMM_GROUP_N="1"), dict(GEMM_SKEW_NS_PER_K="5"),
              dict(GEMM_LN_TAIL="1")):
        assert gemm_ln(shim, 264 * 256, 512, 512, **o) == base


def test_sweep_under_the_sanitizers_as_a_child_process(tmp_path):
    cxx = hip_emu_build.compiler()
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
    exe = str(tmp_path / "gemm_plan_san")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
                           "-I", hip_emu_build.CSRC, "-I", HERE, "-o", exe, os.path.join(HERE, "hip_emu", "gemm_plan_sanitize_main.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), (run.stdout, run.stderr)
