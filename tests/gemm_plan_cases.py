"""Cases for csrc/gemm_plan.h (tests/test_gemm_plan_cpu.py, tools/micro/gemm_plan_trace.py): the GEMMs of the encoder presets with
their recorded plans, and the choice of kernel as gemm_bf16.hip spelled it before it had a plan -- launch_gemm_bf16_ex,
launch_v2_pick, launch_v34, launch_v3 / launch_v4 / launch_v2, gemm_resadd_ln_tail_eligible and launch_gemm_ln_bf16, transcribed
rule by rule -- which is where the boundary tests take their expectations from."""
EPI = {"BF16": 0, "GELU_BF16": 1, "QGELU_BF16": 2, "RESADD_F32": 3, "PATCH_F32": 4, "F32": 5, "LNF_BF16": 6, "LNF_GELU_BF16": 7,
       "LNF_QGELU_BF16": 8, "RESADD_STATS_F32": 9, "LN_RES_F32": 10, "RESADD_LN_F32": 11}
KERNELS = ("V1", "V2_A", "V2_B", "V2_C", "V2_D", "V3", "V4", "LN_ROW_128", "LN_ROW_256", "LN_ROW_512")
PLAN_FIELDS = ("kernel", "tiles_m", "tiles_n", "group_n", "grid", "block", "lds_bytes", "skew", "merge_first", "kernel_slices", "ln_tail")
# GemmSwitches, member by member; the library's switch each one carries
SWITCH_FIELDS = ("v1", "cfg_set", "cfg", "v3_off", "v4_off", "v4_grid_set", "v4_grid", "group_n_set", "group_n", "skew_ns_per_k",
                 "ln_tail", "ln_v4")


def switches(**options):
    """GemmSwitches as gemm_bf16.hip fills it from the library's switches, given by name without the prefix:
    switches(GEMM_CFG="C", GEMM_V4="0") -> the 12 integers of tests/gemm_plan_shim.cpp"""
    o = {k: str(v) for k, v in options.items()}
    assert set(o) <= {"GEMM_V1", "GEMM_CFG", "GEMM_V3", "GEMM_V4", "GEMM_V4_GRID", "GEMM_GROUP_N", "GEMM_SKEW_NS_PER_K", "GEMM_LN_TAIL",
                      "GEMM_LN_V4"}, o
    first = lambda name: ord(o[name][0]) if o.get(name) else 0
    return [int("GEMM_V1" in o), int("GEMM_CFG" in o), first("GEMM_CFG"), int(first("GEMM_V3") == ord("0")),
            int(first("GEMM_V4") == ord("0")), int("GEMM_V4_GRID" in o), int(o.get("GEMM_V4_GRID", 0)), int("GEMM_GROUP_N" in o),
            int(o.get("GEMM_GROUP_N", 0)), int(o.get("GEMM_SKEW_NS_PER_K", 0)), int(first("GEMM_LN_TAIL") == ord("1")), first("GEMM_LN_V4")]


# ---- the rules before the plan, transcribed -----------------------------------------------------------------------------------------
RING = 8 * 16384
V2 = {"A": (2, 4, 8, 4, 4), "B": (4, 2, 4, 4, 4), "C": (1, 4, 8, 4, 3), "D": (2, 2, 8, 4, 3)}


def _bf16_out(e):
    return e in (0, 1, 2, 6, 7, 8)


def _lnf(e):
    return 6 <= e <= 8


def _epi_v4(e):
    return e != EPI["PATCH_F32"]


def _clamp_group(g, tiles_n, o):
    if "GEMM_GROUP_N" in o:
        g = int(o["GEMM_GROUP_N"])
    return 1 if g < 1 else min(g, tiles_n)


def old_v4_shape_ok(tiles_m, tiles_n, n, k, cus, bf16_out):
    a_span, w_span = tiles_m * 256 * k * 2, tiles_n * 256 * k * 2
    out_span_ok = tiles_m * 256 * n * (2 if bf16_out else 4) < 2 ** 32
    return (k % 128 == 0 and 128 <= k <= 3072 and cus % 8 == 0 and tiles_m * tiles_n > cus and a_span < 2 ** 32 and w_span < 2 ** 32
            and out_span_ok)


def _plan(kernel, tiles_m, tiles_n, group_n, grid, block, lds, skew=0, merge_first=0, kernel_slices=0, ln_tail=0):
    return dict(zip(PLAN_FIELDS, (kernel, tiles_m, tiles_n, group_n, grid, block, lds, skew, merge_first, kernel_slices, ln_tail)))


def _old_v2(cfg, m, n, k, o, nslices=0):
    wm, wn, tm, tn, stages = V2[cfg]
    bm, bn, nw = wm * tm * 16, wn * tn * 16, wm * wn
    tiles_m, tiles_n = (m + bm - 1) // bm, (n + bn - 1) // bn
    g = (3 << 19) // (bn * k * 2)
    if tiles_n <= 4:
        g = tiles_n
    skew = int(o.get("GEMM_SKEW_NS_PER_K", 0)) * k // 10
    return _plan("V2_" + cfg, tiles_m, tiles_n, _clamp_group(g, tiles_n, o), tiles_m * tiles_n, nw * 64,
                 max(stages * (bm + bn) * 64, nw * 16384), skew, 0, nslices)


def _old_v34(m, n, k, e, has_slices, nslices, cus, o):
    tiles_m, tiles_n = (m + 255) // 256, (n + 255) // 256
    group = _clamp_group(3 if tiles_n % 4 != 0 and tiles_n % 3 == 0 else 4, tiles_n, o)
    if (_epi_v4(e) and o.get("GEMM_V4", "x")[0] != "0" and old_v4_shape_ok(tiles_m, tiles_n, n, k, cus, _bf16_out(e))
            and (not _lnf(e) or m * 8 < 2 ** 32)):
        grid, g = cus, int(o.get("GEMM_V4_GRID", 0))
        if 8 <= g <= cus and g % 8 == 0:
            grid = g
        merge_first, in_kernel = 0, 0
        if _lnf(e):
            if has_slices and nslices > 12:
                merge_first = 1
            elif has_slices:
                in_kernel = nslices
        lds = RING + (2 * 2048 + 2048 + in_kernel * 2048 if _lnf(e) else 2048)
        return _plan("V4", tiles_m, tiles_n, group, grid, 512, lds, 0, merge_first, in_kernel)
    return _plan("V3", tiles_m, tiles_n, group, tiles_m * tiles_n, 512, RING + 4096, 0, int(_lnf(e) and has_slices), 0)


def old_gemm(m, n, k, e, has_slices=False, nslices=0, cus=256, **o):
    """launch_gemm_bf16_ex for epilogue e under the switches o (names without the prefix, string values)"""
    o = {key: str(v) for key, v in o.items()}
    big_tiles = ((m + 255) // 256) * ((n + 255) // 256)
    fills = big_tiles > (64 if k <= 512 else 128)
    fused = e >= EPI["LNF_BF16"]
    v2 = fused or ("GEMM_V1" not in o and m >= 1024 and k % 32 == 0 and n % 8 == 0 and (fills or "GEMM_CFG" in o))
    if not v2:
        tiles_m, tiles_n = (m + 127) // 128, (n + 127) // 128
        return _plan("V1", tiles_m, tiles_n, 1, tiles_m * tiles_n, 256, 0)
    if fused:
        return _old_v34(m, n, k, e, has_slices, nslices, cus, o) if k % 64 == 0 else _old_v2("A", m, n, k, o, nslices)
    cfg = "A" if n > 128 else "B"
    if k <= 512 and n > 128:
        cfg = "D" if n % 256 != 0 and n % 128 == 0 else "C"
        if _epi_v4(e) and k % 128 == 0 and k >= 128 and n % 256 == 0 and ((m + 255) // 256) * (n // 256) > 256:
            cfg = "A"
    if "GEMM_CFG" in o:
        cfg = o["GEMM_CFG"][0]
    if cfg == "A" and k % 64 == 0 and o.get("GEMM_V3", "x")[0] != "0":
        return _old_v34(m, n, k, e, has_slices, nslices, cus, o)
    return _old_v2(cfg if cfg in "ABC" else "D", m, n, k, o)


def old_tail_eligible(m, n, k, cus=256, **o):
    """gemm_resadd_ln_tail_eligible"""
    o = {key: str(v) for key, v in o.items()}
    if (o.get("GEMM_LN_TAIL", "x")[0] != "1" or o.get("GEMM_V4", "x")[0] == "0" or o.get("GEMM_V3", "x")[0] == "0" or "GEMM_V1" in o
            or "GEMM_CFG" in o or "GEMM_V4_GRID" in o):
        return False
    if n != 768 or k <= 512 or k % 128 != 0 or m < 1024:
        return False
    tiles_m = (m + 255) // 256
    return tiles_m % 8 == 0 and old_v4_shape_ok(tiles_m, n // 256, n, k, cus, False)


def old_gemm_ln(m, n, k, merge_res=0, cus=256, device_in_range=True, **o):
    """launch_gemm_ln_bf16"""
    o = {key: str(v) for key, v in o.items()}
    tiles_m, tiles_n = (m + 255) // 256, n // 256
    shape_ok = ((n == 256 or (n == 512 and tiles_m % 8 == 0)) and k % 128 == 0 and 128 <= k <= 3072 and cus == 256
                and tiles_m * tiles_n > cus and tiles_m * 256 * k * 2 < 2 ** 32 and tiles_m * 256 * n * 4 < 2 ** 32 and device_in_range)
    pays = n == 512 and k >= 512
    ln_v4 = o.get("GEMM_LN_V4", "x")[0]
    if shape_ok and merge_res == 0 and ln_v4 != "0" and (pays or ln_v4 == "1"):
        grid, g = cus, int(o.get("GEMM_V4_GRID", 0))
        if 16 <= g <= cus and g % 16 == 0 and tiles_m * tiles_n >= g:
            grid = g
        return _plan("V4", tiles_m, tiles_n, tiles_n, grid, 512, RING + 2048)
    if n not in (128, 256, 512):
        return None
    wm, wn, stages = {128: (8, 1, 4), 256: (4, 2, 4), 512: (2, 4, 4)}[n]
    blocks = (m + wm * 64 - 1) // (wm * 64)
    return _plan(f"LN_ROW_{n}", blocks, 1, 1, blocks, 512, max(stages * (wm * 64 + wn * 128) * 64, 8 * 16384 + 8192))


# ---- the GEMMs of the presets ---------------------------------------------------------------------------------------------------------
# (tokens, width, mlp, padded patch K, activation) of the ViT presets of vsc_hip/config.py
VIT = {"vit_b16_224": (197, 768, 3072, 768, "GELU_BF16"), "vit_b32_384": (145, 768, 3072, 3072, "GELU_BF16"),
       "clip_vit_l14_224": (257, 1024, 4096, 640, "QGELU_BF16")}
# (stage-0 side, embed) of the Swin-V2 presets of vsc_hip/swin_config.py
SWIN = {"swinv2_base_256": (64, 128), "swinv2_large_384": (96, 192)}
BATCHES = {"vit_b16_224": (8, 32, 332), "vit_b32_384": (8, 32, 332), "clip_vit_l14_224": (8, 32, 332), "swinv2_base_256": (8, 32, 256),
           "swinv2_large_384": (8, 32, 256)}


def model_gemms():
    """(name, entry, arguments) of every GEMM the presets' encoders send to gemm_bf16.hip at 8 and 32 frames and at the benchmark's
    chunks (332 ViT frames, 256 Swin frames).  entry: "gemm" (m, n, k, epilogue, has_slices, nslices), "resadd_ln" (m, n, k) or
    "gemm_ln" (m, n, k, merge_res)."""
    out = []
    for preset, (tokens, d, mlp, kpad, act) in VIT.items():
        for b in BATCHES[preset]:
            m, tag = b * tokens, f"{preset}/b{b}/"
            out.append((tag + "patch", "gemm", (b * (tokens - 1), d, kpad, EPI["PATCH_F32"], 0, 0)))
            out.append((tag + "qkv", "gemm", (m, 3 * d, d, EPI["BF16"], 0, 0)))
            out.append((tag + "proj", "gemm", (m, d, d, EPI["RESADD_F32"], 0, 0)))
            out.append((tag + "fc1", "gemm", (m, mlp, d, EPI[act], 0, 0)))
            out.append((tag + "fc2", "gemm", (m, d, mlp, EPI["RESADD_F32"], 0, 0)))
            # fuse_ln: the LayerNorm-folding kinds, statistics as d / 64 slice partials
            out.append((tag + "qkv_lnf", "gemm", (m, 3 * d, d, EPI["LNF_BF16"], 1, d // 64)))
            out.append((tag + "proj_stats", "gemm", (m, d, d, EPI["RESADD_STATS_F32"], 0, 0)))
            out.append((tag + "fc1_lnf", "gemm", (m, mlp, d, EPI["LNF_" + act], 1, d // 64)))
            out.append((tag + "fc2_stats", "gemm", (m, d, mlp, EPI["RESADD_STATS_F32"], 0, 0)))
            # the residual GEMMs with the LayerNorm behind them
            out.append((tag + "proj_ln", "resadd_ln", (m, d, d)))
            out.append((tag + "fc2_ln", "resadd_ln", (m, d, mlp)))
    for preset, (side, embed) in SWIN.items():
        for b in BATCHES[preset]:
            for s in range(4):
                c, m, tag = embed << s, b * (side >> s) ** 2, f"{preset}/b{b}/s{s}."
                out.append((tag + "qkv", "gemm", (m, 3 * c, c, EPI["BF16"], 0, 0)))
                out.append((tag + "fc1", "gemm", (m, 4 * c, c, EPI["GELU_BF16"], 0, 0)))
                for name, k in (("proj", c), ("fc2", 4 * c)):
                    if c in (128, 256, 512):
                        out.append((tag + name, "gemm_ln", (m, c, k, 0)))
                    else:   # no row-owning tile at this width: fp32 GEMM, then the row kernel
                        out.append((tag + name, "gemm", (m, c, k, EPI["F32"], 0, 0)))
                if s < 3:
                    if 2 * c in (128, 256, 512):
                        out.append((tag + "merge", "gemm_ln", (m // 4, 2 * c, 4 * c, side >> s)))
                    else:
                        out.append((tag + "merge", "gemm", (m // 4, 2 * c, 4 * c, EPI["F32"], 0, 0)))
    return out


# name -> (kernel, tiles_m, tiles_n, group_n, grid, block, lds_bytes, merge_first, kernel_slices, ln_tail) on 256 CUs with no switch set
# (the resadd_ln entries: with VSC_GEMM_LN_TAIL=1, which is what makes the entry differ from its RESADD GEMM)
PINNED_FIELDS = ("kernel", "tiles_m", "tiles_n", "group_n", "grid", "block", "lds_bytes", "merge_first", "kernel_slices", "ln_tail")
PINNED = {
    "vit_b16_224/b8/patch": ('V1', 13, 6, 1, 78, 256, 0, 0, 0, 0),
    "vit_b16_224/b8/qkv": ('V1', 13, 18, 1, 234, 256, 0, 0, 0, 0),
    "vit_b16_224/b8/proj": ('V1', 13, 6, 1, 78, 256, 0, 0, 0, 0),
    "vit_b16_224/b8/fc1": ('V1', 13, 24, 1, 312, 256, 0, 0, 0, 0),
    "vit_b16_224/b8/fc2": ('V1', 13, 6, 1, 78, 256, 0, 0, 0, 0),
    "vit_b16_224/b8/qkv_lnf": ('V3', 7, 9, 3, 63, 512, 135168, 1, 0, 0),
    "vit_b16_224/b8/proj_stats": ('V3', 7, 3, 3, 21, 512, 135168, 0, 0, 0),
    "vit_b16_224/b8/fc1_lnf": ('V3', 7, 12, 4, 84, 512, 135168, 1, 0, 0),
    "vit_b16_224/b8/fc2_stats": ('V3', 7, 3, 3, 21, 512, 135168, 0, 0, 0),
    "vit_b16_224/b8/proj_ln": ('V1', 13, 6, 1, 78, 256, 0, 0, 0, 0),
    "vit_b16_224/b8/fc2_ln": ('V1', 13, 6, 1, 78, 256, 0, 0, 0, 0),
    "vit_b16_224/b32/patch": ('V1', 49, 6, 1, 294, 256, 0, 0, 0, 0),
    "vit_b16_224/b32/qkv": ('V3', 25, 9, 3, 225, 512, 135168, 0, 0, 0),
    "vit_b16_224/b32/proj": ('V1', 50, 6, 1, 300, 256, 0, 0, 0, 0),
    "vit_b16_224/b32/fc1": ('V4', 25, 12, 4, 256, 512, 133120, 0, 0, 0),
    "vit_b16_224/b32/fc2": ('V1', 50, 6, 1, 300, 256, 0, 0, 0, 0),
    "vit_b16_224/b32/qkv_lnf": ('V3', 25, 9, 3, 225, 512, 135168, 1, 0, 0),
    "vit_b16_224/b32/proj_stats": ('V3', 25, 3, 3, 75, 512, 135168, 0, 0, 0),
    "vit_b16_224/b32/fc1_lnf": ('V4', 25, 12, 4, 256, 512, 161792, 0, 12, 0),
    "vit_b16_224/b32/fc2_stats": ('V3', 25, 3, 3, 75, 512, 135168, 0, 0, 0),
    "vit_b16_224/b32/proj_ln": ('V1', 50, 6, 1, 300, 256, 0, 0, 0, 0),
    "vit_b16_224/b32/fc2_ln": ('V1', 50, 6, 1, 300, 256, 0, 0, 0, 0),
    "vit_b16_224/b332/patch": ('V3', 255, 3, 3, 765, 512, 135168, 0, 0, 0),
    "vit_b16_224/b332/qkv": ('V4', 256, 9, 3, 256, 512, 133120, 0, 0, 0),
    "vit_b16_224/b332/proj": ('V4', 256, 3, 3, 256, 512, 133120, 0, 0, 0),
    "vit_b16_224/b332/fc1": ('V4', 256, 12, 4, 256, 512, 133120, 0, 0, 0),
    "vit_b16_224/b332/fc2": ('V4', 256, 3, 3, 256, 512, 133120, 0, 0, 0),
    "vit_b16_224/b332/qkv_lnf": ('V4', 256, 9, 3, 256, 512, 161792, 0, 12, 0),
    "vit_b16_224/b332/proj_stats": ('V4', 256, 3, 3, 256, 512, 133120, 0, 0, 0),
    "vit_b16_224/b332/fc1_lnf": ('V4', 256, 12, 4, 256, 512, 161792, 0, 12, 0),
    "vit_b16_224/b332/fc2_stats": ('V4', 256, 3, 3, 256, 512, 133120, 0, 0, 0),
    "vit_b16_224/b332/proj_ln": ('V4', 256, 3, 3, 256, 512, 139328, 0, 0, 1),
    "vit_b16_224/b332/fc2_ln": ('V4', 256, 3, 3, 256, 512, 139328, 0, 0, 1),
    "vit_b32_384/b8/patch": ('V1', 9, 6, 1, 54, 256, 0, 0, 0, 0),
    "vit_b32_384/b8/qkv": ('V1', 10, 18, 1, 180, 256, 0, 0, 0, 0),
    "vit_b32_384/b8/proj": ('V1', 10, 6, 1, 60, 256, 0, 0, 0, 0),
    "vit_b32_384/b8/fc1": ('V1', 10, 24, 1, 240, 256, 0, 0, 0, 0),
    "vit_b32_384/b8/fc2": ('V1', 10, 6, 1, 60, 256, 0, 0, 0, 0),
    "vit_b32_384/b8/qkv_lnf": ('V3', 5, 9, 3, 45, 512, 135168, 1, 0, 0),
    "vit_b32_384/b8/proj_stats": ('V3', 5, 3, 3, 15, 512, 135168, 0, 0, 0),
    "vit_b32_384/b8/fc1_lnf": ('V3', 5, 12, 4, 60, 512, 135168, 1, 0, 0),
    "vit_b32_384/b8/fc2_stats": ('V3', 5, 3, 3, 15, 512, 135168, 0, 0, 0),
    "vit_b32_384/b8/proj_ln": ('V1', 10, 6, 1, 60, 256, 0, 0, 0, 0),
    "vit_b32_384/b8/fc2_ln": ('V1', 10, 6, 1, 60, 256, 0, 0, 0, 0),
    "vit_b32_384/b32/patch": ('V1', 36, 6, 1, 216, 256, 0, 0, 0, 0),
    "vit_b32_384/b32/qkv": ('V3', 19, 9, 3, 171, 512, 135168, 0, 0, 0),
    "vit_b32_384/b32/proj": ('V1', 37, 6, 1, 222, 256, 0, 0, 0, 0),
    "vit_b32_384/b32/fc1": ('V3', 19, 12, 4, 228, 512, 135168, 0, 0, 0),
    "vit_b32_384/b32/fc2": ('V1', 37, 6, 1, 222, 256, 0, 0, 0, 0),
    "vit_b32_384/b32/qkv_lnf": ('V3', 19, 9, 3, 171, 512, 135168, 1, 0, 0),
    "vit_b32_384/b32/proj_stats": ('V3', 19, 3, 3, 57, 512, 135168, 0, 0, 0),
    "vit_b32_384/b32/fc1_lnf": ('V3', 19, 12, 4, 228, 512, 135168, 1, 0, 0),
    "vit_b32_384/b32/fc2_stats": ('V3', 19, 3, 3, 57, 512, 135168, 0, 0, 0),
    "vit_b32_384/b32/proj_ln": ('V1', 37, 6, 1, 222, 256, 0, 0, 0, 0),
    "vit_b32_384/b32/fc2_ln": ('V1', 37, 6, 1, 222, 256, 0, 0, 0, 0),
    "vit_b32_384/b332/patch": ('V3', 187, 3, 3, 561, 512, 135168, 0, 0, 0),
    "vit_b32_384/b332/qkv": ('V4', 189, 9, 3, 256, 512, 133120, 0, 0, 0),
    "vit_b32_384/b332/proj": ('V4', 189, 3, 3, 256, 512, 133120, 0, 0, 0),
    "vit_b32_384/b332/fc1": ('V4', 189, 12, 4, 256, 512, 133120, 0, 0, 0),
    "vit_b32_384/b332/fc2": ('V4', 189, 3, 3, 256, 512, 133120, 0, 0, 0),
    "vit_b32_384/b332/qkv_lnf": ('V4', 189, 9, 3, 256, 512, 161792, 0, 12, 0),
    "vit_b32_384/b332/proj_stats": ('V4', 189, 3, 3, 256, 512, 133120, 0, 0, 0),
    "vit_b32_384/b332/fc1_lnf": ('V4', 189, 12, 4, 256, 512, 161792, 0, 12, 0),
    "vit_b32_384/b332/fc2_stats": ('V4', 189, 3, 3, 256, 512, 133120, 0, 0, 0),
    "vit_b32_384/b332/proj_ln": ('V4', 189, 3, 3, 256, 512, 133120, 0, 0, 0),
    "vit_b32_384/b332/fc2_ln": ('V4', 189, 3, 3, 256, 512, 133120, 0, 0, 0),
    "clip_vit_l14_224/b8/patch": ('V1', 16, 8, 1, 128, 256, 0, 0, 0, 0),
    "clip_vit_l14_224/b8/qkv": ('V1', 17, 24, 1, 408, 256, 0, 0, 0, 0),
    "clip_vit_l14_224/b8/proj": ('V1', 17, 8, 1, 136, 256, 0, 0, 0, 0),
    "clip_vit_l14_224/b8/fc1": ('V3', 9, 16, 4, 144, 512, 135168, 0, 0, 0),
    "clip_vit_l14_224/b8/fc2": ('V1', 17, 8, 1, 136, 256, 0, 0, 0, 0),
    "clip_vit_l14_224/b8/qkv_lnf": ('V3', 9, 12, 4, 108, 512, 135168, 1, 0, 0),
    "clip_vit_l14_224/b8/proj_stats": ('V3', 9, 4, 4, 36, 512, 135168, 0, 0, 0),
    "clip_vit_l14_224/b8/fc1_lnf": ('V3', 9, 16, 4, 144, 512, 135168, 1, 0, 0),
    "clip_vit_l14_224/b8/fc2_stats": ('V3', 9, 4, 4, 36, 512, 135168, 0, 0, 0),
    "clip_vit_l14_224/b8/proj_ln": ('V1', 17, 8, 1, 136, 256, 0, 0, 0, 0),
    "clip_vit_l14_224/b8/fc2_ln": ('V1', 17, 8, 1, 136, 256, 0, 0, 0, 0),
    "clip_vit_l14_224/b32/patch": ('V1', 64, 8, 1, 512, 256, 0, 0, 0, 0),
    "clip_vit_l14_224/b32/qkv": ('V4', 33, 12, 4, 256, 512, 133120, 0, 0, 0),
    "clip_vit_l14_224/b32/proj": ('V3', 33, 4, 4, 132, 512, 135168, 0, 0, 0),
    "clip_vit_l14_224/b32/fc1": ('V4', 33, 16, 4, 256, 512, 133120, 0, 0, 0),
    "clip_vit_l14_224/b32/fc2": ('V3', 33, 4, 4, 132, 512, 135168, 0, 0, 0),
    "clip_vit_l14_224/b32/qkv_lnf": ('V4', 33, 12, 4, 256, 512, 137216, 1, 0, 0),
    "clip_vit_l14_224/b32/proj_stats": ('V3', 33, 4, 4, 132, 512, 135168, 0, 0, 0),
    "clip_vit_l14_224/b32/fc1_lnf": ('V4', 33, 16, 4, 256, 512, 137216, 1, 0, 0),
    "clip_vit_l14_224/b32/fc2_stats": ('V3', 33, 4, 4, 132, 512, 135168, 0, 0, 0),
    "clip_vit_l14_224/b32/proj_ln": ('V3', 33, 4, 4, 132, 512, 135168, 0, 0, 0),
    "clip_vit_l14_224/b32/fc2_ln": ('V3', 33, 4, 4, 132, 512, 135168, 0, 0, 0),
    "clip_vit_l14_224/b332/patch": ('V3', 332, 4, 4, 1328, 512, 135168, 0, 0, 0),
    "clip_vit_l14_224/b332/qkv": ('V4', 334, 12, 4, 256, 512, 133120, 0, 0, 0),
    "clip_vit_l14_224/b332/proj": ('V4', 334, 4, 4, 256, 512, 133120, 0, 0, 0),
    "clip_vit_l14_224/b332/fc1": ('V4', 334, 16, 4, 256, 512, 133120, 0, 0, 0),
    "clip_vit_l14_224/b332/fc2": ('V3', 334, 4, 4, 1336, 512, 135168, 0, 0, 0),
    "clip_vit_l14_224/b332/qkv_lnf": ('V4', 334, 12, 4, 256, 512, 137216, 1, 0, 0),
    "clip_vit_l14_224/b332/proj_stats": ('V4', 334, 4, 4, 256, 512, 133120, 0, 0, 0),
    "clip_vit_l14_224/b332/fc1_lnf": ('V4', 334, 16, 4, 256, 512, 137216, 1, 0, 0),
    "clip_vit_l14_224/b332/fc2_stats": ('V3', 334, 4, 4, 1336, 512, 135168, 0, 0, 0),
    "clip_vit_l14_224/b332/proj_ln": ('V4', 334, 4, 4, 256, 512, 133120, 0, 0, 0),
    "clip_vit_l14_224/b332/fc2_ln": ('V3', 334, 4, 4, 1336, 512, 135168, 0, 0, 0),
    "swinv2_base_256/b8/s0.qkv": ('V2_D', 128, 3, 3, 384, 256, 73728, 0, 0, 0),
    "swinv2_base_256/b8/s0.fc1": ('V2_C', 256, 2, 2, 512, 256, 73728, 0, 0, 0),
    "swinv2_base_256/b8/s0.proj": ('LN_ROW_128', 64, 1, 1, 64, 512, 163840, 0, 0, 0),
    "swinv2_base_256/b8/s0.fc2": ('LN_ROW_128', 64, 1, 1, 64, 512, 163840, 0, 0, 0),
    "swinv2_base_256/b8/s0.merge": ('LN_ROW_256', 32, 1, 1, 32, 512, 139264, 0, 0, 0),
    "swinv2_base_256/b8/s1.qkv": ('V2_C', 64, 3, 3, 192, 256, 73728, 0, 0, 0),
    "swinv2_base_256/b8/s1.fc1": ('V2_C', 64, 4, 4, 256, 256, 73728, 0, 0, 0),
    "swinv2_base_256/b8/s1.proj": ('LN_ROW_256', 32, 1, 1, 32, 512, 139264, 0, 0, 0),
    "swinv2_base_256/b8/s1.fc2": ('LN_ROW_256', 32, 1, 1, 32, 512, 139264, 0, 0, 0),
    "swinv2_base_256/b8/s1.merge": ('LN_ROW_512', 16, 1, 1, 16, 512, 163840, 0, 0, 0),
    "swinv2_base_256/b8/s2.qkv": ('V1', 16, 12, 1, 192, 256, 0, 0, 0, 0),
    "swinv2_base_256/b8/s2.fc1": ('V1', 16, 16, 1, 256, 256, 0, 0, 0, 0),
    "swinv2_base_256/b8/s2.proj": ('LN_ROW_512', 16, 1, 1, 16, 512, 163840, 0, 0, 0),
    "swinv2_base_256/b8/s2.fc2": ('LN_ROW_512', 16, 1, 1, 16, 512, 163840, 0, 0, 0),
    "swinv2_base_256/b8/s2.merge": ('V1', 4, 8, 1, 32, 256, 0, 0, 0, 0),
    "swinv2_base_256/b8/s3.qkv": ('V1', 4, 24, 1, 96, 256, 0, 0, 0, 0),
    "swinv2_base_256/b8/s3.fc1": ('V1', 4, 32, 1, 128, 256, 0, 0, 0, 0),
    "swinv2_base_256/b8/s3.proj": ('V1', 4, 8, 1, 32, 256, 0, 0, 0, 0),
    "swinv2_base_256/b8/s3.fc2": ('V1', 4, 8, 1, 32, 256, 0, 0, 0, 0),
    "swinv2_base_256/b32/s0.qkv": ('V2_D', 512, 3, 3, 1536, 256, 73728, 0, 0, 0),
    "swinv2_base_256/b32/s0.fc1": ('V4', 512, 2, 2, 256, 512, 133120, 0, 0, 0),
    "swinv2_base_256/b32/s0.proj": ('LN_ROW_128', 256, 1, 1, 256, 512, 163840, 0, 0, 0),
    "swinv2_base_256/b32/s0.fc2": ('LN_ROW_128', 256, 1, 1, 256, 512, 163840, 0, 0, 0),
    "swinv2_base_256/b32/s0.merge": ('LN_ROW_256', 128, 1, 1, 128, 512, 139264, 0, 0, 0),
    "swinv2_base_256/b32/s1.qkv": ('V4', 128, 3, 3, 256, 512, 133120, 0, 0, 0),
    "swinv2_base_256/b32/s1.fc1": ('V4', 128, 4, 4, 256, 512, 133120, 0, 0, 0),
    "swinv2_base_256/b32/s1.proj": ('LN_ROW_256', 128, 1, 1, 128, 512, 139264, 0, 0, 0),
    "swinv2_base_256/b32/s1.fc2": ('LN_ROW_256', 128, 1, 1, 128, 512, 139264, 0, 0, 0),
    "swinv2_base_256/b32/s1.merge": ('LN_ROW_512', 64, 1, 1, 64, 512, 163840, 0, 0, 0),
    "swinv2_base_256/b32/s2.qkv": ('V2_C', 64, 6, 6, 384, 256, 73728, 0, 0, 0),
    "swinv2_base_256/b32/s2.fc1": ('V2_C', 64, 8, 6, 512, 256, 73728, 0, 0, 0),
    "swinv2_base_256/b32/s2.proj": ('LN_ROW_512', 64, 1, 1, 64, 512, 163840, 0, 0, 0),
    "swinv2_base_256/b32/s2.fc2": ('LN_ROW_512', 64, 1, 1, 64, 512, 163840, 0, 0, 0),
    "swinv2_base_256/b32/s2.merge": ('V1', 16, 8, 1, 128, 256, 0, 0, 0, 0),
    "swinv2_base_256/b32/s3.qkv": ('V1', 16, 24, 1, 384, 256, 0, 0, 0, 0),
    "swinv2_base_256/b32/s3.fc1": ('V1', 16, 32, 1, 512, 256, 0, 0, 0, 0),
    "swinv2_base_256/b32/s3.proj": ('V1', 16, 8, 1, 128, 256, 0, 0, 0, 0),
    "swinv2_base_256/b32/s3.fc2": ('V1', 16, 8, 1, 128, 256, 0, 0, 0, 0),
    "swinv2_base_256/b256/s0.qkv": ('V2_D', 4096, 3, 3, 12288, 256, 73728, 0, 0, 0),
    "swinv2_base_256/b256/s0.fc1": ('V4', 4096, 2, 2, 256, 512, 133120, 0, 0, 0),
    "swinv2_base_256/b256/s0.proj": ('LN_ROW_128', 2048, 1, 1, 2048, 512, 163840, 0, 0, 0),
    "swinv2_base_256/b256/s0.fc2": ('LN_ROW_128', 2048, 1, 1, 2048, 512, 163840, 0, 0, 0),
    "swinv2_base_256/b256/s0.merge": ('LN_ROW_256', 1024, 1, 1, 1024, 512, 139264, 0, 0, 0),
    "swinv2_base_256/b256/s1.qkv": ('V4', 1024, 3, 3, 256, 512, 133120, 0, 0, 0),
    "swinv2_base_256/b256/s1.fc1": ('V4', 1024, 4, 4, 256, 512, 133120, 0, 0, 0),
    "swinv2_base_256/b256/s1.proj": ('LN_ROW_256', 1024, 1, 1, 1024, 512, 139264, 0, 0, 0),
    "swinv2_base_256/b256/s1.fc2": ('LN_ROW_256', 1024, 1, 1, 1024, 512, 139264, 0, 0, 0),
    "swinv2_base_256/b256/s1.merge": ('LN_ROW_512', 512, 1, 1, 512, 512, 163840, 0, 0, 0),
    "swinv2_base_256/b256/s2.qkv": ('V4', 256, 6, 3, 256, 512, 133120, 0, 0, 0),
    "swinv2_base_256/b256/s2.fc1": ('V4', 256, 8, 4, 256, 512, 133120, 0, 0, 0),
    "swinv2_base_256/b256/s2.proj": ('V4', 256, 2, 2, 256, 512, 133120, 0, 0, 0),
    "swinv2_base_256/b256/s2.fc2": ('V4', 256, 2, 2, 256, 512, 133120, 0, 0, 0),
    "swinv2_base_256/b256/s2.merge": ('V3', 64, 4, 4, 256, 512, 135168, 0, 0, 0),
    "swinv2_base_256/b256/s3.qkv": ('V4', 64, 12, 4, 256, 512, 133120, 0, 0, 0),
    "swinv2_base_256/b256/s3.fc1": ('V4', 64, 16, 4, 256, 512, 133120, 0, 0, 0),
    "swinv2_base_256/b256/s3.proj": ('V3', 64, 4, 4, 256, 512, 135168, 0, 0, 0),
    "swinv2_base_256/b256/s3.fc2": ('V3', 64, 4, 4, 256, 512, 135168, 0, 0, 0),
    "swinv2_large_384/b8/s0.qkv": ('V2_C', 576, 3, 3, 1728, 256, 73728, 0, 0, 0),
    "swinv2_large_384/b8/s0.fc1": ('V2_C', 576, 3, 3, 1728, 256, 73728, 0, 0, 0),
    "swinv2_large_384/b8/s0.proj": ('V2_C', 576, 1, 1, 576, 256, 73728, 0, 0, 0),
    "swinv2_large_384/b8/s0.fc2": ('V4', 288, 1, 1, 256, 512, 133120, 0, 0, 0),
    "swinv2_large_384/b8/s0.merge": ('V3', 72, 2, 2, 144, 512, 135168, 0, 0, 0),
    "swinv2_large_384/b8/s1.qkv": ('V2_D', 72, 9, 9, 648, 256, 73728, 0, 0, 0),
    "swinv2_large_384/b8/s1.fc1": ('V4', 72, 6, 3, 256, 512, 133120, 0, 0, 0),
    "swinv2_large_384/b8/s1.proj": ('V2_D', 72, 3, 3, 216, 256, 73728, 0, 0, 0),
    "swinv2_large_384/b8/s1.fc2": ('V3', 72, 2, 2, 144, 512, 135168, 0, 0, 0),
    "swinv2_large_384/b8/s1.merge": ('V1', 36, 6, 1, 216, 256, 0, 0, 0, 0),
    "swinv2_large_384/b8/s2.qkv": ('V3', 18, 9, 3, 162, 512, 135168, 0, 0, 0),
    "swinv2_large_384/b8/s2.fc1": ('V3', 18, 12, 4, 216, 512, 135168, 0, 0, 0),
    "swinv2_large_384/b8/s2.proj": ('V1', 36, 6, 1, 216, 256, 0, 0, 0, 0),
    "swinv2_large_384/b8/s2.fc2": ('V1', 36, 6, 1, 216, 256, 0, 0, 0, 0),
    "swinv2_large_384/b8/s2.merge": ('V1', 9, 12, 1, 108, 256, 0, 0, 0, 0),
    "swinv2_large_384/b8/s3.qkv": ('V1', 9, 36, 1, 324, 256, 0, 0, 0, 0),
    "swinv2_large_384/b8/s3.fc1": ('V1', 9, 48, 1, 432, 256, 0, 0, 0, 0),
    "swinv2_large_384/b8/s3.proj": ('V1', 9, 12, 1, 108, 256, 0, 0, 0, 0),
    "swinv2_large_384/b8/s3.fc2": ('V1', 9, 12, 1, 108, 256, 0, 0, 0, 0),
    "swinv2_large_384/b32/s0.qkv": ('V2_C', 2304, 3, 3, 6912, 256, 73728, 0, 0, 0),
    "swinv2_large_384/b32/s0.fc1": ('V2_C', 2304, 3, 3, 6912, 256, 73728, 0, 0, 0),
    "swinv2_large_384/b32/s0.proj": ('V2_C', 2304, 1, 1, 2304, 256, 73728, 0, 0, 0),
    "swinv2_large_384/b32/s0.fc2": ('V4', 1152, 1, 1, 256, 512, 133120, 0, 0, 0),
    "swinv2_large_384/b32/s0.merge": ('V4', 288, 2, 2, 256, 512, 133120, 0, 0, 0),
    "swinv2_large_384/b32/s1.qkv": ('V2_D', 288, 9, 9, 2592, 256, 73728, 0, 0, 0),
    "swinv2_large_384/b32/s1.fc1": ('V4', 288, 6, 3, 256, 512, 133120, 0, 0, 0),
    "swinv2_large_384/b32/s1.proj": ('V2_D', 288, 3, 3, 864, 256, 73728, 0, 0, 0),
    "swinv2_large_384/b32/s1.fc2": ('V4', 288, 2, 2, 256, 512, 133120, 0, 0, 0),
    "swinv2_large_384/b32/s1.merge": ('V3', 72, 3, 3, 216, 512, 135168, 0, 0, 0),
    "swinv2_large_384/b32/s2.qkv": ('V4', 72, 9, 3, 256, 512, 133120, 0, 0, 0),
    "swinv2_large_384/b32/s2.fc1": ('V4', 72, 12, 4, 256, 512, 133120, 0, 0, 0),
    "swinv2_large_384/b32/s2.proj": ('V3', 72, 3, 3, 216, 512, 135168, 0, 0, 0),
    "swinv2_large_384/b32/s2.fc2": ('V3', 72, 3, 3, 216, 512, 135168, 0, 0, 0),
    "swinv2_large_384/b32/s2.merge": ('V1', 36, 12, 1, 432, 256, 0, 0, 0, 0),
    "swinv2_large_384/b32/s3.qkv": ('V4', 18, 18, 3, 256, 512, 133120, 0, 0, 0),
    "swinv2_large_384/b32/s3.fc1": ('V4', 18, 24, 4, 256, 512, 133120, 0, 0, 0),
    "swinv2_large_384/b32/s3.proj": ('V1', 36, 12, 1, 432, 256, 0, 0, 0, 0),
    "swinv2_large_384/b32/s3.fc2": ('V1', 36, 12, 1, 432, 256, 0, 0, 0, 0),
    "swinv2_large_384/b256/s0.qkv": ('V2_C', 18432, 3, 3, 55296, 256, 73728, 0, 0, 0),
    "swinv2_large_384/b256/s0.fc1": ('V2_C', 18432, 3, 3, 55296, 256, 73728, 0, 0, 0),
    "swinv2_large_384/b256/s0.proj": ('V2_C', 18432, 1, 1, 18432, 256, 73728, 0, 0, 0),
    "swinv2_large_384/b256/s0.fc2": ('V4', 9216, 1, 1, 256, 512, 133120, 0, 0, 0),
    "swinv2_large_384/b256/s0.merge": ('V4', 2304, 2, 2, 256, 512, 133120, 0, 0, 0),
    "swinv2_large_384/b256/s1.qkv": ('V2_D', 2304, 9, 9, 20736, 256, 73728, 0, 0, 0),
    "swinv2_large_384/b256/s1.fc1": ('V4', 2304, 6, 3, 256, 512, 133120, 0, 0, 0),
    "swinv2_large_384/b256/s1.proj": ('V2_D', 2304, 3, 3, 6912, 256, 73728, 0, 0, 0),
    "swinv2_large_384/b256/s1.fc2": ('V4', 2304, 2, 2, 256, 512, 133120, 0, 0, 0),
    "swinv2_large_384/b256/s1.merge": ('V4', 576, 3, 3, 256, 512, 133120, 0, 0, 0),
    "swinv2_large_384/b256/s2.qkv": ('V4', 576, 9, 3, 256, 512, 133120, 0, 0, 0),
    "swinv2_large_384/b256/s2.fc1": ('V4', 576, 12, 4, 256, 512, 133120, 0, 0, 0),
    "swinv2_large_384/b256/s2.proj": ('V4', 576, 3, 3, 256, 512, 133120, 0, 0, 0),
    "swinv2_large_384/b256/s2.fc2": ('V4', 576, 3, 3, 256, 512, 133120, 0, 0, 0),
    "swinv2_large_384/b256/s2.merge": ('V4', 144, 6, 3, 256, 512, 133120, 0, 0, 0),
    "swinv2_large_384/b256/s3.qkv": ('V4', 144, 18, 3, 256, 512, 133120, 0, 0, 0),
    "swinv2_large_384/b256/s3.fc1": ('V4', 144, 24, 4, 256, 512, 133120, 0, 0, 0),
    "swinv2_large_384/b256/s3.proj": ('V4', 144, 6, 3, 256, 512, 133120, 0, 0, 0),
    "swinv2_large_384/b256/s3.fc2": ('V3', 144, 6, 3, 864, 512, 135168, 0, 0, 0),
}
