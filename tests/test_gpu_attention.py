"""The three attention families on a real MI355X, kernel by kernel, in both operand builds: the ViT kernel and its variants
(csrc/attention.hip), the Swin-V2 window kernels (csrc/swin.hip), the fp32 kernel of the video-score head (csrc/conv.hip).

The cases, the float64 references, the error model and the checks are tests/attention_cases.py; tests/test_attention_cases_cpu.py
shows without a GPU that a torch emulation of the kernels' rounding points passes every one of them and that an emulation with a
leaked pad key, a mask off by one, swapped V rows, a row sum taken before rounding P, or a wrong / missing shift mask does not.

Which token counts launch which instantiation attention_kernel<KT, .> (KT = ceil(tokens / 32) key tiles); the case ids carry it:"""
import pytest
import torch

import attention_cases as ac

pytestmark = pytest.mark.gpu

KT_CASES = {
    1: [1, 15, 16, 17, 31, 32],
    2: [33, 48, 63, 64],
    3: [65, 96],
    4: [97, 127, 128],
    5: [129, 160],
    6: [161, 191, 192],
    7: [193, 197, 224],
    8: [225, 255, 256],
    9: [257, 272, 273, 288],        # 273..: a third query tile for wave 0
    10: [289, 304, 319, 320],
}
VIT_PARAMS = [pytest.param(t, id=f"kt{kt}-{t}") for kt, ts in KT_CASES.items() for t in ts]
PRECISIONS = ("bf16", "fp16")
MANY = dict(frames=9, heads=32)     # 288 (frame, head) items: more than the 256 CUs


@pytest.fixture(scope="module")
def dev():
    from vsc_hip import _lib
    for precision in PRECISIONS:
        _lib.require_device(precision)
    return torch.device("cuda:0")


def _vit(dev, precision):
    from vsc_hip import ops

    def run(qkv, frames, tokens, heads):
        with ops.operands(precision):
            return ops.attention_bf16(qkv.to(dev), frames, tokens, heads).cpu()
    return run


def _win(dev, precision):
    from vsc_hip import ops

    def run(qkv, table, scale, frames, res, window, shift, heads, bounded=False):
        with ops.operands(precision):
            return ops.window_attention_bf16(qkv.to(dev), table.to(dev), scale.to(dev), frames, res, window, shift, heads, bounded=bounded).cpu()
    return run


def test_case_ids_name_the_key_tiles():
    assert KT_CASES == ac.VIT_KT_CASES and all((t + 31) // 32 == kt for kt, ts in KT_CASES.items() for t in ts)


# ---------------------------------------------------------------------------------------------------------- (a) ViT, random data

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tokens", VIT_PARAMS)
def test_vit_attention_within_error_model(dev, precision, tokens):
    """|got - float64| <= 4 u A + tokens eta Vmax element-wise (attention_cases.assert_within_model) on N(0, 1) and N(0, 2)
    operands, mean |d| < 2e-3 (bf16) / 2.5e-4 (fp16).  The torch emulation of the kernel's rounding points reaches
    0.32 (bf16) / 0.33 (fp16) of the bound (test_attention_cases_cpu.py); the kernel's own figure is printed with every case."""
    report = []
    try:
        ac.check_vit_random(_vit(dev, precision), precision, tokens, report=report)
    finally:
        print(f"vit random {precision}: (check, tokens, worst error / bound, mean |d|) {report}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_vit_attention_refuses_321_tokens(dev, precision):
    from vsc_hip import _lib
    qkv = torch.zeros(321, 192, dtype=ac.LP[precision]["dtype"])
    with pytest.raises(_lib.VscHipError, match=r"321 tokens unsupported \(max 320"):
        _vit(dev, precision)(qkv, 1, 321, 1)


# ---------------------------------------------------------------------------------------------------------- (b) ViT, exactness

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tokens", VIT_PARAMS)
def test_vit_attention_exact_cases(dev, precision, tokens):
    """bit for bit: constant V rows come back whatever the pad keys hold (every true logit is -72: a pad key that leaks takes the
    row); a dominant key on the first / last token returns its V row; the row sum is the sum of the rounded probabilities."""
    run = _vit(dev, precision)
    ac.check_vit_constant_v(run, precision, tokens)
    ac.check_vit_one_hot(run, precision, tokens)
    ac.check_vit_biased_p(run, precision, tokens)


# ---------------------------------------------------------------------------------------------------------- (c) ViT, isolation

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tokens", [33, 197, 257])
def test_vit_attention_frames_and_heads_are_isolated(dev, precision, tokens):
    """frame 1 of 3 (then one head of it) filled with the largest finite value, +inf, NaN: the other frames / heads keep their
    bits -- the pad rows of a frame's last key tile read nothing of the frame behind it (row < tokens)."""
    ac.check_vit_isolation(_vit(dev, precision), precision, tokens)


# ---------------------------------------------------------------------------------------------------------- (d) ViT, variants

def _variant_checks(dev, precision, tokens, option, value, frames, heads):
    """bit-identical to the default kernel on random operands (three launches: a persistent kernel's double buffer wraps), and
    the exactness and isolation checks on the variant itself, at the same item count"""
    from vsc_hip import _lib, ops
    qkv = ac.vit_random(tokens, frames, tokens, heads, 1.0, ac.LP[precision]["dtype"]).to(dev)
    with ops.operands(precision):
        ref = ops.attention_bf16(qkv, frames, tokens, heads).clone()
        with _lib.option(option, value):
            for _ in range(3):
                assert torch.equal(ac.bits(ops.attention_bf16(qkv, frames, tokens, heads)), ac.bits(ref)), f"{option}={value} differs from the default kernel"
    run = _vit(dev, precision)
    with _lib.option(option, value):
        ac.check_vit_constant_v(run, precision, tokens, frames=frames, heads=heads)
        ac.check_vit_one_hot(run, precision, tokens, frames=frames, heads=heads)
        ac.check_vit_biased_p(run, precision, tokens, frames=frames, heads=heads)
        ac.check_vit_isolation(run, precision, tokens, heads=frames * heads // 3)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tokens", [1, 31, 32, 33, 197, 255, 256])
def test_vit_attention_lds_dma_variant(dev, precision, tokens):
    """VSC_ATTN_DMA=1 (attention_dma_kernel: persistent, K / V by LDS-DMA, pad rows = rows past the descriptor's extent).  At 33 and
    197 tokens with 288 items on 256 CUs, so 32 workgroups take a second item into the other half of the double buffer; 9 items
    at the other token counts (the suite's time)."""
    shape = MANY if tokens in (33, 197) else dict(frames=3, heads=3)
    _variant_checks(dev, precision, tokens, "VSC_ATTN_DMA", "1", **shape)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("frames,heads", [(2, 3), (3, 3)])
@pytest.mark.parametrize("tokens", [33, 197, 289])
def test_vit_attention_two_items_per_workgroup_variant(dev, precision, tokens, frames, heads):
    """VSC_ATTN_NI=2 (attention_kernel<KT, 2>) with 6 and with 9 items: the last workgroup of the odd count holds one item."""
    _variant_checks(dev, precision, tokens, "VSC_ATTN_NI", "2", frames, heads)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tokens", [33, 197])
def test_vit_attention_start_skew_branch(dev, precision, tokens):
    """VSC_ATTN_SKEW=2000 cycles with 288 items: workgroups 256..287 take the start-skew branch, and the results are the same bits."""
    _variant_checks(dev, precision, tokens, "VSC_ATTN_SKEW", "2000", **MANY)


# ---------------------------------------------------------------------------------------------------------- (e) window attention

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("window,stream", [(8, None), (12, None), (16, None), (24, None),
                                           (16, "0"), (24, "0")])     # VSC_WATTN_STREAM=0: window_attention_kernel<16>, window_attention_wide_kernel<24>
def test_window_attention_cases(dev, precision, window, stream):
    """Windows 8 / 12 / 16 / 24 at res = 2 window (four windows, three on the masked last row / column) with shift 0, 1, window / 2
    and window - 1, and one window without shift; plain and bounded form: random operands and rows of zeros against float64 with
    the tolerances of the existing window tests (attention_cases.WINDOW_TOL), and bit for bit: V constant per shift-mask region
    of every window comes back as every query's own region vector (a masked key holds < e^-64 of a row), V constant per window
    as that vector (the 16 pad key slots of the 144-key window hold nothing)."""
    from vsc_hip import _lib
    run = _win(dev, precision)
    report = []
    try:
        with _lib.option("VSC_WATTN_STREAM", stream):
            for res, w, shift in ac.window_cases((window,)):
                for bounded in (False, True):
                    report.append((res, w, shift, bounded))
                    ac.check_window_random(run, precision, res, w, shift, bounded=bounded, report=report)
                    ac.check_window_zero_rows(run, precision, res, w, shift, bounded=bounded, report=report)
                    ac.check_window_constant_v(run, precision, res, w, shift, bounded=bounded, by_region=True)
                    ac.check_window_constant_v(run, precision, res, w, shift, bounded=bounded, by_region=False)
    finally:
        print(f"window {precision} stream={stream}: (res, window, shift, bounded), (check, max |d|, excess over the tolerance, mean |d|) {report}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_window_attention_refuses_a_shift_outside_the_window(dev, precision):
    from vsc_hip import _lib
    qkv, table, scale = ac.window_random(1, 1, 16, 8, 2, ac.LP[precision]["dtype"])
    for shift in (8, -1):
        with pytest.raises(_lib.VscHipError, match=f"window_attention: res 16 window 8 shift {shift}"):
            _win(dev, precision)(qkv, table, scale, 1, 16, 8, shift, 2)


# ---------------------------------------------------------------------------------------------------------- (f) fp32 attention

def _f32(dev):
    from vsc_hip import ops
    return lambda qkv, tokens, heads, head_dim: ops.attention_f32(qkv.to(dev), tokens, heads, head_dim).cpu()


@pytest.mark.parametrize("tokens", ac.F32_TOKENS)
def test_attention_f32_within_fp32_bound(dev, tokens):
    """vsc_attention_f32 against float64 at head_dim 1 .. 128 and 1 / 3 heads.  Bound (attention_cases.f32_reference), first
    order in eps = 2^-24 with gamma_n = n eps:
        |out - ref| <= (2 E + 2 gamma_tokens + 4 eps) A + tokens 2^-126 Vmax,
        E = 2 gamma_(head_dim + 2) max_j S_j + (max_j |a_j - max a| + 2) eps,  S_j = sum_d |q_d k_jd| / sqrt(head_dim),  A = sum_j w_j |v_j|
    (the dot product of a score, its scale, the subtraction of the maximum, a 2-ulp expf, the sum of the weights, the weighted sum).
    A plain fp32 torch restatement stays at 0.081 of it (test_attention_cases_cpu.py); the kernel's own figure is printed with every case."""
    report = []
    try:
        for head_dim in ac.F32_HEAD_DIMS:
            for heads in ac.F32_HEADS:
                ac.check_f32(_f32(dev), tokens, heads, head_dim, report=report)
    finally:
        print(f"fp32 attention: (tokens, heads, head_dim, worst error / bound) {report}")


def test_attention_f32_batch_equals_single_calls(dev):
    from vsc_hip import ops
    tokens, heads, head_dim, seqs = 65, 3, 48, 3
    qkv = ac.f32_random(3, seqs * tokens, heads, head_dim).to(dev)
    got = ops.attention_f32(qkv, tokens, heads, head_dim, seqs=seqs)
    for z in range(seqs):
        one = ops.attention_f32(qkv[z * tokens:(z + 1) * tokens], tokens, heads, head_dim)
        assert torch.equal(ac.bits(got[z * tokens:(z + 1) * tokens]), ac.bits(one)), f"sequence {z} of the batch"


def test_attention_f32_varlen_equals_single_calls_and_stays_in_its_rows(dev):
    """lengths [5, 0, 1, 257, 64] starting at row 3 of a buffer with 4 rows behind the last sequence: each sequence has the bits
    of vsc_attention_f32 on it alone, and the sentinel stays in every row outside the sequences"""
    from vsc_hip import ops
    heads, head_dim, lengths = 3, 48, [5, 0, 1, 257, 64]
    offs = [3]
    for n in lengths:
        offs.append(offs[-1] + n)
    rows = offs[-1] + 4
    qkv = ac.f32_random(4, rows, heads, head_dim).to(dev)
    sentinel = -12345.0
    out = torch.full((rows, heads * head_dim), sentinel, device=dev)
    got = ops.attention_f32(qkv, max(lengths), heads, head_dim, seqs=len(lengths), row_offsets=torch.tensor(offs, dtype=torch.int32, device=dev), out=out)
    assert got.data_ptr() == out.data_ptr()
    assert bool((out[:offs[0]] == sentinel).all()) and bool((out[offs[-1]:] == sentinel).all())
    for z, n in enumerate(lengths):
        if n:
            one = ops.attention_f32(qkv[offs[z]:offs[z + 1]], n, heads, head_dim)
            assert torch.equal(ac.bits(out[offs[z]:offs[z + 1]]), ac.bits(one)), f"sequence {z} ({n} tokens)"
    ref, bound = ac.f32_reference(qkv.cpu(), heads, head_dim, offs)
    inside = torch.isfinite(ref)
    assert bool(((out.cpu().double() - ref).abs()[inside] <= bound[inside]).all())


def test_attention_f32_refusals(dev):
    from vsc_hip import _lib, ops
    with pytest.raises(_lib.VscHipError, match="attention_f32: 8193 tokens"):
        ops.attention_f32(torch.zeros(8193, 3, device=dev), 8193, 1, 1)
    with pytest.raises(_lib.VscHipError, match="1 tokens x head_dim 2458 exceeds the kernel's LDS budget"):         # (1 + 5 * 2458) * 4 B = 48 KiB + 12 B
        ops.attention_f32(torch.zeros(1, 3 * 2458, device=dev), 1, 1, 2458)
    ops.attention_f32(torch.zeros(3, 3 * 2457, device=dev), 3, 1, 2457)                                              # (3 + 5 * 2457) * 4 B = 48 KiB: the limit itself
    with pytest.raises(_lib.VscHipError, match="attention_f32_varlen: bad arguments"):
        lib = _lib.require_device()
        qkv, out = torch.zeros(4, 12, device=dev), torch.zeros(4, 4, device=dev)
        _lib.check(lib.vsc_attention_f32_varlen(_lib.ptr(qkv), _lib.ptr(out), None, 1, 4, 1, 4, _lib.current_stream()))
    with pytest.raises(_lib.VscHipError, match="attention_f32_varlen: 8193 tokens"):
        ops.attention_f32(torch.zeros(4, 3, device=dev), 8193, 1, 1, seqs=1, row_offsets=torch.tensor([0, 4], dtype=torch.int32, device=dev))
