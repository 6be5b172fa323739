"""tests/attention_cases.py held to itself, without a GPU: the torch emulation of the kernels' rounding points passes every check
that tests/test_gpu_attention.py runs on the kernels (so the bounds can be met by the arithmetic alone), and an emulation with
one defect fails the check that is there for that defect."""
import pytest
import torch

import attention_cases as ac

PRECISIONS = ("bf16", "fp16")


def _vit(mutation=None):
    return lambda qkv, frames, tokens, heads: ac.vit_emulate(qkv, frames, tokens, heads, mutation)


def _win(mutation=None):
    return lambda *a: ac.window_emulate(*a, mutation=mutation)


def test_every_key_tile_count_has_a_case():
    assert all(ac.VIT_KT_CASES[kt] for kt in range(1, 11))
    assert sum(len(v) for v in ac.VIT_KT_CASES.values()) == len(ac.VIT_TOKENS)
    # the third query tile per wave (tokens > 256) and both sides of every 16-key sub-tile edge of the last tile
    assert {273, 288, 289, 304, 319, 320} <= set(ac.VIT_TOKENS)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_clean_vit_emulation_passes_every_check(precision):
    report = []
    for tokens in ac.VIT_TOKENS:
        ac.check_vit_random(_vit(), precision, tokens, report=report)
        ac.check_vit_constant_v(_vit(), precision, tokens)
        ac.check_vit_one_hot(_vit(), precision, tokens)
        ac.check_vit_biased_p(_vit(), precision, tokens)
    for tokens in (33, 197, 257):
        ac.check_vit_isolation(_vit(), precision, tokens)
    worst = max(r[2] for r in report)
    print(f"{precision}: worst error / bound of the emulation {worst:.3f}")
    assert worst < 0.5      # the reference arithmetic alone leaves half of the bound to the hardware's exp2 / rcp and summation order


@pytest.mark.parametrize("precision", PRECISIONS)
def test_biased_p_construction_has_margin(precision):
    """vit_biased_p: with the sum of the UNROUNDED probabilities a component 2^k of c comes out as 2^k (1 - r m / (1 + m)); the
    next value down is picked once that factor is below 1 - u / 2.  From 15 tokens on the construction clears it by 20 %."""
    u = ac.LP[precision]["u"]
    t, r = ac.biased_logit(u)
    import math
    for tokens in (15, 320):
        m = (tokens - 1) * math.exp(-t)
        assert r * m / (1 + m) > 1.2 * u / 2, (t, r, tokens)
    assert float(torch.tensor(-t).to(ac.LP[precision]["dtype"])) == -t


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("mutation,check,tokens", [
    ("leak_pad_key", ac.check_vit_constant_v, 197),
    ("leak_pad_key", ac.check_vit_constant_v, 319),
    ("mask_off_by_one", ac.check_vit_one_hot, 197),
    ("mask_off_by_one", ac.check_vit_one_hot, 33),
    ("swap_v_rows", ac.check_vit_one_hot, 197),
    ("swap_v_rows", ac.check_vit_one_hot, 256),
    ("sum_before_rounding", ac.check_vit_biased_p, 17),
    ("sum_before_rounding", ac.check_vit_biased_p, 197),
])
def test_vit_mutation_is_caught_by_its_check(precision, mutation, check, tokens):
    name = check.__name__[len("check_vit_"):]
    check(_vit(), precision, tokens)
    with pytest.raises(AssertionError, match=f"^{name}:"):
        check(_vit(mutation), precision, tokens)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_leaked_pad_key_is_invisible_to_the_random_bound_at_197_tokens(precision):
    """why constant_v exists: one unmasked zero pad key among 197 keys moves a random-data output by less than the rounding the
    error model has to allow, and takes the whole output of constant_v"""
    lp = ac.LP[precision]

    def ratio(tokens, std):
        qkv = ac.vit_random(1000 * tokens + int(std), 2, tokens, 2, std, lp["dtype"])
        ref, A, vmax = ac.vit_reference(qkv, 2, tokens, 2)
        return ac.assert_within_model(ac.vit_emulate(qkv, 2, tokens, 2, "leak_pad_key"), ref, A, vmax, tokens, lp["u"], lp["eta"])

    for std in (1.0, 2.0):
        assert ratio(197, std) <= 1.0           # inside the element-wise bound (the fp16 mean check alone notices it at std 1)
    with pytest.raises(AssertionError, match="^random:"):
        ratio(17, 1.0)
    qkv, want = ac.vit_constant_v(7 + 197, 2, 197, 2, ac.LP[precision]["dtype"])
    got = ac.vit_emulate(qkv, 2, 197, 2, "leak_pad_key")
    assert float((got.float() - want.float()).abs().min()) >= 2.0


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("window", [8, 12, 16, 24])
def test_clean_window_emulation_passes_every_check(precision, window):
    for res, w, shift in ac.window_cases((window,)):
        for bounded in (False, True):
            ac.check_window_random(_win(), precision, res, w, shift, bounded=bounded)
            ac.check_window_constant_v(_win(), precision, res, w, shift, bounded=bounded, by_region=True)
            ac.check_window_constant_v(_win(), precision, res, w, shift, bounded=bounded, by_region=False)
            ac.check_window_zero_rows(_win(), precision, res, w, shift, bounded=bounded)


def test_window_regions_are_those_of_the_oracle_mask():
    from oracle import swin_oracle
    for res, w, shift in ac.window_cases():
        reg = ac.window_regions(res, w, shift)
        if not shift:
            assert int(reg.max()) == 0
            continue
        same = reg[:, :, None] == reg[:, None, :]
        assert torch.equal(same, swin_oracle.shift_mask(res, w, shift) == 0)
        assert int(reg[-1].max()) == 3 and int(reg[0].max()) == 0       # the last window holds four regions, the first one


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("mutation,window,shift", [("drop_shift_mask", 8, 4), ("drop_shift_mask", 12, 11), ("drop_shift_mask", 16, 1),
                                                   ("drop_shift_mask", 24, 12), ("mask_of_half_window", 8, 1), ("mask_of_half_window", 12, 1),
                                                   ("mask_of_half_window", 16, 1), ("mask_of_half_window", 24, 1)])
def test_window_mutation_is_caught_by_region_constant_v(precision, mutation, window, shift):
    for bounded in (False, True):
        ac.check_window_constant_v(_win(), precision, 2 * window, window, shift, bounded=bounded)
        with pytest.raises(AssertionError, match="^region_constant_v:"):
            ac.check_window_constant_v(_win(mutation), precision, 2 * window, window, shift, bounded=bounded)


def test_f32_restatement_stays_under_half_of_the_bound():
    """a plain fp32 torch restatement of attention_f32_kernel against float64: under half of f32_reference's bound at every case"""
    report = []
    run = lambda qkv, tokens, heads, head_dim: ac.f32_emulate(qkv, heads, head_dim, [0, tokens])
    for tokens in ac.F32_TOKENS:
        for head_dim in ac.F32_HEAD_DIMS:
            for heads in ac.F32_HEADS:
                ac.check_f32(run, tokens, heads, head_dim, report=report)
    worst = max(r[3] for r in report)
    print(f"fp32 restatement: worst error / bound {worst:.3f}")
    assert worst < 0.5


def test_f32_reference_variable_length_layout():
    qkv = ac.f32_random(5, 20, 2, 8)
    offs = [3, 8, 8, 9, 17]
    ref, bound = ac.f32_reference(qkv, 2, 8, offs)
    assert torch.isnan(ref[:3]).all() and torch.isnan(ref[17:]).all() and torch.isfinite(ref[3:17]).all()
    one, _ = ac.f32_reference(qkv[9:17], 2, 8, [0, 8])
    assert torch.equal(ref[9:17], one)
    assert torch.equal(ref[8], qkv[8, 32:].double())        # a sequence of one token returns its V row
