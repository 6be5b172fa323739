"""tests/attention_stream_cases.py held to itself, without a GPU: a torch emulation of the streaming kernel's rounding points passes
every check that tests/test_gpu_attention_stream.py runs on the kernel, at every token count and at other key blocks than the
library's; an emulation with one defect fails the check that is there for that defect.  And what the streaming attention adds
outside the kernel: the presets, and the constants that the header, the binding and the Python mirror must agree on."""
import os
import re

import pytest

import attention_stream_cases as sc

PRECISIONS = ("bf16", "fp16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _emu(kb=sc.KB, mutation=None):
    return lambda qkv, frames, tokens, heads: sc.stream_emulate(qkv, frames, tokens, heads, kb, mutation)


def test_token_list_covers_the_key_block_edges():
    assert sc.KB == 128
    for j in (1, 2, 3):
        assert {j * sc.KB - 1, j * sc.KB, j * sc.KB + 1} <= set(sc.STREAM_TOKENS)
    assert {320, 321, 577, 401, 1370, 2049} <= set(sc.STREAM_TOKENS)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tokens", sc.STREAM_TOKENS)
def test_clean_emulation_passes_every_check(precision, tokens):
    report = []
    try:
        sc.check_stream_all(_emu(), precision, tokens, report=report)
    finally:
        print(f"stream emulation {precision}: (check, tokens, worst error / bound, mean |d|) {report}")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tokens", [33, 577, 1025])
def test_clean_emulation_is_isolated(precision, tokens):
    sc.check_vit_isolation(_emu(), precision, tokens)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kb", [32, 64, 256])
def test_clean_emulation_at_other_key_blocks(precision, kb):
    """the checks hold for the streaming FORM, not for one block size: the staircase and the spikes follow the block they are given"""
    for tokens in (kb - 1, kb + 1, 3 * kb, 577):
        sc.check_stream_random(_emu(kb), precision, tokens, kb=kb)
        sc.check_vit_constant_v(_emu(kb), precision, tokens)
        sc.check_vit_biased_p(_emu(kb), precision, tokens)
        sc.check_stream_staircase(_emu(kb), precision, tokens, kb=kb)
        sc.check_stream_spike(_emu(kb), precision, tokens, kb=kb)


MUTATION_CASES = [
    ("o_not_rescaled", sc.check_stream_staircase, "staircase", 129),
    ("o_not_rescaled", sc.check_stream_staircase, "staircase", 577),
    ("l_not_rescaled", sc.check_stream_staircase, "staircase", 129),
    ("l_not_rescaled", sc.check_stream_staircase, "staircase", 577),
    ("stale_max", sc.check_stream_spike, "spike", 257),
    ("stale_max", sc.check_stream_spike, "spike", 577),
    ("leak_pad_key", sc.check_vit_constant_v, "constant_v", 127),
    ("leak_pad_key", sc.check_vit_constant_v, "constant_v", 577),
    ("drop_last_block", sc.check_stream_spike, "spike", 129),
    ("drop_last_block", sc.check_stream_spike, "spike", 577),
    ("mask_in_first_block", sc.check_vit_constant_v, "constant_v", 129),
    ("mask_in_first_block", sc.check_vit_constant_v, "constant_v", 577),
]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("mutation,check,name,tokens", MUTATION_CASES)
def test_mutation_is_caught_by_its_check(precision, mutation, check, name, tokens):
    assert mutation in sc.STREAM_MUTATIONS
    check(_emu(), precision, tokens)
    with pytest.raises(AssertionError, match=f"^{name}:"):
        check(_emu(mutation=mutation), precision, tokens)


def test_every_mutation_has_a_case():
    assert {m for m, *_ in MUTATION_CASES} == set(sc.STREAM_MUTATIONS)


def test_presets_hold_the_long_models():
    from vsc_hip.config import PRESETS, aligned_batch
    want = {"vit_b16_384": 577, "clip_vit_l14_336": 577, "tiny_long": 577, "tiny_clip_long": 401}
    assert {n: PRESETS[n].tokens for n in want} == want
    b, c = PRESETS["vit_b16_384"], PRESETS["clip_vit_l14_336"]
    assert (b.image_size, b.patch_size, b.width, b.layers, b.heads, b.ln_eps, b.pool, b.out_dim) == (384, 16, 768, 12, 12, 1e-12, "gem", 512)
    assert (c.image_size, c.patch_size, c.width, c.layers, c.heads, c.pre_ln, c.act, c.pool, c.out_dim) == (336, 14, 1024, 24, 16, True, "quick_gelu", "cls", 0)
    assert PRESETS["tiny_long"].image_size == 384 and PRESETS["tiny_clip_long"].image_size == 320
    for n in want:
        assert PRESETS[n].name == n and PRESETS[n].head_dim == 64
    assert aligned_batch(577) == 113


def test_header_binding_and_mirror_agree():
    import ctypes
    from vsc_hip import _lib
    text = open(os.path.join(ROOT, "include", "vsc_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+VSC_ATTENTION_STREAM_(KEY_BLOCK|MAX_TOKENS)\s+(\d+)", text)}
    assert defs == {"KEY_BLOCK": _lib.ATTENTION_STREAM_KEY_BLOCK, "MAX_TOKENS": _lib.ATTENTION_STREAM_MAX_TOKENS}
    assert defs["MAX_TOKENS"] >= 4096 and defs["KEY_BLOCK"] == sc.KB
    # the stream is the FIRST argument: (stream, qkv, out, frames, tokens, heads)
    decl = re.search(r"int\s+vsc_attention_stream_bf16\s*\(([^)]*)\)", text).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == ["void *stream", "const uint16_t *qkv_dev", "uint16_t *out_dev", "int32_t frames", "int32_t tokens", "int32_t heads"]
    res, argtypes = _lib.SIGNATURES["vsc_attention_stream_bf16"]
    assert res is ctypes.c_int32 and argtypes == [ctypes.c_void_p] * 3 + [ctypes.c_int32] * 3
    # the switch is in the option table
    common = open(os.path.join(ROOT, "vsc22-submission_amd", "csrc", "common.h")).read()
    assert re.search(r"X\(ATTN_LONG\)", common)
