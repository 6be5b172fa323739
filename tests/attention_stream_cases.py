"""Cases of the streaming ViT attention (csrc/attention_stream.hip: key blocks + online softmax), on top of tests/attention_cases.py:
the token counts, a torch emulation of the streaming form's rounding points with the key block as a parameter, defects such a
kernel could have, and the checks that are new with it -- all against float64 of the WHOLE tensor or against values known exactly.
Plain torch, no GPU: tests/test_gpu_attention_stream.py hands the checks the kernel, tests/test_attention_stream_cases_cpu.py the
emulation and its mutations.

A check takes `run(qkv, frames, tokens, heads)` on CPU tensors of the build's operand type and raises AssertionError with a message
that starts with the check's name."""
import functools
import math

import torch
import torch.nn.functional as F

from attention_cases import (DH, LP, assert_within_model, bits, check_vit_biased_p, check_vit_constant_v, check_vit_isolation,  # noqa: F401
                             check_vit_one_hot, check_vit_random, vit_random, vit_reference, _gen)
from vsc_hip import _lib

KB = _lib.ATTENTION_STREAM_KEY_BLOCK      # the library's key block (include/vsc_hip.h: VSC_ATTENTION_STREAM_KEY_BLOCK)
QB = 128                                  # queries per workgroup, 16 per wave

# the issue's list: every path of the encoder's presets (197, 257, 401, 577, 1370), both sides of the 320-token limit of the
# register-row kernel, multiples of 64 / 128 / 512 / 1024 and their neighbours, 2049 (17 key blocks, 17 query blocks) ...
STREAM_TOKENS = [1, 15, 17, 33, 64, 65, 128, 129, 197, 257, 320, 321, 336, 337, 383, 384, 385, 401, 511, 512, 513, 576, 577, 641, 1023,
                 1024, 1025, 1370, 2049]
# ... extended by what the key block of 128 still lacks: j KB - 1, j KB, j KB + 1 for j = 1, 2, 3
STREAM_TOKENS = sorted(set(STREAM_TOKENS) | {127, 255, 256})
assert all(j * KB + d in STREAM_TOKENS for j in (1, 2, 3) for d in (-1, 0, 1)), \
    f"STREAM_TOKENS lacks a neighbour of a multiple of the key block {KB}: extend the list"

FLT_MAX = float(torch.finfo(torch.float32).max)
SCALE = 0.125 * 1.44269504088896340736


def key_blocks(tokens, kb=KB):
    return (tokens + kb - 1) // kb


# ------------------------------------------------------------------------------------------------------------ emulation

STREAM_MUTATIONS = ("o_not_rescaled", "l_not_rescaled", "stale_max", "leak_pad_key", "drop_last_block", "mask_in_first_block")


def stream_emulate(qkv, frames, tokens, heads, kb=KB, mutation=None):
    """The rounding points of attention_stream_kernel in torch.  Per key block of kb keys: fp32 scores (pad rows of K and V are
    zeros; pad keys exist in the last block only and are masked to -inf there only), m' = max(m, block maximum) with m starting at
    -FLT_MAX, alpha = exp2((m - m') c), O and l multiplied by alpha once, P = exp2(s c - m' c) rounded to the operand type, O += P V,
    l += sum of the rounded P; at the end O / l rounded to the operand type.  mutation: one of STREAM_MUTATIONS."""
    dtype = qkv.dtype
    q, k, v = qkv.float().reshape(frames, tokens, 3, heads, DH).permute(2, 0, 3, 1, 4)
    nb = key_blocks(tokens, kb)
    k, v = F.pad(k, (0, 0, 0, nb * kb - tokens)), F.pad(v, (0, 0, 0, nb * kb - tokens))
    scale = torch.tensor(SCALE, dtype=torch.float32)
    m = torch.full((frames, heads, tokens, 1), -FLT_MAX)
    l = torch.zeros(frames, heads, tokens, 1)
    o = torch.zeros(frames, heads, tokens, DH)
    idx = torch.arange(kb)
    for b in range(nb):
        last = b == nb - 1
        if mutation == "drop_last_block" and last:
            continue
        s = q @ k[..., b * kb:(b + 1) * kb, :].transpose(-1, -2)
        if mutation == "mask_in_first_block":
            masked = (idx >= tokens - (nb - 1) * kb) if b == 0 else torch.zeros(kb, dtype=torch.bool)
        else:
            masked = (b * kb + idx >= tokens) if last else torch.zeros(kb, dtype=torch.bool)
            if mutation == "leak_pad_key" and last and tokens < nb * kb:
                masked[tokens - b * kb] = False
        s = s.masked_fill(masked, float("-inf"))
        m_new = torch.maximum(m, s.amax(-1, keepdim=True))
        if mutation == "stale_max" and b > 0:
            m_new = m
        alpha = torch.exp2((m - m_new) * scale)
        p = torch.exp2(s * scale - m_new * scale).to(dtype).float()
        o = o * (1.0 if mutation == "o_not_rescaled" else alpha) + p @ v[..., b * kb:(b + 1) * kb, :]
        l = l * (1.0 if mutation == "l_not_rescaled" else alpha) + p.sum(-1, keepdim=True)
        m = m_new
    return (o / l).permute(0, 2, 1, 3).reshape(frames * tokens, heads * DH).to(dtype)


# ------------------------------------------------------------------------------------------------------------ random data

@functools.lru_cache(maxsize=None)
def _random_case(precision, tokens, frames, heads, std):
    """operands and float64 reference of the whole tensor, computed once and shared (nobody writes to them); the operands are those
    of attention_cases.check_vit_random"""
    qkv = vit_random(1000 * tokens + int(std), frames, tokens, heads, std, LP[precision]["dtype"])
    return (qkv,) + vit_reference(qkv, frames, tokens, heads)


def check_stream_random(run, precision, tokens, frames=2, heads=2, kb=KB, report=None):
    """check_vit_random's operands, error model and mean bound, with the one further term of the streaming form:
        |got - ref| <= 4 u A + tokens eta Vmax + ceil(tokens / kb) 2^-23 A
    -- one fp32 rounding of O and of l per key block (the multiplication by alpha).  A priori; nothing measured is in it."""
    lp = LP[precision]
    extra = 1.0 + key_blocks(tokens, kb) * 2.0 ** -23 / (4.0 * lp["u"])       # 4 u (A extra) = 4 u A + blocks 2^-23 A
    for std in (1.0, 2.0):
        qkv, ref, A, vmax = _random_case(precision, tokens, frames, heads, std)
        got = run(qkv, frames, tokens, heads)
        assert_within_model(got, ref, A * extra, vmax, tokens, lp["u"], lp["eta"], name="random", report=report)
        mean = float((got.double() - ref).abs().mean())
        assert mean < (2e-3 if precision == "bf16" else 2e-3 / 8), f"random: mean |d| {mean:.2e} at {tokens} tokens, std {std}"


# ------------------------------------------------------------------------------------------------------------ staircase

def power_of_two_vectors(frames, heads):
    """[frames, heads, 64] vectors +-2^e, e in -12 .. 11 (normal in fp16 and bf16), the exponent stepping with the column and the
    (frame, head): multiplying by such a component commutes with every rounding of the kernel."""
    idx = torch.arange(frames * heads).reshape(frames, heads, 1)
    d = torch.arange(DH)
    e = (d + 5 * idx) % 24 - 12
    return (1.0 - 2.0 * ((d + idx) % 2)) * torch.exp2(e.float())


def staircase(seed, frames, tokens, heads, dtype, rising, kb=KB):
    """Logits step by 16 from one key block to the next (q[0] = 8, k[0] = +-16 block: 8 * 16 block / 8), plus N(0, 0.25) from the
    other 63 dimensions (q = 1, k = 0.25 N(0, 1)): rising, every block raises the maximum and alpha is about e^-16; falling, the
    first block holds it and every later alpha is 1.  V rows are the (frame, head)'s power-of-two vector c.  -> (qkv, expected)"""
    x = torch.empty(frames, tokens, 3, heads, DH)
    x[:, :, 0] = 1.0
    x[:, :, 0, :, 0] = 8.0
    x[:, :, 1] = 0.25 * torch.randn(frames, tokens, heads, DH, generator=_gen(seed))
    blk = (torch.arange(tokens) // kb).float()
    x[:, :, 1, :, 0] = ((16.0 if rising else -16.0) * blk)[None, :, None]
    c = power_of_two_vectors(frames, heads)
    x[:, :, 2] = c[:, None]
    want = c[:, None].expand(frames, tokens, heads, DH).reshape(frames * tokens, heads * DH)
    return x.reshape(frames * tokens, 3 * heads * DH).to(dtype), want.to(dtype)


def check_stream_staircase(run, precision, tokens, frames=2, heads=2, kb=KB):
    """rising and falling staircase: O = c l whatever the rescale pattern (a power of two commutes with the rounding of alpha O
    against alpha l), so every query returns c, bit for bit.  An O or an l that misses a rescale is off by e^16 per block."""
    for rising in (True, False):
        qkv, want = staircase(23 + tokens, frames, tokens, heads, LP[precision]["dtype"], rising, kb)
        got = run(qkv, frames, tokens, heads)
        bad = int((bits(got) != bits(want)).sum())
        assert bad == 0, f"staircase: {bad} elements differ from c at {tokens} tokens ({'rising' if rising else 'falling'}, key block {kb})"


# ------------------------------------------------------------------------------------------------------------ spike per block

def spike_positions(tokens, kb=KB):
    """-> (queries, keys): a query of the first, a middle and the last 16-query tile; a key of the first, a middle and the last key block"""
    last = tokens - 1
    qtiles, nb = (tokens + 15) // 16, key_blocks(tokens, kb)
    queries = sorted({min(3, last), min(16 * (qtiles // 2) + 5, last), last})
    keys = sorted({min(7, last), min((nb // 2) * kb + 9, last), last, (nb - 1) * kb})
    return queries, keys


def check_stream_spike(run, precision, tokens, frames=2, heads=2, kb=KB):
    """attention_cases.vit_one_hot with several queries at once: N(0, 0.3) rows; the chosen queries and ONE key are 6.0 in every
    head, a logit of 288 against a few units.  Each of those rows is V[key], bit for bit: what earlier blocks accumulated is
    flushed by alpha = exp2(-400) = 0, and every later block adds exp2(-400) = 0."""
    d = heads * DH
    queries, keys = spike_positions(tokens, kb)
    base = torch.randn(frames, tokens, 3, heads, DH, generator=_gen(11 + tokens)) * 0.3
    for key in keys:
        x = base.clone()
        x[:, queries, 0] = 6.0
        x[:, key, 1] = 6.0
        qkv = x.reshape(frames * tokens, 3 * d).to(LP[precision]["dtype"])
        got = run(qkv, frames, tokens, heads).reshape(frames, tokens, d)
        want = qkv.reshape(frames, tokens, 3 * d)[:, key, 2 * d:]
        for query in queries:
            assert torch.isfinite(got[:, query].float()).all(), f"spike: query {query} is not finite with the spike on key {key} at {tokens} tokens"
            assert torch.equal(bits(got[:, query]), bits(want)), f"spike: query {query} does not return V[{key}] at {tokens} tokens (key block {kb})"


def check_stream_all(run, precision, tokens, kb=KB, report=None):
    """every check of a token count"""
    check_stream_random(run, precision, tokens, kb=kb, report=report)
    check_vit_constant_v(run, precision, tokens)
    check_vit_biased_p(run, precision, tokens)
    check_stream_staircase(run, precision, tokens, kb=kb)
    check_stream_spike(run, precision, tokens, kb=kb)
