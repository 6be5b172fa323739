"""Cases of the three attention families (ViT: csrc/attention.hip, Swin-V2 windows: csrc/swin.hip, fp32: csrc/conv.hip):
float64 references, seeded input builders, the error model, plain-torch emulations of the kernels' rounding points and the
checks themselves.  Plain torch, no GPU: tests/test_gpu_attention.py hands the checks a function that launches a kernel,
tests/test_attention_cases_cpu.py hands them the emulation (every check passes) and broken emulations (the check named for
each mutation fails), so a bound that the arithmetic alone could not meet, or a check that sees nothing, shows without a GPU.

A check takes `run`, a callable with the argument list of the matching vsc_hip.ops wrapper on CPU tensors of the build's
operand type, and raises AssertionError with a message that starts with the check's name.

Operand types: u = unit roundoff (2^-8 bf16, 2^-11 fp16), eta = the smallest subnormal a probability can underflow to (fp16: 2^-24;
bf16 has fp32's exponent range: 0)."""
import functools
import math

import torch
import torch.nn.functional as F

from oracle import swin_oracle

LP = {"bf16": dict(dtype=torch.bfloat16, u=2.0 ** -8, eta=0.0), "fp16": dict(dtype=torch.float16, u=2.0 ** -11, eta=2.0 ** -24)}
DH = 64         # ViT head_dim
WHD = 32        # Swin-V2 head_dim

# every key-tile edge (32), every 16-key sub-tile edge and every step of the query tiles per wave (128 queries per round of 8 waves)
VIT_TOKENS = [1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 96, 97, 127, 128, 129, 160, 161, 191, 192, 193, 197, 224, 225, 255, 256,
              257, 272, 273, 288, 289, 304, 319, 320]
# key tiles KT = ceil(tokens / 32) -> the token counts above that launch attention_kernel<KT, .>
VIT_KT_CASES = {kt: [t for t in VIT_TOKENS if (t + 31) // 32 == kt] for kt in range(1, 11)}


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(int(seed))


def constant_vectors(shape_prefix, dim, salt=0):
    """[*shape_prefix, dim] vectors of +-(2 + k / 8), k = 0..15: five significant bits (exact in bf16 and fp16), every
    magnitude in [2, 4) -- an output that lost its V rows to a zero pad key is off by more than 2 -- and different for every
    index of the prefix (neighbouring indices differ in every component)."""
    idx = torch.arange(int(math.prod(shape_prefix))).reshape(*shape_prefix, 1)
    d = torch.arange(dim)
    k = (5 * d + 4 * idx + salt) % 16
    sign = 1.0 - 2.0 * ((d + idx) % 2)
    return sign * (2.0 + k.float() / 8.0)


# ------------------------------------------------------------------------------------------------------------ error model

def assert_within_model(got, ref, A, Vmax, tokens, u, eta, name="random", report=None):
    """|got - ref| <= 4 u A + tokens eta Vmax element-wise; A = sum_j p_j |v_j|.  P is rounded once (u), the denominator is
    the sum of the rounded P (u), the output is rounded once (u), and one more u covers the fp32 accumulation order and the
    hardware exp2 / rcp; a probability that underflows moves the output by at most eta Vmax.  -> worst error / bound."""
    err = (got.double() - ref).abs()
    bound = 4.0 * u * A + tokens * eta * Vmax
    ratio = float((err / bound.clamp_min(1e-300)).max())
    if report is not None:       # the figure is on record before anything is asserted
        report.append((name, tokens, round(ratio, 4), float(err.mean())))
    assert torch.isfinite(got.float()).all(), f"{name}: non-finite output"
    assert bool((err <= bound).all()), f"{name}: error {ratio:.3f} x the bound 4 u A + tokens eta Vmax at {tokens} tokens"
    return ratio


# ------------------------------------------------------------------------------------------------------------ ViT attention

def vit_reference(qkv, frames, tokens, heads):
    """float64 softmax(q k^T / 8) v on the given (already rounded) operands -> (ref, A, Vmax), each [frames * tokens, heads * 64];
    Vmax = max |v| of the (frame, head)."""
    q, k, v = qkv.double().reshape(frames, tokens, 3, heads, DH).permute(2, 0, 3, 1, 4)
    p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(DH), -1)
    back = lambda x: x.permute(0, 2, 1, 3).reshape(frames * tokens, heads * DH)
    vmax = v.abs().amax(dim=(-1, -2), keepdim=True).expand_as(v)
    return back(p @ v), back(p @ v.abs()), back(vmax)


def vit_random(seed, frames, tokens, heads, std, dtype):
    return (torch.randn(frames * tokens, 3 * heads * DH, generator=_gen(seed)) * std).to(dtype)


def vit_constant_v(seed, frames, tokens, heads, dtype):
    """Every V row of a (frame, head) is the same vector c; Q = +3, K = -3 + 0.25 noise: every true logit is about -72, so a
    zero pad key (logit 0, V row 0) that leaks into the softmax takes the whole output.  -> (qkv, expected output)"""
    x = torch.empty(frames, tokens, 3, heads, DH)
    x[:, :, 0] = 3.0
    x[:, :, 1] = -3.0 + 0.25 * torch.randn(frames, tokens, heads, DH, generator=_gen(seed))
    c = constant_vectors((frames, heads), DH)
    x[:, :, 2] = c[:, None]
    want = c[:, None].expand(frames, tokens, heads, DH).reshape(frames * tokens, heads * DH)
    return x.reshape(frames * tokens, 3 * heads * DH).to(dtype), want.to(dtype)


def vit_one_hot(seed, frames, tokens, heads, query, key, dtype):
    """N(0, 0.3) rows; q of `query` and k of `key` are 6.0 in every head: that logit is 64 * 36 / 8 = 288, every other one of the
    row is a few units, so P is exactly one-hot (e^-280 is zero in both types) and the output row is V[key], bit for bit."""
    x = (torch.randn(frames, tokens, 3, heads, DH, generator=_gen(seed)) * 0.3)
    x[:, query, 0] = 6.0
    x[:, key, 1] = 6.0
    return x.reshape(frames * tokens, 3 * heads * DH).to(dtype)


def one_hot_positions(tokens):
    last = tokens - 1
    return sorted({(0, last), (last, 0), (last, last), (16 * (last // 16), last)})


def biased_logit(u):
    """t = k / 128 in [0.5, 1.5] (8 significant bits: exact in both types) whose e^-t lies furthest above its rounded value
    while staying 10 % of a half spacing clear of the tie: -> (t, relative rounding error of e^-t, > 0)."""
    best = None
    for k in range(64, 193):
        t = k / 128.0
        e = math.exp(-t)
        half = 2.0 ** math.floor(math.log2(e)) * u          # half the spacing of the type at e
        down = e - math.floor(e / (2 * half)) * (2 * half)   # distance to the representable value below
        if down < 0.9 * half and (best is None or down / e > best[1]):
            best = (t, down / e)
    return best


def vit_biased_p(frames, tokens, heads, dtype, u):
    """The row sum must be the sum of the ROUNDED probabilities (attention.hip: "the context is an exact weighted mean of the V
    rows").  Key 0 has logit 0, every other key the same logit -t whose e^-t rounds DOWN by the relative amount r (biased_logit);
    V rows are all c with components +-2 and +-4.  With the sum of the rounded P the output is c; with the sum of the unrounded
    e it is c (1 - r m / (1 + m)), m = (tokens - 1) e^-t.  The value below a power of two is u / 2 away (relative), and from 15
    tokens on r m / (1 + m) is 20 % past that (test_biased_p_construction_has_margin): the output drops to the next value
    down.  -> (qkv, expected)"""
    t, _ = biased_logit(u)
    x = torch.zeros(frames, tokens, 3, heads, DH)
    x[:, :, 0, :, 0] = 8.0
    x[:, 1:, 1, :, 0] = -t
    idx = torch.arange(frames * heads).reshape(frames, heads, 1)
    d = torch.arange(DH)
    c = (1.0 - 2.0 * ((d + idx) % 2)) * (2.0 + 2.0 * ((d // 2 + idx) % 2))
    x[:, :, 2] = c[:, None]
    want = c[:, None].expand(frames, tokens, heads, DH).reshape(frames * tokens, heads * DH)
    return x.reshape(frames * tokens, 3 * heads * DH).to(dtype), want.to(dtype)


def vit_emulate(qkv, frames, tokens, heads, mutation=None):
    """The rounding points of attention_kernel in torch: fp32 scores over 32 * ceil(tokens / 32) keys (pad rows of K and V are
    zero, pad keys masked to -inf), exp2 with the folded scale, P rounded to the operand type, the row sum taken from the
    rounded P, the output rounded to the operand type.  mutation: one of VIT_MUTATIONS, a defect a kernel could have."""
    dtype = qkv.dtype
    q, k, v = qkv.float().reshape(frames, tokens, 3, heads, DH).permute(2, 0, 3, 1, 4)
    tp = (tokens + 31) // 32 * 32
    k, v = F.pad(k, (0, 0, 0, tp - tokens)), F.pad(v, (0, 0, 0, tp - tokens))
    if mutation == "swap_v_rows":
        v = v.clone()
        v[..., [0, tokens - 1], :] = v[..., [tokens - 1, 0], :]
    valid = tokens - 1 if mutation == "mask_off_by_one" else tokens
    masked = torch.arange(tp) >= valid
    if mutation == "leak_pad_key" and tokens < tp:
        masked[tokens] = False
    s = (q @ k.transpose(-1, -2)).masked_fill(masked, float("-inf"))
    scale = torch.tensor(0.125 * 1.44269504088896340736, dtype=torch.float32)
    mx = s.amax(-1, keepdim=True)
    e = torch.exp2(s * scale - mx * scale)
    p = e.to(dtype).float()
    den = (e if mutation == "sum_before_rounding" else p).sum(-1, keepdim=True)
    o = (p @ v) / den
    return o.permute(0, 2, 1, 3).reshape(frames * tokens, heads * DH).to(dtype)


VIT_MUTATIONS = ("leak_pad_key", "mask_off_by_one", "swap_v_rows", "sum_before_rounding")


def check_vit_random(run, precision, tokens, frames=2, heads=2, report=None):
    """(a): N(0, 1) and N(0, 2) operands against float64 within the error model, and the mean error."""
    lp = LP[precision]
    for std in (1.0, 2.0):
        qkv = vit_random(1000 * tokens + int(std), frames, tokens, heads, std, lp["dtype"])
        ref, A, vmax = vit_reference(qkv, frames, tokens, heads)
        got = run(qkv, frames, tokens, heads)
        assert_within_model(got, ref, A, vmax, tokens, lp["u"], lp["eta"], name="random", report=report)
        mean = float((got.double() - ref).abs().mean())
        assert mean < (2e-3 if precision == "bf16" else 2e-3 / 8), f"random: mean |d| {mean:.2e} at {tokens} tokens, std {std}"


def check_vit_constant_v(run, precision, tokens, frames=2, heads=2):
    """(b): the output equals c for every query of every (frame, head), bit for bit."""
    qkv, want = vit_constant_v(7 + tokens, frames, tokens, heads, LP[precision]["dtype"])
    got = run(qkv, frames, tokens, heads)
    bad = int((bits(got) != bits(want)).sum())
    assert bad == 0, f"constant_v: {bad} elements differ from c at {tokens} tokens (max |d| {float((got.float() - want.float()).abs().max()):.3g})"


def check_vit_one_hot(run, precision, tokens, frames=2, heads=2):
    """(b): a dominant (query, key) pair on the first / last token and on the last query tile: the row is that V row, bit for bit."""
    d = heads * DH
    for query, key in one_hot_positions(tokens):
        qkv = vit_one_hot(11 + tokens, frames, tokens, heads, query, key, LP[precision]["dtype"])
        got = run(qkv, frames, tokens, heads).reshape(frames, tokens, d)
        want = qkv.reshape(frames, tokens, 3 * d)[:, key, 2 * d:]
        assert torch.equal(bits(got[:, query]), bits(want)), f"one_hot: query {query} does not return V[{key}] at {tokens} tokens"


def check_vit_biased_p(run, precision, tokens, frames=2, heads=2):
    """(b): the denominator is the sum of the rounded probabilities (needs >= 15 tokens: m >= 5 in vit_biased_p)."""
    if tokens < 15:
        return
    qkv, want = vit_biased_p(frames, tokens, heads, LP[precision]["dtype"], LP[precision]["u"])
    got = run(qkv, frames, tokens, heads)
    bad = int((bits(got) != bits(want)).sum())
    assert bad == 0, f"biased_p: {bad} elements differ from c at {tokens} tokens"


POISONS = ("max", "inf", "nan")


def _poison_value(kind, dtype):
    return {"max": torch.finfo(dtype).max, "inf": float("inf"), "nan": float("nan")}[kind]


def check_vit_isolation(run, precision, tokens, heads=2):
    """(c): 3 frames; frame 1 (then one head of frame 1) filled with the largest finite value, +inf and NaN: every row of the
    other frames (the other heads) keeps the bits of the clean run -- a frame's pad rows read nothing of the frame behind it."""
    frames, d = 3, heads * DH
    dtype = LP[precision]["dtype"]
    clean = vit_random(31 + tokens, frames, tokens, heads, 1.0, dtype)
    base = run(clean, frames, tokens, heads).reshape(frames, tokens, heads, DH)
    for kind in POISONS:
        x = clean.clone().reshape(frames, tokens, 3, heads, DH)
        x[1] = _poison_value(kind, dtype)
        got = run(x.reshape(frames * tokens, 3 * d), frames, tokens, heads).reshape(frames, tokens, heads, DH)
        assert torch.equal(bits(got[[0, 2]]), bits(base[[0, 2]])), f"isolation: frames 0 / 2 change when frame 1 is {kind} at {tokens} tokens"
        x = clean.clone().reshape(frames, tokens, 3, heads, DH)
        x[1, :, :, 0] = _poison_value(kind, dtype)
        got = run(x.reshape(frames * tokens, 3 * d), frames, tokens, heads).reshape(frames, tokens, heads, DH)
        keep = torch.ones(frames, heads, dtype=torch.bool)
        keep[1, 0] = False
        same = (bits(got) == bits(base)).all(dim=-1).all(dim=1)
        assert bool(same[keep].all()), f"isolation: another head changes when head 0 of frame 1 is {kind} at {tokens} tokens"


# ------------------------------------------------------------------------------------------------------- window attention

WINDOW_TOL = {"bf16": dict(rtol=2 ** -6, atol=2e-2, mean=4e-3),      # test_gpu_swin.py::test_window_attention
              "fp16": dict(rtol=2 ** -6, atol=2e-2, mean=2e-3)}      # test_gpu_fp16_operands.py::test_window_attention_with_fp16_operands


def window_cases(windows=(8, 12, 16, 24)):
    """(res, window, shift): four windows (three of them on the masked last row or column) at every shift class, and one window."""
    out = []
    for w in windows:
        out += [(2 * w, w, s) for s in (0, 1, w // 2, w - 1)] + [(w, w, 0)]
    return out


def _to_windows(x, frames, res, window, shift):        # [frames * res * res, C] -> [frames * nW, n, C]
    x = x.reshape(frames, res, res, -1)
    if shift:
        x = torch.roll(x, (-shift, -shift), (1, 2))
    return swin_oracle._windows(x, res, window)


def _from_windows(xw, frames, res, window, shift):     # inverse
    x = swin_oracle._unwindows(xw, res, window, frames)
    if shift:
        x = torch.roll(x, (shift, shift), (1, 2))
    return x.reshape(frames * res * res, -1)


def _bias_matrix(table, window):
    n = window * window
    return table[:, swin_oracle.relative_position_index(window).reshape(-1)].reshape(table.shape[0], n, n)


def window_reference(qkv, table, scale, frames, res, window, shift, heads):
    """float64 statement of WindowAttention.forward on the given operands -> (ref, A, Vmax), [frames * res * res, heads * 32]"""
    n, c = window * window, heads * WHD
    xw = _to_windows(qkv.double(), frames, res, window, shift)
    q, k, v = xw.reshape(-1, n, 3, heads, WHD).permute(2, 0, 3, 1, 4)
    attn = F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1) * scale.double().reshape(1, heads, 1, 1)
    attn = attn + _bias_matrix(table.double(), window)[None]
    if shift:
        m = swin_oracle.shift_mask(res, window, shift).double()
        attn = (attn.reshape(frames, -1, heads, n, n) + m[None, :, None]).reshape(-1, heads, n, n)
    p = torch.softmax(attn, -1)
    back = lambda o: _from_windows(o.transpose(1, 2).reshape(-1, n, c), frames, res, window, shift)
    vmax = v.abs().amax(dim=(-1, -2), keepdim=True).expand_as(v)
    return back(p @ v), back(p @ v.abs()), back(vmax)


def window_random(seed, frames, res, window, heads, dtype):
    """Operands, table and logit scales drawn exactly as tests/test_gpu_swin.py::test_window_attention draws them: its tolerances are
    stated for these scales (14.8 and 8.4 with two heads; a cosine rounded to bf16 is off by 2^-8, i.e. by scale * 2^-8 in the logit)."""
    from tools import synth
    rand = lambda s, shape, std=1.0: torch.from_numpy(synth.normalish(s, shape, std))
    qkv = rand(seed, (frames * res * res, 3 * heads * WHD)).to(dtype)
    table = 16 * torch.sigmoid(rand(7, (heads, (2 * window - 1) ** 2)))
    scale = torch.exp(torch.clamp(math.log(10.0) + rand(8, (heads,), 0.4), max=math.log(100.0)))
    return qkv, table, scale


def window_regions(res, window, shift):
    """[nW, n] region number (0..3 inside a window) of every window token, read off the oracle's shift mask; all 0 without shift."""
    nw, n = (res // window) ** 2, window * window
    if not shift:
        return torch.zeros(nw, n, dtype=torch.long)
    first = (swin_oracle.shift_mask(res, window, shift) == 0).float().argmax(-1)      # first token of the same region
    out = torch.empty(nw, n, dtype=torch.long)
    for w in range(nw):
        out[w] = torch.unique(first[w], return_inverse=True)[1]
    return out


def window_constant_v(seed, frames, res, window, shift, heads, dtype, by_region):
    """Random q and k, scale <= 10, table in [0, 16); V is one vector per (frame, window, head) -- and, by_region, per shift-mask
    region of the window (region_constant_v).  Every query then returns the vector of its own region, which is its own V row:
    a masked key holds at most e^(-100 + 36) of the row, far under half a unit of either type.  -> (qkv, table, scale, expected)"""
    g = _gen(seed)
    nw, n, c = (res // window) ** 2, window * window, heads * WHD
    qk = torch.randn(frames * res * res, 2 * c, generator=g)
    table = 16 * torch.rand(heads, (2 * window - 1) ** 2, generator=g)
    scale = 4.0 + 6.0 * torch.rand(heads, generator=g)
    reg = window_regions(res, window, shift) if by_region else torch.zeros(nw, n, dtype=torch.long)
    idx = torch.arange(frames * nw * heads).reshape(frames, nw, 1, heads) + reg[None, :, :, None]      # region r -> + r: 4 r in the pattern
    d = torch.arange(WHD)
    k = (5 * d + 4 * idx[..., None]) % 16
    vw = (1.0 - 2.0 * ((d + idx[..., None]) % 2)) * (2.0 + k.float() / 8.0)                             # [frames, nW, n, heads, 32]
    v = _from_windows(vw.reshape(frames * nw, n, c), frames, res, window, shift)
    qkv = torch.cat([qk, v], 1).to(dtype)
    return qkv, table, scale, v.to(dtype)


def window_emulate(qkv, table, scale, frames, res, window, shift, heads, bounded=False, mutation=None):
    """The rounding points of the window kernels in torch: q-hat / k-hat (1 / max(|x|, 1e-12) in fp32) rounded to the operand
    type, fp32 logits, the row maximum -- or, bounded, the head's folded upper bound scale + max(bias) -- subtracted, P and V
    rounded to bf16 in both builds, the row sum taken from the rounded P, the output rounded to the operand type."""
    dtype, n, c = qkv.dtype, window * window, heads * WHD
    xw = _to_windows(qkv.float(), frames, res, window, shift)
    q, k, v = xw.reshape(-1, n, 3, heads, WHD).permute(2, 0, 3, 1, 4)
    hat = lambda x: (x * torch.rsqrt(x.pow(2).sum(-1, keepdim=True).clamp_min(1e-24))).to(dtype).float()
    scale, table = scale.float(), table.float()
    attn = hat(q) @ hat(k).transpose(-2, -1) * scale.reshape(1, heads, 1, 1) + _bias_matrix(table, window)[None]
    mask_shift = {None: shift, "drop_shift_mask": 0, "mask_of_half_window": window // 2}[mutation]
    if mask_shift:
        m = swin_oracle.shift_mask(res, window, mask_shift)
        attn = (attn.reshape(frames, -1, heads, n, n) + m[None, :, None]).reshape(-1, heads, n, n)
    top = attn.amax(-1, keepdim=True)
    if bounded:
        bmax, bmin = table.amax(1), table.amin(1)
        ok = (2 * scale + (bmax - bmin)) <= 69.0
        top = torch.where(ok.reshape(1, heads, 1, 1), (scale + bmax).reshape(1, heads, 1, 1), top)
    p = torch.exp(attn - top).to(torch.bfloat16).float()
    o = (p @ v.to(torch.bfloat16).float()) / p.sum(-1, keepdim=True)
    return _from_windows(o.transpose(1, 2).reshape(-1, n, c), frames, res, window, shift).to(dtype)


WINDOW_MUTATIONS = ("drop_shift_mask", "mask_of_half_window")


def _assert_window_close(got, ref, precision, name, report=None):
    tol = WINDOW_TOL[precision]
    err = (got.double() - ref).abs()
    excess = float((err - (tol["atol"] + tol["rtol"] * ref.abs())).max())
    if report is not None:
        report.append((name, float(err.max()), round(excess, 5), float(err.mean())))
    assert torch.isfinite(got.float()).all(), f"{name}: non-finite output"
    assert excess <= 0, f"{name}: |d| exceeds atol {tol['atol']} + rtol 2^-6 |ref| by {excess:.3g}"
    assert float(err.mean()) < tol["mean"], f"{name}: mean |d| {float(err.mean()):.2e}"


@functools.lru_cache(maxsize=None)
def _window_random_case(precision, res, window, shift, frames, heads, zero_rows):
    """operands and float64 reference of one case, computed once and shared (nobody writes to them)"""
    qkv, table, scale = window_random(res + shift, frames, res, window, heads, LP[precision]["dtype"])
    if zero_rows:
        c, t = heads * WHD, res * res
        for f in range(frames):
            qkv[[f * t, f * t + 5, f * t + t - 1], :c] = 0             # q rows: first, last, one inside
            qkv[[f * t + 1, f * t + 5, f * t + res + 2], c:2 * c] = 0  # k rows, one of them a zero-q token as well
    ref, _, _ = window_reference(qkv, table, scale, frames, res, window, shift, heads)
    return qkv, table, scale, ref


def check_window_random(run, precision, res, window, shift, frames=2, heads=2, bounded=False, report=None):
    """(e): random operands against float64 with the tolerances the existing window tests state."""
    qkv, table, scale, ref = _window_random_case(precision, res, window, shift, frames, heads, False)
    _assert_window_close(run(qkv, table, scale, frames, res, window, shift, heads, bounded), ref, precision, "window_random", report)


def check_window_constant_v(run, precision, res, window, shift, frames=2, heads=2, bounded=False, by_region=True):
    """(e): region_constant_v (by_region) / constant_v per window: every query returns its own V row, bit for bit."""
    name = "region_constant_v" if by_region else "window_constant_v"
    qkv, table, scale, want = window_constant_v(200 * window + shift + res, frames, res, window, shift, heads, LP[precision]["dtype"], by_region)
    got = run(qkv, table, scale, frames, res, window, shift, heads, bounded)
    bad = int((bits(got) != bits(want)).sum())
    assert bad == 0, f"{name}: {bad} elements differ from the region's vector (window {window}, res {res}, shift {shift}, bounded {bounded})"


def check_window_zero_rows(run, precision, res, window, shift, frames=2, heads=2, bounded=False, report=None):
    """(e): all-zero q rows and k rows (F.normalize's eps: q-hat = 0, the logits are the bias alone): finite, and the float64
    reference within the random-data tolerance."""
    qkv, table, scale, ref = _window_random_case(precision, res, window, shift, frames, heads, True)
    _assert_window_close(run(qkv, table, scale, frames, res, window, shift, heads, bounded), ref, precision, "window_zero_rows", report)


# --------------------------------------------------------------------------------------------------------- fp32 attention

F32_TOKENS = (1, 2, 63, 64, 65, 255, 256, 257, 1000)
F32_HEAD_DIMS = (1, 3, 48, 64, 65, 100, 128)
F32_HEADS = (1, 3)
EPS32 = 2.0 ** -24


def f32_reference(qkv, heads, head_dim, row_offsets):
    """float64 softmax(q k^T / sqrt(head_dim)) v of sequences rows row_offsets[z] .. row_offsets[z + 1] -> (ref, bound); rows outside
    every sequence are NaN in both.  The bound, per output element, first order in eps = 2^-24 (gamma_n = n eps):
        score a_j = fl(sum_d q_d k_jd) * fl(rsqrt(dh)): |da_j| <= gamma_(dh + 2) S_j,  S_j = sum_d |q_d k_jd| / sqrt(dh)
        e_j = expf(a_j - max): relative error <= da_j + da_max + (|a_j - max| + 2) eps  =: E_j  (the subtraction, a 2-ulp expf)
        w_j = e_j / sum e: relative error <= 2 max_j E_j + gamma_tokens  (the sum; the division and the final product in the 4 eps)
        out = sum_j w_j v_j in fp32: gamma_tokens A more,  A = sum_j w_j |v_j|
    => |out - ref| <= (2 E + 2 gamma_tokens + 4 eps) A + tokens 2^-126 Vmax,  E = max_j [2 gamma_(dh + 2) max_j S_j + (|a_j - max| + 2) eps]
    over the keys that carry weight (w_j >= 2^-126: a key below that contributes at most 2^-126 |v_j|, the last term)."""
    width = heads * head_dim
    rows = qkv.shape[0]
    ref = torch.full((rows, width), float("nan"), dtype=torch.float64)
    bound = torch.full((rows, width), float("nan"), dtype=torch.float64)
    x = qkv.double()
    for z in range(len(row_offsets) - 1):
        r0, r1 = int(row_offsets[z]), int(row_offsets[z + 1])
        if r1 == r0:
            continue
        n = r1 - r0
        q, k, v = x[r0:r1].reshape(n, 3, heads, head_dim).permute(1, 2, 0, 3)
        a = q @ k.transpose(-1, -2) / math.sqrt(head_dim)
        s_abs = (q.abs() @ k.abs().transpose(-1, -2) / math.sqrt(head_dim)).amax(-1, keepdim=True)
        w = torch.softmax(a, -1)
        gap = (a.amax(-1, keepdim=True) - a).masked_fill(w < 2.0 ** -126, 0.0).amax(-1, keepdim=True)
        e = 2 * (head_dim + 2) * EPS32 * s_abs + (gap + 2) * EPS32
        A = w @ v.abs()
        b = (2 * e + 2 * n * EPS32 + 4 * EPS32) * A + n * 2.0 ** -126 * v.abs().amax()
        ref[r0:r1] = (w @ v).permute(1, 0, 2).reshape(n, width)
        bound[r0:r1] = b.permute(1, 0, 2).reshape(n, width)
    return ref, bound


def f32_emulate(qkv, heads, head_dim, row_offsets):
    """attention_f32_kernel's arithmetic as plain fp32 torch (its own summation orders)"""
    width = heads * head_dim
    out = torch.full((qkv.shape[0], width), float("nan"), dtype=torch.float32)
    for z in range(len(row_offsets) - 1):
        r0, r1 = int(row_offsets[z]), int(row_offsets[z + 1])
        if r1 == r0:
            continue
        n = r1 - r0
        q, k, v = qkv[r0:r1].float().reshape(n, 3, heads, head_dim).permute(1, 2, 0, 3)
        a = (q @ k.transpose(-1, -2)) * torch.rsqrt(torch.tensor(float(head_dim)))
        e = torch.exp(a - a.amax(-1, keepdim=True))
        o = (e @ v) * (1.0 / e.sum(-1, keepdim=True))
        out[r0:r1] = o.permute(1, 0, 2).reshape(n, width)
    return out


def f32_random(seed, rows, heads, head_dim):
    return torch.randn(rows, 3 * heads * head_dim, generator=_gen(seed))


def check_f32(run, tokens, heads, head_dim, report=None):
    """(f): one sequence of N(0, 1) rows against float64 within f32_reference's bound.  run(qkv, tokens, heads, head_dim) -> out"""
    qkv = f32_random(tokens * 131 + head_dim * 7 + heads, tokens, heads, head_dim)
    ref, bound = f32_reference(qkv, heads, head_dim, [0, tokens])
    got = run(qkv, tokens, heads, head_dim)
    ratio = float(((got.double() - ref).abs() / bound).max())
    if report is not None:
        report.append((tokens, heads, head_dim, round(ratio, 4)))
    assert torch.isfinite(got).all(), f"f32: non-finite output at {tokens} tokens, head_dim {head_dim}"
    assert ratio <= 1.0, f"f32: error {ratio:.3f} x the bound at {tokens} tokens, {heads} heads, head_dim {head_dim}"
    return ratio
