"""Cases, references and checks for the GEMM kernels of csrc/gemm_bf16.hip (tests/test_gpu_gemm.py runs them on the kernels,
tests/test_gemm_cases_cpu.py on a torch emulation of the kernels' rounding points and on that emulation with one defect).  No GPU
is needed to import this; every function takes the device its tensors live on.

A case is (kernel, m, n, k, switches): the kernel csrc/gemm_plan.h picks for the shape on 256 CUs, without a switch (default route)
or under the library's diagnostic switches (forced route: the only way to V2_A and to short-K V3).  m is one row past whole
tiles; n ends in an 8-column (V1: 4-column) tile unless the row says otherwise.

Three checks:

A  check_exact.  Small integer operands (|a|, |w| <= amp, bias in halves, residual / pos integers): K amp^2 < 2^24, so every
   product and every partial sum is exact in fp32 whatever the order, and the fp32 write-outs must equal the float64 result bit for
   bit, the 16-bit one that result rounded once to nearest even.  amp grows as K shrinks (int_amp) so that the results reach past
   the operand type's integers: at least 10 % of them are not representable (ties included) and all stay below 65504 -- asserted
   on the reference alone in test_gemm_cases_cpu.py.  GELU / QGELU of the same operands: every plan gives V1's bits
   (check_same_bits); V1 itself goes through B.

B  check_bound.  A ~ N(0, 1), W ~ N(0, 1 / K), bias ~ N(0, 0.5^2), residual, pos ~ N(0, 1), element-wise over the whole output:

       |got - y64| <= u |y64| + 2 K 2^-24 (|A| |W|^T) + e_epi            u = 2^-8 (bf16), 2^-11 (fp16), 0 (fp32 outputs)

   The accumulation term is that of test_conv2d_against_float64_of_the_same_operands: products of 16-bit operands are exact in
   fp32, K additions round by 2^-24 of a partial sum that sum |a||w| bounds, the factor 2 covers the pipe's internal order.
   e_epi, derived (epilogue_error):
     every fp32 addition of the write-out (bias; residual; pos) rounds its result by 2^-24; written with 2^-23 per addition of
       the magnitudes that enter it, which also covers the second-order terms;
     the store rounds the ERRONEOUS value, not y64: u times everything above; fp16 results below 2^-14 are subnormal and round by
       2^-25 absolutely (GELU of -4.5 is -1.5e-5);
     GELU: 1.13 (accumulation term + additions) + 4.3e-5 + 3.5e-6 |z| -- the polynomial's error against erf is asserted in
       tests/test_gelu_poly.py, 1.13 bounds |gelu'| (1.129 at z = 1.41);
     QGELU: the write-out is quick_gelu() of gemm_bf16.hip, `x * rcp(1.0f + exp2(x * -2.45546696f))`: one v_mul (2^-24), v_exp_f32
       (1 ulp = 2^-23), one v_add (2^-24), v_rcp_f32 (1 ulp), one v_mul (2^-24).  The rounded exponent x c (1 + d), c itself
       rounded, moves exp2 by ln 2 |x c| 2^-23 = 1.702 |x| 2^-23 relatively; 1 + e inherits e / (1 + e) = 1 - s of it
       (s = the sigmoid), so the result moves by |x| s (1 - s) 1.702 |x| 2^-23 <= 0.28 * 2^-23 absolutely (s^2 / (1 + e^s) peaks
       at 0.48 for s = 1.702 |x| = 2.2) plus (2^-23 + 2^-23 + 2^-24 + 2^-24) = 3 * 2^-23 of |y|.  With |quick_gelu'| <= 1.1:
       e_epi = 1.1 (accumulation term + additions) + 2^-21 |y| + 2^-24.
   On the CPU the plain fp32 emulation reaches 0.96 - 1.00 of the bf16 bound: the store's half ulp saturates u |y64|.

C  check_isolation.  One row of A at a tile boundary and the one row of the last ragged tile (then, separately, two such rows of W)
   are filled with the operand type's largest finite value, +inf, NaN: exactly those output rows (columns) change, every other
   element keeps the bits of the clean run.

emulate() states the kernels' rounding points in torch: fp32 accumulation in 64-wide K chunks, the write-out's arithmetic in fp32
(the GELU polynomial with the coefficients of csrc/gelu_poly.h), one round-to-nearest-even store.  MUTATIONS are the defects the
checks are there for."""
import math
import os
import re
from dataclasses import dataclass

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPI = {"BF16": 0, "GELU_BF16": 1, "QGELU_BF16": 2, "RESADD_F32": 3, "PATCH_F32": 4, "F32": 5}
EPILOGUES = tuple(EPI)
EXACT_EPILOGUES = ("BF16", "RESADD_F32", "PATCH_F32", "F32")      # check A; the two activations: check_same_bits
LP_OUT = ("BF16", "GELU_BF16", "QGELU_BF16")
# u: unit roundoff; tiny: absolute rounding of a subnormal result; sigma: the standard deviation int_amp aims the integer results at
LP = {"bf16": dict(dtype=torch.bfloat16, u=2.0 ** -8, tiny=0.0, sigma=1000.0),
      "fp16": dict(dtype=torch.float16, u=2.0 ** -11, tiny=2.0 ** -25, sigma=3000.0)}
PRECISIONS = tuple(LP)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---- the case table --------------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Case:
    kernel: str
    m: int
    n: int
    k: int
    switches: tuple = ()      # (("GEMM_CFG", "C"), ...): names as tests/gemm_plan_cases.switches takes them, the library's carry VSC_ in front
    note: str = ""            # a (kernel, K-tile count) pair no test ran before: where the kernel handles the count

    @property
    def forced(self):
        return bool(self.switches)

    @property
    def id(self):
        sw = "".join(f"-{name[5:]}={value}" for name, value in self.switches)
        return f"{self.kernel}-{self.m}x{self.n}x{self.k}{sw}"

    def kernel_for(self, epilogue):
        """the persistent kernel has no PATCH write-out: the plan sends PATCH to V2_C (K <= 512, N > 128) or V3 instead, also where
        VSC_GEMM_V4=0 stands in for it"""
        v4_row = self.kernel == "V4" or dict(self.switches).get("GEMM_V4") == "0"
        if epilogue == "PATCH_F32" and v4_row:
            return "V2_C" if self.k <= 512 else "V3"
        return self.kernel


def _sweep(kernel, m, n, ks, switches, notes):
    return [Case(kernel, m, n, k, switches, notes.get(k, "")) for k in ks]


# K-tile counts that ran for the first time with this table, and where the code handles them (read before the first launch):
_V2 = ("gemm_bf16_v2_kernel: the prologue stages min(nk, STAGES - 1) tiles and waits with wait_tiles(issued - 1); the loop's "
       "`allowed = clamp(nk - 2 - kt, 0, STAGES - 2)` counts the tiles behind kt + 1 for every nk >= 1")
_V2A = {k: f"V2_A nk = {k // 32}: " + _V2 for k in (64, 128, 192, 256)}
_V2CD = {64: "nk = 2 = STAGES - 1: " + _V2}
_V3 = {64: "V3 nk = 1: ml64::prologue stages units 0..3 only and waits vmcnt(4); tiles() skips the steady loop and runs ktile<0, false>(rem = 1), "
           "whose waits drain 2 / 0 / 0 / 0 and which stages and pre-reads nothing",
       192: "V3 nk = 3: tiles() goes straight to the draining loop: rem = 3 (stages like a steady tile), rem = 2 (TAIL1 8 / 8 / 6 / 4), then rem = 1 "
            "on slot parity 0",
       320: "V3 nk = 5: one steady pair (t + 4 <= total), then the rem = 3, 2, 1 tail as at nk = 3"}
_SMALL = (1281, 264)          # 11 x 3 tiles of 128 x 128, 6 x 2 of 256 x 256: several blocks, ragged in M (1 row) and in N (8 columns)

CASES = [
    # V1, 128 x 128: default wherever fewer than 65 (K <= 512) / 129 tiles of 256 x 256 exist
    Case("V1", 1, 4, 64), Case("V1", 129, 132, 128), Case("V1", 257, 260, 192), Case("V1", 1281, 264, 64),
    Case("V1", 16641, 1024, 128, (("GEMM_V1", "1"),)),
    # V2_B, 256 x 128 on 8 waves: N <= 128
    Case("V2_B", 16385, 128, 64), Case("V2_B", 16385, 120, 192),
    *_sweep("V2_B", 1281, 120, (64, 128, 192, 256), (("GEMM_CFG", "B"),), {}),
    # V2_C, 128 x 256 on 4 waves, 3 stages: K <= 512
    Case("V2_C", 8449, 512, 64, note=_V2CD[64]), Case("V2_C", 8449, 264, 192), Case("V2_C", 8449, 520, 128),
    *_sweep("V2_C", *_SMALL, (64, 128, 192, 256), (("GEMM_CFG", "C"),), _V2CD),
    # V2_D, 256 x 128 on 4 waves, 3 stages: K <= 512 and N % 256 == 128
    Case("V2_D", 8449, 384, 64, note=_V2CD[64]), Case("V2_D", 8449, 384, 256),
    *_sweep("V2_D", *_SMALL, (64, 128, 192, 256), (("GEMM_CFG", "D"),), _V2CD),
    # V2_A, 256 x 256 on 8 waves, 4 stages: no default route leads here any more (v3 took its shapes)
    *_sweep("V2_A", *_SMALL, (64, 128, 192, 256), (("GEMM_CFG", "A"), ("GEMM_V3", "0")), _V2A),
    # V3, 256 x 256 on the mainloop64 K loop, one tile per workgroup: 9, 10 and 50 K-tiles by default, 1..5 under VSC_GEMM_CFG=A
    Case("V3", 8449, 1024, 576), Case("V3", 8449, 1000, 640), Case("V3", 8449, 1032, 576), Case("V3", 16641, 1024, 3200),
    *_sweep("V3", *_SMALL, (64, 128, 192, 256, 320), (("GEMM_CFG", "A"),), _V3),
    Case("V3", 16641, 1024, 128, (("GEMM_V4", "0"),)),
    # V4, V3 as a persistent kernel: more tiles than CUs, K % 128 == 0, K <= 3072; whole and ragged N tiles (1000: 232, 1032: 8 columns)
    Case("V4", 16641, 1024, 128), Case("V4", 16641, 1024, 256), Case("V4", 16641, 1024, 384), Case("V4", 16641, 1000, 640),
    Case("V4", 16897, 1032, 640), Case("V4", 16641, 1024, 3072),
]
DEFAULT_CASES = [c for c in CASES if not c.forced]
FORCED_CASES = [c for c in CASES if c.forced]
KERNELS = ("V1", "V2_A", "V2_B", "V2_C", "V2_D", "V3", "V4")
# the switches under which V4's bits must equal its default run's
V4_VARIANTS = ((("GEMM_GROUP_N", "1"),), (("GEMM_GROUP_N", "2"),), (("GEMM_V4_GRID", "128"),))


def case(kernel, m, n, k, forced=None):
    found = [c for c in CASES if (c.kernel, c.m, c.n, c.k) == (kernel, m, n, k) and (forced is None or c.forced == forced)]
    assert len(found) == 1, (kernel, m, n, k, forced, found)
    return found[0]


# one default-route and one forced-route shape per kernel: every exact epilogue (the other rows: BF16 and RESADD_F32)
ALL_EPILOGUE_CASES = [case("V1", 257, 260, 192), case("V1", 16641, 1024, 128, True), case("V2_B", 16385, 120, 192), case("V2_B", 1281, 120, 128),
                      case("V2_C", 8449, 520, 128), case("V2_C", 1281, 264, 64), case("V2_D", 8449, 384, 256), case("V2_D", 1281, 264, 192),
                      case("V2_A", 1281, 264, 256), case("V3", 8449, 1032, 576), case("V3", 1281, 264, 320), case("V4", 16897, 1032, 640)]
# check C, one row per kernel
ISOLATION_CASES = [case("V1", 257, 260, 192), case("V2_A", 1281, 264, 128), case("V2_B", 16385, 120, 192), case("V2_C", 8449, 264, 192),
                   case("V2_D", 8449, 384, 64), case("V3", 8449, 1000, 640), case("V4", 16897, 1032, 640)]
# GELU / QGELU across the plans: one operand set through V1 (no switch: fewer than 65 tiles), then under each row's switches
CROSS_PLAN = [[Case("V1", 1281, 264, 64), case("V2_A", 1281, 264, 64), case("V2_C", 1281, 264, 64, True), case("V2_D", 1281, 264, 64),
               case("V3", 1281, 264, 64)],
              [Case("V1", 1281, 120, 64), case("V2_B", 1281, 120, 64)]]     # VSC_GEMM_CFG=B needs N <= 128


def exact_epilogues(c):
    return EXACT_EPILOGUES if c in ALL_EPILOGUE_CASES else ("BF16", "RESADD_F32")


def patch_tokens(m):
    """tokens of a PATCH launch: tokens - 1 = the largest divisor of m up to 300 (1281 = 21 x 61, 8449 = 119 x 71, 16385 = 113 x 145, ...)"""
    return max(d for d in range(1, min(m, 300) + 1) if m % d == 0) + 1


# ---- operands --------------------------------------------------------------------------------------------------------------------------

def int_amp(precision, k):
    """the smallest amplitude whose results (variance K (amp (amp + 1) / 3)^2 for uniform integers) have the standard deviation
    LP[precision]['sigma']: 19 (bf16) / 34 (fp16) at K = 64, 7 / 13 at K = 3200"""
    amp = 1
    while math.sqrt(k) * amp * (amp + 1) / 3.0 < LP[precision]["sigma"]:
        amp += 1
    assert k * amp * amp < 2 ** 24, (precision, k, amp)
    return amp


class Operands:
    """a [m, k], w [n, k] of the operand type; bias [n], res [m, n], pos [tokens, n] fp32"""

    def __init__(self, c, precision, a, w, bias, res, pos, dev):
        self.case, self.precision, self.dev = c, precision, dev
        self.m, self.n, self.k, self.tokens = c.m, c.n, c.k, pos.shape[0]
        self.a, self.w, self.bias, self.res, self.pos = (t.to(dev) for t in (a, w, bias, res, pos))
        self._cache = {}

    def acc64(self):
        if "acc" not in self._cache:
            self._cache["acc"] = self.a.double() @ self.w.double().t()
        return self._cache["acc"]

    def mag64(self):
        if "mag" not in self._cache:
            self._cache["mag"] = self.a.double().abs() @ self.w.double().abs().t()
        return self._cache["mag"]

    def with_rows(self, which, rows, value):
        """a copy whose rows `rows` of a (which = "a") or w hold `value`"""
        o = Operands.__new__(Operands)
        o.__dict__.update(self.__dict__)
        o._cache = {}
        t = getattr(self, which).clone()
        t[list(rows)] = value
        setattr(o, which, t)
        return o

    def patch(self, t, fill=0.0):
        """[m, n] by patch row -> [frames * tokens, n] by token row, the CLS rows (token 0) holding `fill`"""
        frames = self.m // (self.tokens - 1)
        out = torch.full((frames, self.tokens, self.n), fill, dtype=t.dtype, device=t.device)
        out[:, 1:] = t.reshape(frames, self.tokens - 1, self.n)
        return out.reshape(frames * self.tokens, self.n)

    def pos_rows(self, dtype):
        frames = self.m // (self.tokens - 1)
        return self.pos[1:].to(dtype).repeat(frames, 1)


def _seed(c, salt):
    return (c.m * 1000003 + c.n * 10007 + c.k * 101 + salt) % (2 ** 31)


def int_operands(c, precision, dev="cpu"):
    g = torch.Generator().manual_seed(_seed(c, 1))
    amp, dtype = int_amp(precision, c.k), LP[precision]["dtype"]
    tokens = patch_tokens(c.m)
    a = torch.randint(-amp, amp + 1, (c.m, c.k), generator=g, dtype=torch.int8).to(dtype)
    w = torch.randint(-amp, amp + 1, (c.n, c.k), generator=g, dtype=torch.int8).to(dtype)
    bias = torch.randint(-9, 10, (c.n,), generator=g, dtype=torch.int8).float() * 0.5
    res = torch.randint(-64, 65, (c.m, c.n), generator=g, dtype=torch.int8).float()
    pos = torch.randint(-64, 65, (tokens, c.n), generator=g, dtype=torch.int8).float()
    return Operands(c, precision, a, w, bias, res, pos, dev)


def real_operands(c, precision, dev="cpu"):
    g = torch.Generator().manual_seed(_seed(c, 2))
    dtype, tokens = LP[precision]["dtype"], patch_tokens(c.m)
    a = torch.randn(c.m, c.k, generator=g).to(dtype)
    w = (torch.randn(c.n, c.k, generator=g) * c.k ** -0.5).to(dtype)
    bias = torch.randn(c.n, generator=g) * 0.5
    res = torch.randn(c.m, c.n, generator=g)
    pos = torch.randn(tokens, c.n, generator=g)
    return Operands(c, precision, a, w, bias, res, pos, dev)


# ---- references ------------------------------------------------------------------------------------------------------------------------

def reference64(o, epilogue):
    """float64 statement of the operation on the operands as given -> (y, z): the output and the pre-activation a + bias"""
    z = o.acc64() + o.bias.double()
    if epilogue == "GELU_BF16":
        return z * 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))), z
    if epilogue == "QGELU_BF16":
        return z * torch.sigmoid(1.702 * z), z
    if epilogue == "RESADD_F32":
        return z + o.res.double(), z
    if epilogue == "PATCH_F32":
        return o.patch(z + o.pos_rows(torch.float64)), z
    return z, z


def exact_reference(o, epilogue):
    """check A: the float64 result, rounded once to the output type (float64 -> fp32 is exact here: integers and halves below 2^23)"""
    assert epilogue in EXACT_EPILOGUES
    y, _ = reference64(o, epilogue)
    assert float(y.abs().max()) < 2 ** 23
    y32 = y.float()
    assert torch.equal(y32.double(), y)
    return y32.to(LP[o.precision]["dtype"]) if epilogue in LP_OUT else y32


def exact_conditions(o):
    """(largest |y|, share of y that the operand type cannot hold) of the BF16 epilogue's float64 result"""
    y, _ = reference64(o, "BF16")
    held = y.float().to(LP[o.precision]["dtype"]).double() == y
    return float(y.abs().max()), 1.0 - float(held.double().mean())


def epilogue_error(o, epilogue, y, z, accterm):
    """e_epi of check B (the module docstring derives each term)"""
    lp = LP[o.precision]
    adds = 2.0 ** -23 * (o.acc64().abs() + o.bias.double().abs())                  # fl(acc + bias)
    if epilogue == "RESADD_F32":
        return adds + 2.0 ** -23 * (z.abs() + o.res.double().abs())
    if epilogue == "PATCH_F32":
        return o.patch(adds + 2.0 ** -23 * (z.abs() + o.pos_rows(torch.float64).abs()))
    if epilogue == "F32":
        return adds
    if epilogue == "GELU_BF16":
        e = 1.13 * (accterm + adds) + 4.3e-5 + 3.5e-6 * z.abs()
    elif epilogue == "QGELU_BF16":
        e = 1.1 * (accterm + adds) + 2.0 ** -21 * y.abs() + 2.0 ** -24
    else:
        e = adds
    return e + lp["u"] * (accterm + e) + lp["tiny"]                                # the store rounds the erroneous value


# ---- the checks ------------------------------------------------------------------------------------------------------------------------
# run(operands, epilogue) -> the output tensor ([m, n], PATCH: [frames * tokens, n]) on any device

def _first(bad):
    i = int(torch.nonzero(bad.reshape(-1))[0])
    return divmod(i, bad.shape[-1])


def check_exact(run, o, epilogues):
    for e in epilogues:
        want = exact_reference(o, e)
        got = run(o, e).to(want.device)
        assert got.dtype == want.dtype and got.shape == want.shape, f"exact: {o.case.id} {e}: {got.dtype} {tuple(got.shape)}"
        bad = bits(got) != bits(want)
        if bool(bad.any()):
            r, c = _first(bad)
            raise AssertionError(f"exact: {o.case.id} {e} {o.precision}: {int(bad.sum())} of {bad.numel()} elements differ from the float64 result "
                                 f"rounded once, first at ({r}, {c}): got {float(got[r, c])}, want {float(want[r, c])}")


def check_same_bits(outs, what):
    """outs: [(name, tensor)]; every tensor has the bits of the first"""
    name0, t0 = outs[0]
    for name, t in outs[1:]:
        bad = bits(t) != bits(t0)
        if bool(bad.any()):
            r, c = _first(bad)
            raise AssertionError(f"same_bits: {what}: {name} differs from {name0} in {int(bad.sum())} of {bad.numel()} elements, first at ({r}, {c}): "
                                 f"{float(t[r, c])} vs {float(t0[r, c])}")


def check_bound(run, o, epilogues, report=None):
    """-> worst |d| / bound over the epilogues; report gets (case id, precision, epilogue, ratio) before anything is asserted"""
    lp, worst, failed = LP[o.precision], 0.0, []
    accterm = 2.0 * o.k * 2.0 ** -24 * o.mag64()
    for e in epilogues:
        y, z = reference64(o, e)
        u = lp["u"] if e in LP_OUT else 0.0
        acc_e = o.patch(accterm) if e == "PATCH_F32" else accterm
        bound = u * y.abs() + acc_e + epilogue_error(o, e, y, z, accterm)
        got = run(o, e).to(y.device)
        assert got.shape == y.shape and got.dtype == (lp["dtype"] if e in LP_OUT else torch.float32), f"bound: {o.case.id} {e}: {got.dtype} {tuple(got.shape)}"
        d = (got.double() - y).abs()
        d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
        ratio = torch.where(bound > 0, d / bound.clamp(min=1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
        r = float(ratio.max())
        worst = max(worst, r)
        if report is not None:
            report.append((o.case.id, o.precision, e, round(r, 4)))
        if r > 1.0:
            failed.append(f"{e}: {r:.3f} x the bound, {float((ratio > 1).double().mean()) * 100:.2f} % of elements above it")
    assert not failed, f"bound: {o.case.id} {o.precision}: " + "; ".join(failed)
    return worst


def boundary_and_ragged(count, tile=256):
    """the last row of the last whole 256 (else 128) tile and the last row (the ragged tile's): a tile boundary lies between them when
    count is one past whole tiles"""
    last = count - 1
    for t in (tile, 128):
        if last >= t:
            return sorted({(last // t) * t - 1, last})
    return [last]


def poison_values(precision):
    return (float(torch.finfo(LP[precision]["dtype"]).max), float("inf"), float("nan"))


def check_isolation(run, o, epilogues=("BF16", "RESADD_F32")):
    rows, cols = boundary_and_ragged(o.m), boundary_and_ragged(o.n)
    for e in epilogues:
        clean = run(o, e).cpu()
        assert bool(torch.isfinite(clean.float()).all())
        for value in poison_values(o.precision):
            for which, idx in (("a", rows), ("w", cols)):
                got = run(o.with_rows(which, idx, value), e).cpu()
                differs = bits(got) != bits(clean)
                hit = torch.zeros_like(differs)
                if which == "a":
                    hit[idx] = True
                else:
                    hit[:, idx] = True
                leaked = differs & ~hit
                if bool(leaked.any()):
                    r, c = _first(leaked)
                    raise AssertionError(f"isolation: {o.case.id} {e} {o.precision}: {which} rows {idx} = {value} changed {int(leaked.sum())} elements "
                                         f"outside them, first at ({r}, {c})")
                # ... and the poison reached the kernel: each of those rows (columns) changed somewhere
                reached = differs.any(dim=1)[idx] if which == "a" else differs.any(dim=0)[idx]
                assert bool(reached.all()), f"isolation: {o.case.id} {e}: {which} rows {idx} = {value} left an output row unchanged"


# ---- the torch emulation of the kernels' rounding points, and its defects ----------------------------------------------------------------

MUTATIONS = ("truncating_store", "round_half_away", "drop_last_k_tile", "drop_one_k_element", "bias_shifted_four_columns",
             "swap_two_column_groups_in_last_n_tile", "last_m_tile_row_from_previous_tile", "nan_row_leaks_to_neighbour")


def _gelu_coefficients():
    src = open(os.path.join(ROOT, "vsc22-submission_amd", "csrc", "gelu_poly.h")).read()
    assert "GELU_DEG = 8;" in src and "GELU_U = 4.5f" in src
    body = re.search(r"constexpr float GELU_C\[GELU_DEG \+ 1\] = \{([^}]*)\}", src).group(1)
    return [float(v.strip().rstrip("f")) for v in body.split(",")]


def gelu_poly_f32(x):
    """csrc/gelu_poly.h::gelu2 in fp32 (multiply-adds unfused)"""
    c = _gelu_coefficients()
    t = x.clamp(-4.5, 4.5)
    z = t * t * torch.tensor(2.0 / (4.5 * 4.5), dtype=torch.float32) - 1.0
    q = torch.full_like(x, c[8])
    for i in range(7, -1, -1):
        q = q * z + c[i]
    return x * (t * q + 0.5)


def quick_gelu_f32(x):
    return x * (1.0 / (1.0 + torch.exp2(x * torch.tensor(-2.45546696, dtype=torch.float32))))


def _toward_zero(v, dtype):
    """fp32 -> dtype, truncated: the nearest-even result stepped back by one where it lies beyond v"""
    h = v.to(dtype)
    beyond = h.double().abs() > v.double().abs()
    return torch.where(beyond, (bits(h) - 1).view(dtype), h)


def _store(v, dtype, mutation):
    if mutation == "truncating_store":
        return _toward_zero(v, dtype)
    h = v.to(dtype)
    if mutation == "round_half_away":
        lo = _toward_zero(v, dtype)
        hi = (bits(lo) + 1).view(dtype)
        tie = (v.double() - lo.double()).abs() == (hi.double() - v.double()).abs()
        return torch.where(tie, hi, h)
    return h


def smallest_nonzero_k(o):
    """drop_one_k_element drops a[m - 1, k*] for the k* where that row's |a| is smallest but not zero: a kernel that loses an element
    does not pick a large one.  On integer operands that is still a whole product (|a| >= 1) in every column with w[., k*] != 0."""
    row = o.a[o.m - 1].double().abs()
    return int(torch.where(row > 0, row, torch.full_like(row, float("inf"))).argmin())


def emulate(o, epilogue, mutation=None):
    assert mutation is None or mutation in MUTATIONS, mutation
    key = ("emulated acc", mutation if mutation in ("drop_one_k_element", "drop_last_k_tile") else None)
    if key not in o._cache:      # (shared by the epilogues of one operand set)
        a, w = o.a.float(), o.w.float()
        if mutation == "drop_one_k_element":
            a[o.m - 1, smallest_nonzero_k(o)] = 0.0
        chunks = o.k // 64 - (1 if mutation == "drop_last_k_tile" else 0)
        acc = torch.zeros((o.m, o.n), dtype=torch.float32, device=a.device)
        for i in range(chunks):
            acc += a[:, i * 64:(i + 1) * 64] @ w[:, i * 64:(i + 1) * 64].t()
        o._cache[key] = acc
    acc = o._cache[key]
    bias = o.bias
    if mutation == "bias_shifted_four_columns":      # the last four columns take the bias of the four before them (n = 4: none)
        bias = bias.clone()
        bias[o.n - 4:] = o.bias[o.n - 8:o.n - 4] if o.n >= 8 else 0.0
    v = acc + bias
    if epilogue == "GELU_BF16":
        v = gelu_poly_f32(v)
    elif epilogue == "QGELU_BF16":
        v = quick_gelu_f32(v)
    elif epilogue == "RESADD_F32":
        v = v + o.res
    elif epilogue == "PATCH_F32":
        v = v + o.pos_rows(torch.float32)
    if mutation == "swap_two_column_groups_in_last_n_tile":      # two 4-column groups (n = 4: two 2-column halves)
        g = 4 if o.n >= 8 else 2
        v = torch.cat([v[:, :o.n - 2 * g], v[:, o.n - g:], v[:, o.n - 2 * g:o.n - g]], dim=1)
    if mutation == "last_m_tile_row_from_previous_tile":
        v = v.clone()
        v[o.m - 1] = v[o.m - 2] if o.m >= 2 else 0.0
    if mutation == "nan_row_leaks_to_neighbour":
        v = v.clone()
        bad = ~torch.isfinite(o.a.float()).all(dim=1)
        before = torch.roll(bad, -1)      # the row in front of a row that is not finite
        before[-1] = False
        v[before & ~bad] = float("nan")
    if epilogue in LP_OUT:
        v = _store(v, LP[o.precision]["dtype"], mutation)
    return o.patch(v) if epilogue == "PATCH_F32" else v


def emulation(mutation=None):
    return lambda o, epilogue: emulate(o, epilogue, mutation)


# ---- vsc_gemm_ln_bf16: x0 + LayerNorm(a w^T + bias), K edges of the row-owning tiles ------------------------------------------------------
# one row past a row block (512 x 128, 256 x 256, 128 x 512); K / 32 = 1..5 straddles the 4-stage ring (prologue min(nk, 3) tiles)
LN_CASES = [(m, n, k) for n, m in ((128, 513), (256, 257), (512, 129)) for k in (32, 64, 96, 128, 160)]
LN_PERSISTENT = (34816, 512, 128)      # VSC_GEMM_LN_V4=1: 136 x 2 = 272 tiles of 256 x 256 on 256 CUs, tiles_m % 8 == 0 (the pair exchange)


def ln_operands(m, n, k, precision, dev="cpu"):
    g = torch.Generator().manual_seed(m * 31 + n * 7 + k)
    dtype = LP[precision]["dtype"]
    t = dict(a=torch.randn(m, k, generator=g).to(dtype), w=(torch.randn(n, k, generator=g) * k ** -0.5).to(dtype), bias=torch.randn(n, generator=g) * 0.2,
             x0=torch.randn(m, n, generator=g), gamma=0.3 + torch.randn(n, generator=g) * 0.05, beta=torch.randn(n, generator=g) * 0.05)
    return {name: v.to(dev) for name, v in t.items()}


def ln_reference64(t, eps=1e-5):
    z = t["a"].double() @ t["w"].double().t() + t["bias"].double()
    mean, var = z.mean(dim=1, keepdim=True), z.var(dim=1, unbiased=False, keepdim=True)
    return t["x0"].double() + (z - mean) / torch.sqrt(var + eps) * t["gamma"].double() + t["beta"].double()
