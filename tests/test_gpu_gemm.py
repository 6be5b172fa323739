"""The GEMM kernels of csrc/gemm_bf16.hip on a real MI355X, plan by plan, in both operand builds: V1, the four configurations of the
256-row v2 kernel, V3 and the persistent V4, and the row-owning gemm_ln tiles.

The cases, the float64 references, the bounds and the checks are tests/gemm_cases.py; tests/test_gemm_cases_cpu.py shows without a GPU
that every row is on the kernel it names, that a torch emulation of the kernels' rounding points passes every check, and that an
emulation with a truncating or tie-away store, a lost K-tile or k-element, a shifted bias, swapped column groups, a row taken from
the tile before or a NaN row that leaks does not.  Every launch here first asks the library for its plan (ops.gemm_plan) under the
row's switches, so a routing rule that moves cannot leave a case on another kernel unnoticed.  The forced routes use the library's
diagnostic switches: they are the only way to V2_A (never a default) and to V3 with 1..5 K-tiles."""
import contextlib

import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu

PRECISIONS = gc.PRECISIONS


def _ids(cases):
    return [pytest.param(c, id=c.id) for c in cases]


@pytest.fixture(scope="module")
def dev():
    from vsc_hip import _lib
    for precision in PRECISIONS:
        _lib.require_device(precision)
    return torch.device("cuda:0")


@contextlib.contextmanager
def _under(precision, switches):
    """the operand build and the row's switches, nested: a failure inside cannot leave a switch set"""
    from vsc_hip import _lib, ops
    with contextlib.ExitStack() as stack:
        stack.enter_context(ops.operands(precision))
        for name, value in switches:
            stack.enter_context(_lib.option("VSC_" + name, value))
        yield


def _launch(o, e):
    from vsc_hip import ops
    aux = o.res if e == "RESADD_F32" else o.pos if e == "PATCH_F32" else None
    out = ops.gemm_bf16(o.a, o.w, o.bias, epilogue=gc.EPI[e], aux=aux, tokens=o.tokens if e == "PATCH_F32" else 0)
    torch.cuda.synchronize()
    return out


def _runner(c, switches=None, kernel=None):
    """run(operands, epilogue) on the kernel the row names: the plan is asserted under the switches before every launch"""
    from vsc_hip import ops
    switches = c.switches if switches is None else switches

    def run(o, e):
        with _under(o.precision, switches):
            plan = ops.gemm_plan(o.m, o.n, o.k, gc.EPI[e])
            assert plan["kernel"] == (kernel or c.kernel_for(e)), (c.id, e, switches, plan)
            return _launch(o, e)
    return run


# ------------------------------------------------------------------------------------------------------------ (A) integer-exact

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("c", _ids(gc.CASES))
def test_gemm_is_exact_on_integer_operands(dev, precision, c):
    """bit for bit the float64 result (fp32 write-outs), that result rounded once to nearest even (16-bit write-out): every product and
    partial sum of these operands is exact in fp32.  BF16 and RESADD_F32 on every row, PATCH_F32 and F32 as well on one default and
    one forced row per kernel -- and there GELU_BF16 and QGELU_BF16 with the bits of the 128 x 128 kernel (VSC_GEMM_V1=1), which
    test_gemm_within_float64_bound holds to float64."""
    o = gc.int_operands(c, precision, dev)
    gc.check_exact(_runner(c), o, gc.exact_epilogues(c))
    if c in gc.ALL_EPILOGUE_CASES and c.kernel != "V1":
        for e in ("GELU_BF16", "QGELU_BF16"):
            gc.check_same_bits([("V1", _runner(c, (("GEMM_V1", "1"),), "V1")(o, e)), (c.id, _runner(c)(o, e))], f"{e} {precision}")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("group", [pytest.param(g, id=f"{g[0].m}x{g[0].n}x{g[0].k}") for g in gc.CROSS_PLAN])
def test_activations_have_the_bits_of_v1_on_every_plan(dev, precision, group):
    """GELU / QGELU of one integer operand set through V1, then through every 256-row plan under its switches: the fp32 pre-activation is
    the same number and all plans share csrc/gelu_poly.h and quick_gelu()"""
    o = gc.int_operands(group[0], precision, dev)
    for e in ("GELU_BF16", "QGELU_BF16"):
        gc.check_same_bits([(c.id, _runner(c)(o, e)) for c in group], f"{e} {precision}")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("c", _ids([c for c in gc.CASES if c.kernel == "V4"]))
def test_persistent_kernel_activations_have_the_bits_of_v1(dev, precision, c):
    o = gc.int_operands(c, precision, dev)
    for e in ("GELU_BF16", "QGELU_BF16"):
        gc.check_same_bits([("V1", _runner(c, (("GEMM_V1", "1"),), "V1")(o, e)), (c.id, _runner(c)(o, e))], f"{e} {precision}")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("c", _ids([c for c in gc.CASES if c.kernel == "V4"]))
def test_persistent_kernel_regrouped_and_on_half_the_grid_equals_itself(dev, precision, c):
    """VSC_GEMM_GROUP_N = 1, 2 and VSC_GEMM_V4_GRID = 128 change the tile order and the tiles per workgroup, never a bit; each is
    launched twice, so the second launch finds the first one's ring in LDS"""
    o = gc.real_operands(c, precision, dev)
    for e in ("BF16", "GELU_BF16", "RESADD_F32"):
        outs = [("default", _runner(c)(o, e))]
        for switches in gc.V4_VARIANTS:
            for launch in (1, 2):
                outs.append((f"{switches[0][0]}={switches[0][1]} launch {launch}", _runner(c, switches)(o, e)))
        gc.check_same_bits(outs, f"{c.id} {e} {precision}")


# ------------------------------------------------------------------------------------------------------------ (B) float64 bound

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("c", _ids(gc.DEFAULT_CASES))
def test_gemm_within_float64_bound(dev, precision, c):
    """|got - y64| <= u |y64| + 2 K 2^-24 (|A| |W|^T) + e_epi element-wise over the whole output, every epilogue the kernel serves
    (gemm_cases.check_bound derives e_epi).  The emulation reaches 0.99 (bf16) / 0.97 (fp16) of the bound on the 16-bit outputs and
    0.05 on the fp32 ones; the kernel's own figures are printed with every case (profiles/gemm_parity_ratios.txt)."""
    epilogues = [e for e in gc.EPILOGUES if c.kernel_for(e) == c.kernel]
    report = []
    try:
        gc.check_bound(_runner(c), gc.real_operands(c, precision, dev), epilogues, report=report)
    finally:
        for cid, prec, e, ratio in report:
            print(f"gemm parity {prec} {c.kernel} {cid} {e}: worst |d| / bound {ratio:.4f}")


# ------------------------------------------------------------------------------------------------------------ (C) isolation

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("c", _ids(gc.ISOLATION_CASES))
def test_gemm_rows_and_columns_are_isolated(dev, precision, c):
    """a row of A at a tile boundary and the row of the ragged last tile (then two such rows of W) filled with the largest finite
    value, +inf, NaN: exactly those output rows (columns) change"""
    gc.check_isolation(_runner(c), gc.real_operands(c, precision, dev))


# ------------------------------------------------------------------------------------------------------------ gemm_ln, K edges

def _gemm_ln(t):
    from vsc_hip import ops
    x, xb = ops.gemm_ln_bf16(t["a"], t["w"], t["bias"], t["gamma"], t["beta"], 1e-5, x_in=t["x0"])
    torch.cuda.synchronize()
    return x, xb


def _check_gemm_ln(dev, precision, m, n, k, rows):
    """x0 + LayerNorm(a w^T + bias) against float64 at the tolerance of test_gemm_ln_matches_torch; the shadow is the rounded output; rows
    of A that are not finite stay their own (the row statistics travel through LDS partials and, on the persistent kernel at N = 512,
    through the pair exchange in L2)"""
    t = gc.ln_operands(m, n, k, precision, dev)
    x, xb = _gemm_ln(t)
    torch.testing.assert_close(x.double(), gc.ln_reference64(t), rtol=1e-4, atol=1e-4)
    assert xb.dtype == gc.LP[precision]["dtype"] and torch.equal(gc.bits(xb), gc.bits(x.to(xb.dtype)))
    others = torch.ones(m, dtype=torch.bool, device=dev)
    others[rows] = False
    for value in gc.poison_values(precision):
        a = t["a"].clone()
        a[rows] = value
        x2, xb2 = _gemm_ln(dict(t, a=a))
        assert torch.equal(gc.bits(x2[others]), gc.bits(x[others])) and torch.equal(gc.bits(xb2[others]), gc.bits(xb[others])), \
            f"gemm_ln {(m, n, k)} {precision}: rows {rows} = {value} changed other rows"
        assert bool((gc.bits(x2[rows]) != gc.bits(x[rows])).any(dim=1).all())


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("m,n,k", gc.LN_CASES)
def test_gemm_ln_k_edges(dev, precision, m, n, k):
    """K / 32 = 1..5 against the 4-stage ring of the row-owning tiles (prologue min(nk, 3) tiles), one row past a row block"""
    from vsc_hip import ops
    with ops.operands(precision):
        _check_gemm_ln(dev, precision, m, n, k, gc.boundary_and_ragged(m, tile=m - 1))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_gemm_ln_persistent_kernel_at_two_k_tiles(dev, precision):
    """VSC_GEMM_LN_V4=1 at K = 128: the persistent kernel's LN_RES write-out with two K-tiles per output tile, 272 tiles in pairs"""
    m, n, k = gc.LN_PERSISTENT
    with _under(precision, (("GEMM_LN_V4", "1"),)):
        _check_gemm_ln(dev, precision, m, n, k, gc.boundary_and_ragged(m))
