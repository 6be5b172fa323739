"""tests/gemm_cases.py held to itself, without a GPU: every row of the table is on the kernel it names (csrc/gemm_plan.h compiled for the
host, at 256 CUs), the integer operands meet the conditions check A rests on, the torch emulation of the kernels' rounding points
passes every check tests/test_gpu_gemm.py runs on the kernels (so the bounds can be met by the arithmetic alone), and an emulation
with one defect fails the check that is there for that defect."""
import ctypes
import os
import subprocess

import pytest

import gemm_cases as gc
import gemm_plan_cases as P
import hip_emu_build

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gemm_cases") / "libgemm_plan_shim.so")
    subprocess.check_call([hip_emu_build.compiler(), "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Werror", "-I", hip_emu_build.CSRC,
                           "-o", out, os.path.join(HERE, "gemm_plan_shim.cpp")])
    return ctypes.CDLL(out)


def _kernel(shim, m, n, k, epilogue, switches=(), cus=256):
    sw, out = (ctypes.c_int * 12)(*P.switches(**dict(switches))), (ctypes.c_longlong * 11)()
    shim.plan_gemm(ctypes.c_longlong(m), n, k, gc.EPI[epilogue], 0, 0, cus, sw, out)
    return P.KERNELS[out[0]]


def test_every_row_is_on_the_kernel_it_names(shim):
    for c in gc.CASES:
        for e in gc.EPILOGUES:
            assert _kernel(shim, c.m, c.n, c.k, e, c.switches) == c.kernel_for(e), (c.id, e)
        assert c.m % 128 == 1 and c.k % 64 == 0 and c.m % (gc.patch_tokens(c.m) - 1) == 0
    # the forced rows are forced: without their switches these shapes run the 128 x 128 kernel (the V4=0 / V1=1 row: V4)
    for c in gc.FORCED_CASES:
        assert _kernel(shim, c.m, c.n, c.k, "BF16") == ("V4" if c.m == 16641 else "V1"), c.id
    # the persistent kernel's variants stay on it, and PATCH never reaches it
    for c in gc.CASES:
        if c.kernel == "V4":
            for sw in gc.V4_VARIANTS:
                assert _kernel(shim, c.m, c.n, c.k, "RESADD_F32", sw) == "V4", (c.id, sw)
            assert c.kernel_for("PATCH_F32") in ("V2_C", "V3")
            assert _kernel(shim, c.m, c.n, c.k, "BF16", (("GEMM_V1", "1"),)) == "V1"
    # the cross-plan sets: one shape each, V1 first
    for group in gc.CROSS_PLAN:
        assert group[0].kernel == "V1" and not group[0].forced and len({(c.m, c.n, c.k) for c in group}) == 1
        for c in group:
            for e in ("GELU_BF16", "QGELU_BF16"):
                assert _kernel(shim, c.m, c.n, c.k, e, c.switches) == c.kernel
    assert {c.kernel for c in gc.CASES} == set(gc.KERNELS) == {c.kernel for c in gc.ISOLATION_CASES} == {c.kernel for c in gc.ALL_EPILOGUE_CASES}
    assert len({c.id for c in gc.CASES}) == len(gc.CASES)


def _ln_kernel(shim, m, n, k, **options):
    sw, out = (ctypes.c_int * 12)(*P.switches(**options)), (ctypes.c_longlong * 11)()
    shim.plan_gemm_ln(ctypes.c_longlong(m), n, k, 0, 256, 1, sw, out)
    return P.KERNELS[out[0]]


def test_the_table_holds_the_k_tile_counts_it_is_there_for(shim):
    nk = lambda kernel, per: {c.k // per for c in gc.CASES if c.kernel == kernel}
    assert {1, 2, 3, 4, 5, 9, 10, 50} <= nk("V3", 64)
    assert nk("V2_A", 32) == {2, 4, 6, 8} and {2, 4, 6, 8} <= nk("V2_C", 32) & nk("V2_D", 32) & nk("V2_B", 32)
    assert {2, 4, 6, 10, 48} <= nk("V4", 64)
    # every (kernel, K-tile count) pair that no test ran before says where the kernel handles it
    first = [c for c in gc.CASES if (c.kernel == "V2_A") or (c.kernel == "V3" and c.k in (64, 192, 320)) or (c.kernel in ("V2_C", "V2_D") and c.k == 64)]
    assert len(first) == 4 + 3 + 4 and all(c.note for c in first)
    # V4 with a ragged N tile, V3 / V4 with whole ones
    assert {c.n % 256 for c in gc.CASES if c.kernel == "V4"} == {0, 232, 8}
    # gemm_ln: K / 32 on both sides of the 4-stage ring, one row past a row block
    assert {k // 32 for _, _, k in gc.LN_CASES} == {1, 2, 3, 4, 5} and all(m % {128: 512, 256: 256, 512: 128}[n] == 1 for m, n, _ in gc.LN_CASES)
    m, n, k = gc.LN_PERSISTENT
    assert _ln_kernel(shim, m, n, k, GEMM_LN_V4="1") == "V4" and _ln_kernel(shim, m, n, k) == "LN_ROW_512"
    assert (m // 256) % 8 == 0 and (m // 256) * 2 == 272
    assert all(_ln_kernel(shim, m, n, k) == f"LN_ROW_{n}" for m, n, k in gc.LN_CASES)


@pytest.mark.parametrize("precision", gc.PRECISIONS)
def test_integer_operands_meet_the_conditions_of_check_a(precision):
    """on the reference alone: exact in fp32 (K amp^2 < 2^24, asserted by int_amp), below 65504, and at least 10 % of the results are not
    values of the operand type -- so a store that truncates or rounds ties away cannot pass"""
    seen = {}
    for c in gc.CASES:
        if (c.m, c.n, c.k) in seen:
            continue
        big, share = gc.exact_conditions(gc.int_operands(c, precision))
        seen[(c.m, c.n, c.k)] = (big, share)
        assert big < 65504 and share >= 0.10, (c.id, precision, big, share)
    print(f"{precision}: max |y| {max(v[0] for v in seen.values()):.0f}, not representable {min(v[1] for v in seen.values()) * 100:.0f} .. "
          f"{max(v[1] for v in seen.values()) * 100:.0f} % of the results")


@pytest.mark.parametrize("precision", gc.PRECISIONS)
def test_clean_emulation_passes_every_check(precision):
    run, report = gc.emulation(), []
    for c in gc.CASES:
        o = gc.int_operands(c, precision)
        gc.check_exact(run, o, gc.exact_epilogues(c))
        if not c.forced:
            gc.check_bound(run, gc.real_operands(c, precision), gc.EPILOGUES, report=report)
    for group in gc.CROSS_PLAN:
        o = gc.int_operands(group[0], precision)
        for e in ("GELU_BF16", "QGELU_BF16"):
            gc.check_same_bits([(c.id, run(o, e)) for c in group], e)
    for c in gc.ISOLATION_CASES:
        gc.check_isolation(run, gc.real_operands(c, precision))
    worst = {e: max(r[3] for r in report if r[2] == e) for e in gc.EPILOGUES}
    print(f"{precision}: worst |d| / bound of the emulation per epilogue {worst}")
    assert max(worst.values()) <= 1.0


MUTATION_ROWS = [gc.case("V1", 129, 132, 128), gc.case("V2_C", 1281, 264, 128), gc.case("V3", 1281, 264, 320)]
# which checks must catch which defect (others may as well)
MUST_CATCH = {"truncating_store": "A", "round_half_away": "A", "drop_last_k_tile": "A", "drop_one_k_element": "A", "bias_shifted_four_columns": "A",
              "swap_two_column_groups_in_last_n_tile": "A", "last_m_tile_row_from_previous_tile": "A", "nan_row_leaks_to_neighbour": "C"}


def _caught(check, *args):
    try:
        check(*args)
    except AssertionError as exc:
        assert str(exc).startswith(("exact:", "bound:", "isolation:")), exc
        return True
    return False


@pytest.mark.parametrize("precision", gc.PRECISIONS)
def test_each_mutation_is_caught_and_by_the_check_that_is_there_for_it(precision):
    table = {}
    for c in MUTATION_ROWS:
        ints, reals = gc.int_operands(c, precision), gc.real_operands(c, precision)
        for mutation in gc.MUTATIONS:
            run = gc.emulation(mutation)
            table[(c.id, mutation)] = "".join(name for name, hit in (("A", _caught(gc.check_exact, run, ints, gc.EXACT_EPILOGUES)),
                                                                     ("B", _caught(gc.check_bound, run, reals, gc.EPILOGUES)),
                                                                     ("C", _caught(gc.check_isolation, run, reals))) if hit)
    print(f"{precision}: checks that catch each mutation")
    for (cid, mutation), hits in table.items():
        print(f"  {cid:24s} {mutation:40s} {hits or '-'}")
    for (cid, mutation), hits in table.items():
        assert MUST_CATCH[mutation] in hits, (cid, mutation, hits)
    # B alone sees a truncating store (on the 16-bit outputs) but never ties rounded away: random data has none to speak of
    assert all("B" in hits for (_, mutation), hits in table.items() if mutation == "truncating_store")
    assert all("B" not in hits for (_, mutation), hits in table.items() if mutation == "round_half_away")


@pytest.mark.parametrize("precision", gc.PRECISIONS)
def test_one_lost_k_element_is_the_reason_for_check_a(precision):
    """B's accumulation term is 2 K^2 2^-24 mean products wide: 0.002 of one at K = 128, where B still sees the lost element of the
    table above, 0.04 at K = 576, 1.1 at K = 3072.  From the ViT's K on, a lost a[m - 1, k*] w[., k*] of a small |a| stays inside every
    bound of B for every epilogue, while on the integer operands it is a whole product in every column with w[., k*] != 0."""
    c = gc.case("V3", 8449, 1024, 576)
    run = gc.emulation("drop_one_k_element")
    reals, ints = gc.real_operands(c, precision), gc.int_operands(c, precision)
    assert gc.check_bound(run, reals, gc.EPILOGUES) <= 1.0
    with pytest.raises(AssertionError, match="^exact:"):
        gc.check_exact(run, ints, ("BF16",))
    with pytest.raises(AssertionError, match="^exact:"):
        gc.check_exact(run, ints, ("RESADD_F32",))


@pytest.mark.parametrize("precision", gc.PRECISIONS)
def test_gemm_ln_reference_is_the_fp32_statement(precision):
    """the float64 reference of the gemm_ln cases against torch's fp32 layer_norm of the fp32 product: inside the tolerance the GPU test uses"""
    import torch
    import torch.nn.functional as F
    for m, n, k in gc.LN_CASES[::4]:
        t = gc.ln_operands(m, n, k, precision)
        ref32 = t["x0"] + F.layer_norm(t["a"].float() @ t["w"].float().t() + t["bias"], (n,), t["gamma"], t["beta"], 1e-5)
        torch.testing.assert_close(ref32.double(), gc.ln_reference64(t), rtol=1e-4, atol=1e-4)
