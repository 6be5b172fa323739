"""Temporal-network (TN) alignment, host side: the fixture's inputs rebuild bit for bit, the documented contract
(tests/tn_contract.py) reproduces the reference's boxes, parameters outside the kernel's limits are refused, and the
`--alignment` switch of the eval entry point.  With VSC_RUN_REFERENCE_CODE=1 and the reference tree present, the
generator reproduces tests/golden/tn_align.json from the reference's own `tn`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import tn_cases
import tn_contract

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLD, "tn_align.json")
OPT_IN = "VSC_RUN_REFERENCE_CODE"


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_inputs_rebuild(fixture):
    cases = tn_cases.cases()
    assert [c["name"] for c in cases] == [c["name"] for c in fixture["cases"]]
    assert len(cases) >= 150
    for c, rec in zip(cases, fixture["cases"]):
        assert tn_cases.digest(tn_cases.matrix(c)) == rec["digest"], c["name"]
        assert c["params"] == rec["params"] and c["bias"] == rec["bias"], c["name"]
    assert fixture["reference_sha256"] == "1a86a766f183f1de7d749f2d2fc0cfffe0d923e8058fe36d0bd8da1748283418"
    assert fixture["numpy"] and fixture["networkx"]


def test_fixture_covers_the_issue_cases(fixture):
    names = [c["name"] for c in fixture["cases"]]
    for prefix in ("diag1_b05", "diag1_b0", "diag2", "overlap", "stretch", "quant", "dup", "const", "q1_", "r1_", "rltk",
                   "qlestep", "lastnode", "tnvta", "large_300x1200", "large_1000x4000"):
        assert any(n.startswith(prefix) for n in names), prefix
    assert any(c["default_sort_differs"] for c in fixture["cases"])      # the tie rule matters on these inputs


def test_contract_statement_reproduces_reference(fixture):
    """The contract as include/vsc_hip.h states it, executed on the host, gives the reference's boxes (small cases)."""
    for c in fixture["cases"]:
        if c["q"] * c["r"] > 20000:
            continue
        boxes, _ = tn_contract.tn_contract(tn_cases.matrix(c), c["bias"], **c["params"])
        assert boxes == c["boxes"], c["name"]


@pytest.mark.parametrize("kw,match", [(dict(tn_top_k=17), "tn_top_k"), (dict(tn_top_k=0), "tn_top_k"),
                                      (dict(tn_max_step=0), "tn_max_step"), (dict(tn_max_step=18, tn_top_k=4), "predecessor bits"),
                                      (dict(tn_max_step=11, tn_top_k=7), "predecessor bits"), (dict(max_path=-1), "max_path"),
                                      (dict(min_length=-1), "min_length")])
def test_parameters_outside_limits_refused(kw, match):
    from vsc_hip.alignment import TnAlignment
    with pytest.raises(ValueError, match=match):
        TnAlignment(**kw)


def test_parameter_limits_cover_baseline_and_defaults():
    from vsc_hip.alignment import TnAlignment, check_shape
    TnAlignment(tn_max_step=5, min_length=4)          # sscd_baseline: (5 - 1) * 5 = 20 bits
    TnAlignment()                                      # TnVtaModel defaults: (10 - 1) * 5 = 45 bits
    TnAlignment(tn_max_step=17, tn_top_k=4)            # 64 bits, the limit
    check_shape(4096, 65536)
    with pytest.raises(ValueError, match="outside"):
        check_shape(70000, 10)


def test_library_refuses_parameters_outside_limits():
    """The C entry point validates before touching the device, so the refusal is visible without a GPU."""
    import ctypes

    from vsc_hip import _lib
    if not all(os.path.exists(p) for p in _lib.LIB_PATHS.values()):
        import __graft_entry__
        __graft_entry__.build()
    for precision in _lib.LIB_PATHS:
        lib = _lib.load(precision)
        pairs = np.array([[0, 4, 4]], dtype=np.int64)
        rc = lib.vsc_tn_align_f32(None, 16, pairs.ctypes.data, 1, 0.5, 5, 17, 10, 0.2, 4, 0.3, None, None, None, None)
        assert rc != 0 and b"top_k" in lib.vsc_last_error()
        rc = lib.vsc_tn_align_f32(None, 16, pairs.ctypes.data, 1, 0.5, 18, 4, 10, 0.2, 4, 0.3, None, None, None, None)
        assert rc != 0 and b"predecessor bits" in lib.vsc_last_error()
        rc = lib.vsc_tn_align_f32(None, 16, pairs.ctypes.data, 1, 0.5, 5, 5, 10, 0.2, -1, 0.3, None, None, None, None)
        assert rc != 0 and b"min_length" in lib.vsc_last_error()
        big = np.array([[0, 4, 5]], dtype=np.int64)          # 4 x 5 = 20 similarities, 16 available
        out = ctypes.c_void_p(1)                              # never dereferenced: the bounds check fails first
        rc = lib.vsc_tn_align_f32(out, 16, big.ctypes.data, 1, 0.5, 5, 5, 10, 0.2, 4, 0.3, out, out, out, None)
        assert rc != 0 and b"outside" in lib.vsc_last_error()
        assert lib.vsc_tn_align_f32(None, 0, None, 0, 0.5, 5, 5, 10, 0.2, 4, 0.3, None, None, None, None) == 0


def test_alignment_switch_parses():
    import vsc.baseline.sscd_baseline as entry
    base = ["--query_features", "q.npz", "--ref_features", "r.npz", "--output_path", "out"]
    assert entry.build_parser().parse_args(base).alignment == "vcsl"
    assert entry.build_parser().parse_args(base + ["--alignment", "hip"]).alignment == "hip"
    with pytest.raises(SystemExit):
        entry.build_parser().parse_args(base + ["--alignment", "dtw"])


def test_eval_script_forwards_alignment():
    text = open(os.path.join(ROOT, "vsc22-submission_amd", "eval.sh")).read()
    assert '--alignment "${ALIGNMENT:-vcsl}"' in text


@pytest.mark.skipif(not (os.path.isdir("/root/reference") and os.environ.get(OPT_IN) == "1"),
                    reason=f"executes reference code: needs /root/reference and {OPT_IN}=1")
def test_generator_reproduces_fixture(tmp_path):
    env = {"PATH": "/usr/bin:/bin", "HOME": str(tmp_path), "TMPDIR": str(tmp_path), OPT_IN: "1",
           "PYTHONDONTWRITEBYTECODE": "1"}
    r = subprocess.run([sys.executable, os.path.join(GOLD, "gen_tn_golden.py"), "--check"], env=env, cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "reproduced" in r.stdout
