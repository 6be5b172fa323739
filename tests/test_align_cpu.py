"""DP and HV temporal alignment, host side: the fixture's inputs rebuild bit for bit, the documented contracts
(tests/align_contract.py) reproduce the reference's boxes on every case, parameters and shapes outside the kernels' limits are
refused, `build_alignment` mirrors `build_vta_model`, and the `--alignment_model` switch of the eval entry point.  With
VSC_RUN_REFERENCE_CODE=1 and the reference tree present, the generator reproduces tests/golden/align_dp_hv.json from the
reference's own `dp` and `hv`."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import align_cases
import align_contract

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLD, "align_dp_hv.json")
OPT_IN = "VSC_RUN_REFERENCE_CODE"


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def contract(fixture):
    """{name: (boxes, maxsim, stats)} of the contract on every case, computed once."""
    out = {}
    for c in fixture["cases"]:
        stats = {}
        fn = align_contract.dp_contract if c["model"] == "DP" else align_contract.hv_contract
        boxes, maxsim = fn(align_cases.matrix(c), c["bias"], stats=stats, **c["params"])
        out[c["name"]] = (boxes, maxsim, stats)
    return out


def test_fixture_inputs_rebuild(fixture):
    cases = json.loads(json.dumps(align_cases.cases()))          # tuples of the recipes as the lists the fixture holds
    assert [c["name"] for c in cases] == [c["name"] for c in fixture["cases"]]
    assert sum(c["model"] == "DP" for c in cases) >= 60 and sum(c["model"] == "HV" for c in cases) >= 120
    for c, rec in zip(cases, fixture["cases"]):
        assert align_cases.digest(align_cases.matrix(c)) == rec["digest"], c["name"]
        assert all(rec[k] == v for k, v in c.items()), c["name"]
        assert ("wide_differs" in rec) == (c["model"] == "DP")
    assert fixture["reference_sha256"] == "1a86a766f183f1de7d749f2d2fc0cfffe0d923e8058fe36d0bd8da1748283418"
    assert fixture["numpy"]


def test_contracts_reproduce_reference_on_every_case(fixture, contract):
    bad = [c["name"] for c in fixture["cases"] if contract[c["name"]][0] != c["boxes"]]
    assert not bad, f"{len(bad)} of {len(fixture['cases'])} cases differ from the reference: {bad[:5]}"
    assert sum(len(c["boxes"]) for c in fixture["cases"] if c["model"] == "DP") >= 60
    assert sum(len(c["boxes"]) for c in fixture["cases"] if c["model"] == "HV") >= 500


def test_fixture_covers_the_issue_cases(fixture, contract):
    by = {c["name"]: c for c in fixture["cases"]}
    dp = [c for c in fixture["cases"] if c["model"] == "DP"]
    hv = [c for c in fixture["cases"] if c["model"] == "HV"]
    stats = {c["name"]: contract[c["name"]][2] for c in fixture["cases"]}
    for model in (dp, hv):
        assert {(c["q"], c["r"]) for c in model} >= set(align_cases.SHAPES)
    for prefix in ("diag1", "diag2", "overlap", "vrun9", "vrun10", "vrun11", "hrun9", "hrun10", "hrun11", "half", "double", "lshape",
                   "below_300x300", "const", "mask_all", "mask_not", "minsim13", "mean_at_1.3", "mean_at_0.3"):
        assert any(c["name"].startswith(prefix) for c in dp), prefix
    assert len(dp) / 4 <= sum(bool(c.get("grid")) for c in dp) <= len(dp) / 2  # about a third on the 2^-10 grid
    assert any(stats[c["name"]]["crossed"] for c in dp if c["name"].startswith("lshape"))       # cut_path's s > e ranges occur
    assert stats["below_300x300"]["max_acc"] > 255 and stats["below_noise_300x300_g"]["max_acc"] > 255     # an 8-bit wrap would show
    assert any(stats[c["name"]]["stopped"] and stats[c["name"]]["rounds"] > 1 for c in dp if c["name"].startswith("mask_all"))
    assert stats["mask_not_40x120"]["rounds"] == 100 and not stats["mask_not_40x120"]["stopped"]
    assert any(stats[c["name"]]["mean_at_threshold"] for c in dp if c["name"].startswith("mean_at_1.3"))
    assert any(stats[c["name"]]["mean_at_threshold"] for c in dp if c["name"].startswith("mean_at_0.3"))
    assert any(len(c["boxes"]) > 2 for c in dp)                                # the GPU test stores two of them
    assert any(c["wide_differs"] for c in dp)                                  # numba's typing matters on these inputs
    # boxes differ between diagonal_thres - 1, +0 and +1 cells of a vertical run
    assert by["vrun9_b0"]["boxes"] != by["vrun10_b0_g"]["boxes"] or by["vrun8_b0"]["boxes"] != by["vrun11_b0"]["boxes"]
    assert {c["params"]["min_sim"] for c in hv} == {-1.0, 0.0, 0.2}
    assert {c["params"]["max_peaks"] for c in hv} == {1, 3, 100} and {c["params"]["iou_thresh"] for c in hv} == {0.3, 0.9}
    assert sum(stats[c["name"]]["ties"] for c in hv) > 100 and sum(stats[c["name"]]["rejected"] for c in hv) > 100
    assert any(x == -np.inf for c in hv for x in contract[c["name"]][1])        # one-cell corner diagonals: empty MaxSim extent
    neg = [c for c in hv if c["name"].startswith("neg_")]
    assert len(neg) == 18 and not any(c["boxes"] for c in neg)                  # all-negative matrices: no score above 0


def test_pairwise_sum_is_numpys():
    for n in list(range(0, 40)) + [127, 128, 129, 255, 256, 257, 1000, 1299, 5000, 70001]:
        a = np.random.RandomState(n).uniform(-1, 2, n).astype(np.float32)
        assert align_contract.pairwise_f32(list(a)).view(np.uint32) == np.float32(np.sum(a)).view(np.uint32), n
        if n:
            mean = np.float32(align_contract.pairwise_f32(list(a)) / np.float32(n))
            assert mean.view(np.uint32) == np.mean(a).view(np.uint32), n


@pytest.mark.parametrize("cls,kw,match", [("DpAlignment", dict(discontinue=255), "discontinue"), ("DpAlignment", dict(discontinue=-1), "discontinue"),
                                          ("DpAlignment", dict(min_length=-1), "min_length"), ("DpAlignment", dict(diagonal_thres=-1), "diagonal_thres"),
                                          ("DpAlignment", dict(max_boxes=0), "max_boxes"), ("DpAlignment", dict(max_boxes=4097), "max_boxes"),
                                          ("HvAlignment", dict(max_peaks=0), "max_peaks"), ("HvAlignment", dict(max_peaks=4097), "max_peaks")])
def test_parameters_outside_limits_refused(cls, kw, match):
    import vsc_hip.alignment as alignment
    with pytest.raises(ValueError, match=match):
        getattr(alignment, cls)(**kw)


def test_defaults_are_the_reference_models():
    from vsc_hip.alignment import DpAlignment, HvAlignment, check_align_shape
    d = DpAlignment()
    assert (d.discontinue, d.min_sim, d.min_length, d.ave_sim, d.diagonal_thres) == (3, 0.0, 5, 0.3, 10)
    DpAlignment(max_iou=0.3, sum_sim=8, discontinue=254)          # accepted and unused; the limit
    h = HvAlignment()
    assert (h.iou_thresh, h.min_sim, h.max_peaks, h.max_boxes) == (0.9, 0.0, 100, 100)
    HvAlignment(min_bins=1, min_peaks=10, max_peaks=4096)
    check_align_shape(65536, 1024)
    check_align_shape(0, 70)
    with pytest.raises(ValueError, match="rows and columns"):
        check_align_shape(65537, 1)
    with pytest.raises(ValueError, match="cells"):
        check_align_shape(65536, 1025)
    for model in (d, h):
        with pytest.raises(ValueError, match="cells"):
            model.align(None, [[0, 9000, 9000]])


def test_build_alignment_mirrors_build_vta_model():
    from vsc_hip.alignment import DpAlignment, HvAlignment, TnAlignment, build_alignment
    assert isinstance(build_alignment("TN", tn_max_step=5, min_length=4, concurrency=16), TnAlignment)
    dp = build_alignment("DP", min_length=4, concurrency=16, version="v1")
    assert isinstance(dp, DpAlignment) and dp.min_length == 4
    assert isinstance(build_alignment("HV", max_peaks=3), HvAlignment)
    with pytest.raises(NotImplementedError, match="tslearn"):
        build_alignment("DTW")
    with pytest.raises(NotImplementedError, match="tslearn"):
        build_alignment()                                         # the reference's default method
    with pytest.raises(ValueError, match="Unknown method"):
        build_alignment("SPD")


def test_library_refuses_parameters_outside_limits():
    """The C entry points validate before touching the device, so the refusals are visible without a GPU."""
    from vsc_hip import _lib
    if not all(os.path.exists(p) for p in _lib.LIB_PATHS.values()):
        import __graft_entry__
        __graft_entry__.build()
    for precision in _lib.LIB_PATHS:
        lib = _lib.load(precision)
        h = ctypes.c_void_p()
        assert lib.vsc_align_create(None, ctypes.byref(h)) == 0
        pairs = np.array([[0, 4, 4]], dtype=np.int64)
        out = ctypes.c_void_p(1)                                  # never dereferenced: the checks fail first

        def dp(pairs=pairs, n=1, sims_len=16, discontinue=3, min_length=5, diagonal_thres=10, max_boxes=100, handle=h):
            return lib.vsc_align_dp_f32(handle, out, sims_len, pairs.ctypes.data, n, 0.5, discontinue, 0.0, 0.3, min_length, diagonal_thres,
                                        max_boxes, out, out, out)

        def hv(pairs=pairs, n=1, sims_len=16, max_peaks=100, handle=h):
            return lib.vsc_align_hv_f32(handle, out, sims_len, pairs.ctypes.data, n, 0.5, 0.0, 0.9, max_peaks, out, out, out)

        for call, match in [(lambda: dp(discontinue=255), b"discontinue"), (lambda: dp(discontinue=-1), b"discontinue"),
                            (lambda: dp(min_length=-1), b"min_length"), (lambda: dp(diagonal_thres=-1), b"diagonal_thres"),
                            (lambda: dp(max_boxes=0), b"max_boxes"), (lambda: dp(max_boxes=4097), b"max_boxes"),
                            (lambda: hv(max_peaks=0), b"max_peaks"), (lambda: hv(max_peaks=4097), b"max_peaks"),
                            (lambda: dp(handle=None), b"null handle"), (lambda: hv(handle=None), b"null handle")]:
            assert call() != 0 and match in lib.vsc_last_error(), match
        for table, match in [([[0, 65537, 1]], b"rows and columns"), ([[0, 1, 65537]], b"rows and columns"),
                             ([[0, 65536, 1025]], b"cells"), ([[0, 4, 5]], b"outside"), ([[-1, 4, 4]], b"outside"),
                             ([[0, 4, 4], [8, 3, 3]], b"outside")]:
            t = np.array(table, dtype=np.int64)
            for entry in (dp, hv):
                assert entry(pairs=t, n=len(t)) != 0 and match in lib.vsc_last_error(), (table, match)
        assert dp(n=0) == 0 and hv(n=0) == 0
        launches, used = ctypes.c_int64(-1), ctypes.c_int64(-1)
        assert lib.vsc_align_scratch(h, 0, ctypes.byref(launches), ctypes.byref(used)) == 0 and launches.value == 0
        assert lib.vsc_align_scratch(h, -1, None, None) != 0 and b"cap_bytes" in lib.vsc_last_error()
        assert lib.vsc_align_scratch(h, 1 << 20, None, None) == 0
        lib.vsc_align_destroy(h)


def test_wrappers_refuse_slot_counts_before_allocating():
    from vsc_hip import ops
    with pytest.raises(ValueError, match="box slots"):
        ops._align_call("vsc_align_dp_f32", None, [[0, 0, 0]], 0, (), None)


def test_alignment_model_switch_parses():
    import vsc.baseline.sscd_baseline as entry
    base = ["--query_features", "q.npz", "--ref_features", "r.npz", "--output_path", "out"]
    assert entry.build_parser().parse_args(base).alignment_model == "TN"
    for model in ("TN", "DP", "HV"):
        assert entry.build_parser().parse_args(base + ["--alignment_model", model]).alignment_model == model
    with pytest.raises(SystemExit):
        entry.build_parser().parse_args(base + ["--alignment_model", "DTW"])
    with pytest.raises(ValueError, match="alignment_model"):
        entry.localize_and_verify([], [], [], alignment="hip", alignment_model="DTW")


def test_vcsl_branch_hands_the_model_type_on(monkeypatch):
    """`--alignment vcsl --alignment_model DP`: VCSL's model_type, TN's bias and min_length, otherwise the model's defaults."""
    import vsc.baseline.localization as loc
    import vsc.baseline.sscd_baseline as entry
    seen = []
    monkeypatch.setattr(loc, "_load_vcsl_model", lambda model_type, options: seen.append((model_type, options)) or object())
    entry.localize_and_verify([], [], [], score_normalization=True, alignment_model="DP")
    entry.localize_and_verify([], [], [], score_normalization=True, alignment_model="HV")
    entry.localize_and_verify([], [], [], score_normalization=True)
    assert seen == [("DP", dict(min_length=4, concurrency=16)), ("HV", dict(concurrency=16)),
                    ("TN", dict(tn_max_step=5, min_length=4, concurrency=16))]


def test_eval_script_forwards_alignment_model():
    text = open(os.path.join(ROOT, "vsc22-submission_amd", "eval.sh")).read()
    assert '--alignment_model "${ALIGNMENT_MODEL:-TN}"' in text


@pytest.mark.skipif(not (os.path.isdir("/root/reference") and os.environ.get(OPT_IN) == "1"),
                    reason=f"executes reference code: needs /root/reference and {OPT_IN}=1")
def test_generator_reproduces_fixture(tmp_path):
    env = {"PATH": "/usr/bin:/bin", "HOME": str(tmp_path), "TMPDIR": str(tmp_path), OPT_IN: "1",
           "PYTHONDONTWRITEBYTECODE": "1"}
    r = subprocess.run([sys.executable, os.path.join(GOLD, "gen_align_golden.py"), "--check"], env=env, cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "reproduced" in r.stdout
