"""Device score normalisation, the parts that need no GPU: the executable contract (tests/score_norm_contract.py) against numpy
itself -- bit for bit, on data whose column means sit at ten standard deviations, so that any other summation order shows -- and the
host plumbing of ``device="hip"`` / ``--score_norm hip``: the refusals, the parsers, namespaces from before the option, the symbols
of both libraries, the zero-copy view of a loaded set."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import score_norm_cases as cases  # noqa: E402
import score_norm_contract as C  # noqa: E402

NEW_SYMBOLS = ("vsc_column_var_f32", "vsc_score_norm_rows_f32", "vsc_score_norm_bias_f32", "vsc_score_norm_create", "vsc_score_norm_destroy")


@pytest.mark.parametrize("n,d", [(1, 4), (1, 1), (2, 3), (7, 64), (513, 65), (4099, 130), (70001, 17), (20000, 512)])
def test_contract_variance_is_numpys(n, d):
    x = np.ascontiguousarray(cases.offset_rows(n, d))
    assert n < 64 or (abs(x.mean(axis=0)) > 8 * x.std(axis=0)).all()          # the offset the summation order shows on
    want = x.var(axis=0)
    assert np.array_equal(C.bits(C.column_var(x)), C.bits(want))
    assert C.low_variance_dim(x) == int(want.argmin())


def test_contract_variance_ties_and_refusal():
    x = np.ascontiguousarray(cases.offset_rows(300, 9))
    x[:, 7] = x[:, 2]
    x[:, [2, 7]] *= np.float32(1e-4)
    assert C.low_variance_dim(x) == 2 == int(x.var(axis=0).argmin())
    with pytest.raises(ValueError):
        C.column_var(np.zeros((0, 4), np.float32))


@pytest.mark.parametrize("nk", [1, 2, 3, 5, 7, 8, 9, 10, 16, 17, 128])
def test_contract_mean_and_bias_are_numpys(nk):
    sims, gate = cases.topk_scores(2000, nk, nk)
    assert sims.mean() > 10 * sims.std()                               # scores near 0.9 +- 0.05: every partial sum rounds
    assert np.array_equal(C.bits(C.row_mean(sims, nk)), C.bits(sims[:, :nk].mean(axis=1)))
    wide, _ = cases.topk_scores(500, nk, nk + 5)
    for beta in (1.0, 1.2, 1.5):
        want = -beta * sims[:, :nk].mean(axis=1, keepdims=True)       # the expression of _bias_terms
        assert want.dtype == np.float32
        assert np.array_equal(C.bits(C.bias(sims, nk, beta)), C.bits(want[:, 0]))
        assert np.array_equal(C.bits(C.bias(wide, nk, beta)), C.bits(-beta * wide[:, :nk].mean(axis=1)))
    gated = C.bias(sims, nk, 1.2, gate)
    ones = -100.0 * np.ones_like(sims[:, :1])                          # the expression of query_score_normalize
    assert np.array_equal(C.bits(gated[gate != 0]), C.bits(ones[gate != 0, 0]))
    assert np.array_equal(C.bits(gated[gate == 0]), C.bits(C.bias(sims, nk, 1.2)[gate == 0]))
    with pytest.raises(ValueError):
        C.row_sum(np.zeros((2, 130), np.float32), 129)


@pytest.mark.parametrize("d", cases.ROWS_D)
def test_contract_rows_put_every_column_where_numpy_puts_it(d):
    """with the normalisation injected: np.delete -> normalize -> np.concatenate"""
    x = np.ascontiguousarray(cases.descriptor_rows(d, d))
    marker = lambda a: (a * np.float32(0.5) + np.float32(3.0)).astype(np.float32)      # any row-wise map of the narrowed rows
    last = np.linspace(-5, 5, len(x)).astype(np.float32)
    for drop in cases.drops(d):
        narrowed = np.delete(x, drop, axis=1) if drop >= 0 else x
        for normalize in (False, True):
            body = marker(narrowed) if normalize else narrowed
            for append, col in ((0, None), (1, np.ones_like(body[:, :1])), (2, last[:, None])):
                want = body if col is None else np.concatenate([body, col], axis=1)
                got = C.rows(x, drop, normalize, append, last, normalize_fn=marker)
                assert got.dtype == np.float32 and np.array_equal(C.bits(got), C.bits(want)), (d, drop, normalize, append)


def test_contract_normalisation_properties():
    """what can be said of the contract's l2_normalize without the device: a zero row and a row whose squares underflow stay as they
    are, other rows come out at unit length, fma32 rounds once"""
    x = np.ascontiguousarray(cases.descriptor_rows(129, 129))
    y = C.l2_normalize(x)
    assert np.array_equal(C.bits(y[[2, 4]]), C.bits(x[[2, 4]]))
    assert np.allclose(np.linalg.norm(y[[0, 1, 3, 5]].astype(np.float64), axis=1), 1.0, atol=1e-6)
    import fractions
    rs = np.random.RandomState(5)
    a, b, c = (rs.standard_normal(2000).astype(np.float32) * np.float32(10.0) ** rs.randint(-6, 6, 2000).astype(np.float32) for _ in range(3))
    got = C.fma32(a, b, c)
    for i in range(0, 2000, 7):
        exact = fractions.Fraction(float(a[i])) * fractions.Fraction(float(b[i])) + fractions.Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        err = abs(fractions.Fraction(float(got[i])) - exact)
        assert err <= abs(fractions.Fraction(float(lo)) - exact) and err <= abs(fractions.Fraction(float(hi)) - exact)


def _videos(lens, d, seed=0, prefix="R"):
    from vsc.index import VideoFeature
    rs = np.random.RandomState(seed)
    base = rs.standard_normal((sum(lens), d)).astype(np.float32)
    out, lo = [], 0
    for i, n in enumerate(lens):
        out.append(VideoFeature(video_id=f"{prefix}{i:06d}", timestamps=np.arange(n, dtype=np.float32), feature=base[lo:lo + n]))
        lo += n
    return base, out


def test_host_rows_is_the_base_array_when_the_videos_are_consecutive_views():
    from vsc.baseline.score_normalization import host_rows
    base, videos = _videos([3, 0, 5, 1], 8)
    assert host_rows(videos) is not None and np.shares_memory(host_rows(videos), base) and host_rows(videos).shape == (9, 8)
    assert np.shares_memory(host_rows(videos[2:]), base) and np.array_equal(host_rows(videos[2:]), base[3:9])
    swapped = [videos[2], videos[0]]                                   # views of one base, but not consecutive: one concatenation
    got = host_rows(swapped)
    assert not np.shares_memory(got, base) and np.array_equal(got, np.concatenate([base[3:8], base[:3]]))
    import dataclasses
    copies = [dataclasses.replace(v, feature=v.feature.astype(np.float64)) for v in videos]
    got = host_rows(copies)
    assert got.dtype == np.float32 and got.flags.c_contiguous and np.array_equal(got, base)


def test_device_argument_is_checked_and_hip_has_no_cpu_fallback():
    import torch
    from vsc.baseline import score_normalization as sn
    from vsc_hip._lib import HipPathUnavailable
    _, refs = _videos([4, 3], 8)
    _, norm = _videos([5, 2], 8, seed=1)
    import dataclasses
    norm = [dataclasses.replace(v, video_id="N" + v.video_id) for v in norm]
    scores = {v.video_id: 1.0 for v in refs}
    for call in (lambda dev: sn.low_variance_dim(norm, device=dev),
                 lambda dev: sn.ref_score_normalize(refs, norm, device=dev),
                 lambda dev: sn.query_score_normalize(refs, norm, scores, device=dev),
                 lambda dev: sn.score_normalize(refs, refs, norm, device=dev)):
        with pytest.raises(ValueError, match="bogus"):
            call("bogus")
        if not torch.cuda.is_available():
            with pytest.raises(HipPathUnavailable):
                call("hip")
    from src import matching
    with pytest.raises(ValueError, match="bogus"):
        matching.calclualte_low_var_dim(norm, device="bogus")
    if not torch.cuda.is_available():
        with pytest.raises(HipPathUnavailable):
            matching.calclualte_low_var_dim(norm, device="hip")
        with pytest.raises(HipPathUnavailable):
            sn.ScoreNormBank(norm)
    assert sn.low_variance_dim(norm) == matching.calclualte_low_var_dim(norm) == C.low_variance_dim(np.concatenate([v.feature for v in norm]))


def test_all_four_parsers_take_score_norm_and_default_to_host():
    import concat_pca_sn
    import extract_query_feats
    import infer_matching
    from vsc.baseline import sscd_baseline
    bases = {
        concat_pca_sn: [],
        extract_query_feats: ["--models", "a:b:c", "--pca_model", "p.npz", "--input_file", "ids.txt"],
        infer_matching: ["--query_features", "q", "--norm_refs", "n", "--refs", "r", "--sn_refs", "s", "--cls_models", "c",
                         "--refine_models", "m", "--output", "o"],
        sscd_baseline: ["--query_features", "q.npz", "--ref_features", "r.npz", "--output_path", "out"],
    }
    for module, base in bases.items():
        parser = module.build_parser()
        assert parser.parse_args(base).score_norm == "host", module.__name__
        assert parser.parse_args(base + ["--score_norm", "hip"]).score_norm == "hip", module.__name__
        with pytest.raises(SystemExit):
            parser.parse_args(base + ["--score_norm", "cuda"])
    import inspect
    assert inspect.signature(infer_matching.run).parameters["score_norm"].default == "host"
    for script in ("infer_ref.sh", "infer_query.sh"):
        text = open(os.path.join(os.path.dirname(HERE), "vsc22-submission_amd", script)).read()
        assert '--score_norm "${SCORE_NORM:-host}"' in text, script


def test_namespace_from_before_the_option_runs_the_host_path(tmp_path, monkeypatch):
    """main() of the entry points is also called with hand-built namespaces: without `score_norm` they normalise on the host"""
    from vsc.baseline import sscd_baseline
    from vsc.storage import store_features
    store_features(str(tmp_path / "f.npz"), _videos([4, 3], 8)[1])
    store_features(str(tmp_path / "q.npz"), _videos([2, 3], 8, prefix="Q")[1])
    seen = {}

    class Reached(Exception):
        pass

    def spy(*a, **kw):
        seen.update(kw)
        raise Reached

    monkeypatch.setattr(sscd_baseline, "score_normalize", spy)
    old = types.SimpleNamespace(query_features=str(tmp_path / "q.npz"), ref_features=str(tmp_path / "f.npz"),
                                score_norm_features=str(tmp_path / "f.npz"), output_path=str(tmp_path / "out"), overwrite=True,
                                ground_truth=None, alignment="vcsl")
    with pytest.raises(Reached):
        sscd_baseline.main(old)
    assert seen["device"] == "host"
    old.score_norm = "hip"
    with pytest.raises(Reached):
        sscd_baseline.main(old)
    assert seen["device"] == "hip"


def test_index_adopts_only_what_fits(monkeypatch):
    """FlatIPBank.adopt_device_rows: inner-product banks only, the shape of the added rows only; add() drops the adopted bank"""
    from vsc.index import METRIC_L2, FlatIPBank

    class FakeRows:                                                    # what the method looks at, without a device
        is_cuda, shape = True, (7, 8)

        def __init__(self):
            import torch
            self.dtype = torch.float32

        def is_contiguous(self):
            return True

    bank = FlatIPBank(8)
    bank.add(np.zeros((7, 8), np.float32))
    rows = FakeRows()
    bank.adopt_device_rows(rows)
    assert bank.adopted and bank.device_bank() is rows                 # no upload: the device bank IS the adopted tensor
    bank.add(np.zeros((1, 8), np.float32))
    assert not bank.adopted and bank._bank is None
    with pytest.raises(ValueError, match="expected a contiguous float32"):
        bank.adopt_device_rows(rows)                                   # 8 rows now
    l2 = FlatIPBank(8, METRIC_L2)
    l2.add(np.zeros((7, 8), np.float32))
    with pytest.raises(ValueError, match="inner-product"):
        l2.adopt_device_rows(rows)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_both_libraries_export_the_new_symbols(precision):
    from vsc_hip import _lib
    if not all(os.path.exists(p) for p in _lib.LIB_PATHS.values()):
        import __graft_entry__
        __graft_entry__.build()
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATHS[precision]], text=True)
    for name in NEW_SYMBOLS:
        assert f" T {name}\n" in nm, (precision, name)
        assert name in _lib.SIGNATURES and hasattr(_lib.load(precision), name)
