"""(CPU) The PCA fit's contract (tests/pca_contract.py) against sklearn's exact solver, the recorded exact-fit uAP of the small
end-to-end fixture, the model file, and the entry point's refusals.  The device side is tests/test_gpu_pca_fit.py."""
import json
import os
import sys

import numpy as np
import pytest

import pca_contract

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(600, 48, 16, 0.93), (700, 96, 24, 0.96), (4100, 160, 40, 0.97)]


@pytest.mark.parametrize("n,d,k,ratio", SHAPES)
def test_contract_equals_sklearn_full_solver(n, d, k, ratio):
    from sklearn.decomposition import PCA
    x = pca_contract.spectrum_data(50 + d, n, d, ratio).astype(np.float64)
    got = pca_contract.fit(x, k)
    want = PCA(n_components=k, svd_solver="full").fit(x)
    errs = (np.abs(got.components_ - want.components_).max(), np.abs(got.explained_variance_ / want.explained_variance_ - 1).max(),
            np.abs(got.mean_ - want.mean_).max())
    auto = PCA(n_components=k, random_state=2023).fit(x.astype(np.float32))       # the reference's call: float32 in, default solver
    print(f"{n} x {d} -> {k}: vs svd_solver='full' components {errs[0]:.1e}, variances (relative) {errs[1]:.1e}, mean {errs[2]:.1e}; "
          f"sklearn's default solver ({auto._fit_svd_solver}, float32) is {np.abs(auto.components_ - got.components_).max():.1e} from the contract")
    assert max(errs) <= 1e-10
    np.testing.assert_allclose(pca_contract.transform(got, x[:50]), want.transform(x[:50]), atol=1e-10)
    assert got.whiten is False and got.n_components_ == k and got.n_samples_ == n


def test_sign_rule_flips_a_component_whose_largest_coordinate_is_negative():
    """Data along (-3, 1, 1) / sqrt(11): whichever sign eigh returns, the contract (and vsc_hip.pca_fit, and sklearn 1.7's
    svd_flip(u_based_decision=False)) reports the component with its largest-magnitude coordinate positive: (3, -1, -1) / sqrt(11).
    A tie in magnitude goes to the first index."""
    from sklearn.decomposition import PCA
    from vsc_hip.pca_fit import components_from_covariance
    t = np.linspace(-1, 1, 41)[:, None]
    axis = np.array([-3.0, 1.0, 1.0]) / np.sqrt(11.0)
    x = t * axis + 1e-3 * np.sin(7 * t) * np.array([0.0, 1.0, -1.0])
    got = pca_contract.fit(x, 2)
    assert np.allclose(got.components_[0], -axis, atol=1e-3) and got.components_[0, 0] > 0
    assert np.allclose(PCA(n_components=2, svd_solver="full").fit(x).components_, got.components_, atol=1e-10)
    # the same rule whatever sign the eigenvectors arrive with (numpy.linalg.eigh is free to return either)
    import unittest.mock
    w, v = np.linalg.eigh(pca_contract.covariance(x)[1])
    for flip in (1.0, -1.0):
        with unittest.mock.patch("numpy.linalg.eigh", lambda a, w=w, v=v, flip=flip: (w, v * flip)):
            assert np.array_equal(pca_contract.fit(x, 2).components_, got.components_)
            assert np.array_equal(components_from_covariance(pca_contract.covariance(x)[1], 2)[0], got.components_)
    s = np.sqrt(0.5)                # an exact tie in magnitude: (-s, s, 0) -> the first index decides -> (s, -s, 0)
    with unittest.mock.patch("numpy.linalg.eigh", lambda a: (np.array([0.0, 0.5, 2.0]), np.array([[0.0, s, -s], [0.0, s, s], [1.0, 0.0, 0.0]]))):
        for comps in (components_from_covariance(np.eye(3), 1)[0], pca_contract.fit(x, 1).components_):
            assert np.array_equal(comps, [[s, -s, 0.0]])


def test_recorded_exact_fit_uap_is_recomputed():
    """tests/golden/uap_e2e_exact_pca.json is what gen_uap_exact_pca_golden.py computes from the small fixture's stored descriptors:
    the reference chain with the exact fit gives uAP 0.7524107 where sklearn's randomized fit (the fixture's own number) gives
    0.7510685 -- more than the 1e-3 criterion apart, which is why the device fit has a yardstick of its own."""
    from oracle import knn_oracle
    try:
        knn_oracle.knn_ip(np.eye(2, dtype=np.float32), np.eye(2, dtype=np.float32), 1)
    except Exception as e:      # no C compiler: the knn oracle's library cannot be built
        pytest.skip(f"knn oracle unavailable: {e}")
    sys.path.insert(0, GOLDEN)
    import gen_uap_exact_pca_golden as G
    gold = json.load(open(G.OUT))
    got = G.compute(exact=True)
    assert abs(got["uap"] - gold["uap"]) <= 1e-9
    for key in ("pca_dim", "n_candidates", "gt_ranks", "low_var_dim", "kept_counts", "top_candidates"):
        assert got[key] == gold[key], key
    fixture = np.load(os.path.join(GOLDEN, "uap_e2e.npz"))
    assert abs(gold["uap_sklearn"] - float(fixture["uap"])) <= 1e-9 and gold["low_var_dim"] == int(fixture["low_var_dim"])
    assert gold["kept_counts"] == fixture["kept_counts"].tolist() and gold["sklearn_same_low_var_dim"] and gold["sklearn_same_kept_counts"]
    assert abs(gold["uap"] - 0.7524107) < 5e-8 and gold["uap"] - gold["uap_sklearn"] > 1e-3


def _model(seed=3, d=40, k=12):
    from vsc_hip.pca_fit import FittedPCA
    w = pca_contract.fit(pca_contract.spectrum_data(seed, 300, d, 0.95), k)
    return FittedPCA(w.mean_, w.components_, w.explained_variance_, whiten=False, n_components_=k, n_samples_=300)


def test_model_file_round_trip(tmp_path):
    from src.query_postprocess import HipPCA, load_pca_model, save_pca_model
    fitted = _model()
    loaded = {}
    for ext in ("npz", "pkl"):
        path = str(tmp_path / f"pca.{ext}")
        save_pca_model(fitted, path)
        loaded[ext] = load_pca_model(path)
    assert sorted(np.load(str(tmp_path / "pca.npz"), allow_pickle=False).files) == sorted(type(fitted).FIELDS)
    hips = [HipPCA(m) for m in (fitted, loaded["npz"], loaded["pkl"])]
    for h in hips[1:]:
        assert np.array_equal(h.mean_, hips[0].mean_) and np.array_equal(h.components_, hips[0].components_) and h.scale_ is None
        assert h.mean_.dtype == np.float32 and h.components_.dtype == np.float32
    for m in loaded.values():
        assert np.array_equal(m.explained_variance_, fitted.explained_variance_) and m.whiten is False
        assert m.n_components_ == 12 and m.n_samples_ == 300
    with pytest.raises(ValueError, match="not a PCA model file"):
        np.savez(str(tmp_path / "other.npz"), a=np.zeros(3))
        load_pca_model(str(tmp_path / "other.npz"))


def test_sklearn_pickle_still_loads(tmp_path):
    """the reference's own model file: a pickled sklearn PCA goes through load_pca_model / save_pca_model unchanged"""
    import pickle
    from sklearn.decomposition import PCA
    from src.query_postprocess import HipPCA, load_pca_model, save_pca_model
    x = pca_contract.spectrum_data(5, 200, 32, 0.9)
    p = PCA(n_components=8, random_state=2023).fit(x)
    save_pca_model(p, str(tmp_path / "pca_model.pkl"))
    assert open(tmp_path / "pca_model.pkl", "rb").read() == pickle.dumps(p)
    assert np.array_equal(HipPCA(load_pca_model(str(tmp_path / "pca_model.pkl"))).components_, p.components_.astype(np.float32))


def test_npz_model_needs_neither_pickle_nor_sklearn(tmp_path, monkeypatch):
    from src.query_postprocess import HipPCA, load_pca_model, save_pca_model
    fitted = _model()
    monkeypatch.setitem(sys.modules, "pickle", None)
    monkeypatch.setitem(sys.modules, "sklearn", None)
    path = str(tmp_path / "pca_model.npz")
    save_pca_model(fitted, path)
    assert np.array_equal(HipPCA(load_pca_model(path)).components_, fitted.components_)
    with pytest.raises(ImportError):
        load_pca_model(str(tmp_path / "pca_model.pkl"))


def test_fit_on_the_device_refuses_a_pickle_path_and_needs_a_device(tmp_path, monkeypatch):
    """--fit_pca --pca_fit hip: a model path that is not .npz is refused before any work; without a device the fit raises
    HipPathUnavailable (no quiet fall-back to sklearn, which is not even importable here)."""
    import torch
    import concat_pca_sn as C
    from vsc_hip._lib import HipPathUnavailable
    monkeypatch.setitem(sys.modules, "sklearn", None)
    base = ["--root", str(tmp_path / "nowhere"), "--models", "m_a", "m_b", "--fit_pca", "--pca_fit", "hip", "--dim", "16"]
    with pytest.raises(SystemExit, match=r"\.npz"):
        C.main(C.build_parser().parse_args(base + ["--pca_model", str(tmp_path / "pca_model.pkl")]))
    assert C.build_parser().parse_args(["--fit_pca"]).pca_fit == "sklearn"
    with pytest.raises(SystemExit):
        C.build_parser().parse_args(["--pca_fit", "cuda"])
    if not torch.cuda.is_available():
        with pytest.raises(HipPathUnavailable):
            C.main(C.build_parser().parse_args(base + ["--pca_model", str(tmp_path / "pca_model.npz")]))
        from vsc_hip.pca_fit import HipPCAFit
        with pytest.raises(HipPathUnavailable):
            HipPCAFit(64)


def test_video_blocks_cover_every_video_once():
    import concat_pca_sn as C
    lens = [6, 7, 8, 30, 1, 1]
    for limit in (1, 7, 14, 1000):
        blocks = list(C.video_blocks(lens, limit))
        assert [lo for lo, _ in blocks] == [0] + [hi for _, hi in blocks[:-1]] and blocks[-1][1] == len(lens)
        assert all(hi - lo == 1 or sum(lens[lo:hi]) <= limit for lo, hi in blocks)
