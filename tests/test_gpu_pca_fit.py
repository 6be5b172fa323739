"""PCA fit on the device (vsc_pca_fit_*, vsc_hip/pca_fit.py, concat_pca_sn.py --fit_pca --pca_fit hip) against float64 numpy and
the executable contract tests/pca_contract.py.

Bounds.  Every element of the raw moments is an fp64 sum of n exact products of fp32 numbers (an fp32 x fp32 product has 48
significant bits: exact in fp64), so for ANY summation order  |S2 - exact| <= n 2^-53 (|X|^T |X|) (1 + O(n 2^-53)); the tests allow
2 n 2^-52 (|X|^T |X|), the same for numpy's own float64 result on the other side, and 2 n 2^-52 sum|x| for the column sums.  An fp32
accumulator misses this by eight orders of magnitude."""
import os
import sys
import types

import numpy as np
import pytest

import pca_contract
from tools import synth

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
# (n, D, ld): n below one K-step (4 rows), ragged K-steps and slabs (16 rows), several row splits (> 256 rows), D below / at / across
# the 128-column tile with a ragged last tile, a strided input
SHAPES = [(1, 16, 16), (3, 20, 20), (67, 48, 48), (1031, 130, 130), (4100, 160, 160), (5000, 272, 288), (20000, 256, 256)]
_CACHE = {}


@pytest.fixture(scope="module")
def dev():
    import torch
    from vsc_hip import _lib
    _lib.require_device()
    return torch.device("cuda:0")


def _case(n, d, ld):
    """(fp32 [n, ld] buffer whose first d columns are the data, float64 sum, float64 S2, |X|^T |X|, sum |x|) -- computed once"""
    key = (n, d, ld)
    if key not in _CACHE:
        buf = synth.normalish(7000 + n + d, (n, ld)) * (1.0 + synth.uniform(n + 3 * d, (1, ld), 0.0, 2.0))
        buf = np.ascontiguousarray(buf, dtype=np.float32)
        x = buf[:, :d].astype(np.float64)
        _CACHE[key] = (buf, x.sum(axis=0), x.T @ x, np.abs(x).T @ np.abs(x), np.abs(x).sum(axis=0))
    return _CACHE[key]


def _moments(dev, d, blocks, ld=None):
    """a fresh handle fed the given row blocks -> (sum, S2, n) on the host"""
    import torch
    from vsc_hip.pca_fit import HipPCAFit
    fit = HipPCAFit(d)
    for b in blocks:
        t = torch.from_numpy(np.ascontiguousarray(b)).to(dev)
        fit.partial_fit(t[:, :d] if t.shape[1] != d else t)
    s, s2 = fit.moments()
    out = s.cpu().numpy(), s2.cpu().numpy(), fit.n_samples
    fit.close()
    return out


@pytest.mark.parametrize("n,d,ld", SHAPES)
def test_moments_match_float64_numpy(dev, n, d, ld):
    buf, s64, s264, absprod, abssum = _case(n, d, ld)
    s, s2, seen = _moments(dev, d, [buf])
    assert seen == n
    err2, err1 = np.abs(s2 - s264), np.abs(s - s64)
    print(f"{n} x {d} (ld {ld}): S2 error / bound {np.max(err2 / (2 * n * U * absprod)):.3f}, sum error / bound {np.max(err1 / (2 * n * U * abssum)):.3f}")
    assert np.all(err2 <= 2 * n * U * absprod)
    assert np.all(err1 <= 2 * n * U * abssum)
    assert np.array_equal(s2, s2.T)


def test_asymmetric_exact_integers(dev):
    """Small integers: every product and sum is exact, so a wrong C/D row map, a swapped operand or a row added twice shows as a
    whole-number error (the data is not symmetric in its columns)."""
    n, d = 37, 150
    x = (np.arange(n)[:, None] * 3 + np.arange(d)[None, :] ** 2 % 17 - 7).astype(np.float32)
    s, s2, seen = _moments(dev, d, [x])
    x64 = x.astype(np.float64)
    assert seen == n and np.array_equal(s, x64.sum(axis=0)) and np.array_equal(s2, x64.T @ x64)


def test_common_offset_covariance(dev):
    """mean = 10 standard deviations: the covariance from raw fp64 moments is held to the raw moments' bound, against the two-pass
    float64 covariance."""
    import torch
    from vsc_hip.pca_fit import HipPCAFit
    n, d = 4100, 160
    x = np.ascontiguousarray(synth.normalish(91, (n, d)) + 10.0, dtype=np.float32)
    mean64, cov64 = pca_contract.covariance(x)
    fit = HipPCAFit(d)
    fit.partial_fit(torch.from_numpy(x).to(dev))
    mean, cov = (t.cpu().numpy() for t in fit.covariance())
    x64 = np.abs(x.astype(np.float64))
    bound = 2 * n * U * (x64.T @ x64)
    err = np.abs(cov - cov64) * (n - 1)
    print(f"offset data: covariance error / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    assert np.all(np.abs(mean - mean64) * n <= 2 * n * U * x64.sum(axis=0))
    assert np.array_equal(cov, cov.T)
    fit.close()


def test_blocks_agree_with_one_call(dev):
    n, d, ld = 1031, 130, 130
    buf, s64, s264, absprod, abssum = _case(n, d, ld)
    cuts = np.cumsum([1, 5, 0, 130, 895])
    assert cuts[-1] == n
    one = _moments(dev, d, [buf])
    many = _moments(dev, d, np.split(buf, cuts[:-1]))
    assert one[2] == n and many[2] == n
    for s, s2, _ in (one, many):
        assert np.all(np.abs(s2 - s264) <= 2 * n * U * absprod) and np.all(np.abs(s - s64) <= 2 * n * U * abssum)
    assert np.all(np.abs(one[1] - many[1]) <= 2 * n * U * absprod)


def test_symmetric_and_repeatable(dev):
    import torch
    from vsc_hip.pca_fit import HipPCAFit
    n, d, ld = 20000, 256, 256
    buf = _case(n, d, ld)[0]
    a, b = _moments(dev, d, [buf]), _moments(dev, d, [buf])
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    assert np.array_equal(a[1], a[1].T)
    fit = HipPCAFit(d)
    fit.partial_fit(torch.from_numpy(buf).to(dev))
    cov = fit.covariance()[1].cpu().numpy()
    assert np.array_equal(cov.view(np.uint64), cov.T.copy().view(np.uint64))
    fit.close()


def test_refusals(dev):
    import ctypes
    import torch
    from vsc_hip import _lib
    from vsc_hip.pca_fit import HipPCAFit
    lib = _lib.require_device()
    for d in (15, 4097, 0):
        h = ctypes.c_void_p()
        assert lib.vsc_pca_fit_create(d, ctypes.byref(h)) != 0 and b"unsupported" in lib.vsc_last_error() and not h.value
    fit = HipPCAFit(16)
    x = torch.zeros((4, 16), device=dev)
    assert lib.vsc_pca_fit_update_f32(fit._h, _lib.ptr(x), 4, 8, None) != 0 and b"row stride" in lib.vsc_last_error()
    assert lib.vsc_pca_fit_update_f32(fit._h, _lib.ptr(x), -1, 16, None) != 0
    assert lib.vsc_pca_fit_update_f32(fit._h, None, 0, 16, None) == 0 and fit.n_samples == 0
    with pytest.raises(_lib.VscHipError, match="needs 2"):
        fit.covariance()
    fit.partial_fit(x[:1])
    with pytest.raises(_lib.VscHipError, match="needs 2"):
        fit.covariance()
    with pytest.raises(ValueError):
        fit.partial_fit(x[:, :8])
    fit.close()
    with pytest.raises(ValueError):
        HipPCAFit(8)


@pytest.mark.parametrize("n,d,k,ratio", [(4100, 160, 40, 0.97), (700, 96, 24, 0.96)])
def test_finalize_matches_the_contract(dev, n, d, k, ratio):
    import torch
    from vsc_hip.pca_fit import HipPCAFit
    x = pca_contract.spectrum_data(50 + d, n, d, ratio)
    want = pca_contract.fit(x, k)
    fit = HipPCAFit(d)
    fit.partial_fit(torch.from_numpy(x).to(dev))
    mean, cov = (t.cpu().numpy() for t in fit.covariance())
    from vsc_hip.pca_fit import components_from_covariance
    comps64, var64 = components_from_covariance(cov, k)
    got = fit.finalize(k)
    errs = (np.abs(comps64 - want.components_).max(), np.abs(var64 - want.explained_variance_).max(), np.abs(mean - want.mean_).max())
    print(f"{n} x {d} -> {k}: components {errs[0]:.2e}, variances {errs[1]:.2e}, mean {errs[2]:.2e}")
    assert max(errs) <= 1e-9
    assert got.components_.dtype == np.float32 and got.mean_.dtype == np.float32
    assert np.abs(got.components_ - want.components_).max() <= 1e-6 and np.abs(got.mean_ - want.mean_).max() <= 1e-6
    assert np.abs(got.explained_variance_ - want.explained_variance_).max() <= 1e-9
    assert got.n_components_ == k and got.n_samples_ == n and got.whiten is False
    with pytest.raises(ValueError):
        fit.finalize(d + 1)
    small = HipPCAFit(d)
    small.partial_fit(torch.from_numpy(x[:k]).to(dev))
    with pytest.raises(ValueError, match="more rows"):
        small.finalize(k)
    small.close()
    fit.close()


def test_entry_point_fits_on_the_device(dev, tmp_path, monkeypatch):
    """concat_pca_sn --fit_pca --pca_fit hip on the small per-model files of test_gpu_knn.py::test_concat_pca_sn_entry_point, with
    sklearn blocked: the .npz model equals the contract fitted on the numpy-normalised concatenation, the merged descriptors equal
    the contract's transform, and extract_query_feats's loader reads the file."""
    import concat_pca_sn as C
    from src.query_postprocess import HipPCA, load_pca_model
    from vsc.index import VideoFeature
    from vsc.storage import load_features, store_features
    monkeypatch.setitem(sys.modules, "sklearn", None)
    models, dims = ["m_a", "m_b"], [24, 40]
    vids = {"train_refs": ["R100001", "R100002", "R100003"], "test_refs": ["R200001", "R200002"]}
    raw = {}
    for mi, (m, d) in enumerate(zip(models, dims)):
        os.makedirs(tmp_path / m)
        for si, (name, ids) in enumerate(vids.items()):
            feats = [VideoFeature(video_id=v, timestamps=np.arange(6 + vi, dtype=np.float64),
                                  feature=synth.normalish(1000 * mi + 100 * si + vi, (6 + vi, d)) * (1 + vi)) for vi, v in enumerate(ids)]
            raw[(m, name)] = feats
            store_features(str(tmp_path / m / f"{name}.npz"), feats)
    model_path = str(tmp_path / "pca.npz")
    C.main(C.build_parser().parse_args(["--root", str(tmp_path), "--models"] + models + ["--pca_model", model_path, "--fit_pca", "--pca_fit", "hip",
                                                                                          "--dim", "16"]))
    normalize = lambda f: f / np.linalg.norm(f.astype(np.float64), axis=1, keepdims=True)
    cat = {name: [np.concatenate([normalize(raw[(m, name)][vi].feature) for m in models], axis=1) for vi in range(len(ids))] for name, ids in vids.items()}
    want = pca_contract.fit(np.concatenate(cat["train_refs"]), 16)
    fitted = load_pca_model(model_path)
    print(f"entry point: components {np.abs(fitted.components_ - want.components_).max():.2e}, mean {np.abs(fitted.mean_ - want.mean_).max():.2e}")
    assert np.abs(fitted.components_ - want.components_).max() <= 1e-5 and np.abs(fitted.mean_ - want.mean_).max() <= 1e-5
    assert np.abs(fitted.explained_variance_ - want.explained_variance_).max() <= 1e-5 and fitted.n_samples_ == 21
    for name, ids in vids.items():
        merged = {vf.video_id: vf for vf in load_features(str(tmp_path / f"{name}.npz"))}
        assert sorted(merged) == sorted(ids)
        for vi, v in enumerate(ids):
            np.testing.assert_allclose(merged[v].feature, pca_contract.transform(want, cat[name][vi]), rtol=1e-4, atol=2e-5)
        assert all(vf.feature.shape[1] == 16 for vf in load_features(str(tmp_path / f"{name}_sn.npz")))
    assert np.array_equal(HipPCA(fitted).components_, fitted.components_)
    # fitting in blocks of any size gives the same model within the moments' bound
    paths = [str(tmp_path / m / "train_refs.npz") for m in models]
    whole, parts = C.fit_pca_hip(paths, 16), C.fit_pca_hip(paths, 16, block_rows=7)
    assert np.abs(whole.components_ - parts.components_).max() <= 1e-6 and np.array_equal(whole.components_, fitted.components_)


def test_uap_with_the_pca_fitted_on_the_device(dev, tmp_path, capsys, monkeypatch):
    """The chain of test_gpu_uap_e2e.py (small fixture, fp16 operands) with the PCA FITTED by concat_pca_sn --fit_pca --pca_fit hip on the
    HIP path's own train-reference descriptors.  The yardstick is tests/golden/uap_e2e_exact_pca.json: the reference chain with the
    exact fit in sklearn's place (its randomized solver moves the reference's own uAP by 1.3e-3); the criterion is the
    project's 1e-3.  The same descriptors give the model file = the contract's fit to 1e-5, so a miss can be assigned to the operands
    or to the fit."""
    import json
    import torch
    import concat_pca_sn
    import extract_query_feats
    import extract_ref_feats
    import vsc.baseline.sscd_baseline as entry
    from src.query_postprocess import load_pca_model
    from test_gpu_uap_e2e import GOLDS, UAP_ATOL, _checkpoints, _data, _uap
    from tools import synth_videos
    from vsc.metrics import CandidatePair
    from vsc.storage import load_features
    precision = "fp16"
    g = np.load(GOLDS["small"])
    gold = json.load(open(os.path.join(os.path.dirname(GOLDS["small"]), "uap_e2e_exact_pca.json")))
    data = _data("small")
    root = str(tmp_path)
    zips, out = os.path.join(root, "jpg_zips"), os.path.join(root, "outputs")
    os.makedirs(out)
    for grp in ("refs", "norm", "queries"):
        synth_videos.write_zips(data[grp], zips)
    lists = {}
    for name, grp in (("test_refs", "refs"), ("train_refs", "norm"), ("test_query", "queries")):
        lists[name] = os.path.join(root, name + ".txt")
        with open(lists[name], "w") as f:
            f.write("\n".join(v for v, _ in data[grp]) + "\n")
    models = _checkpoints(g, root)
    model_path = os.path.join(root, "pca_model.npz")
    for key, arch, fmt, ckpt in models:
        os.makedirs(os.path.join(out, key))
        for split in ("train_refs", "test_refs"):
            extract_ref_feats.main(types.SimpleNamespace(save_file=os.path.join(out, key, split), zip_prefix=zips, input_file=lists[split],
                                                         checkpoint_path=ckpt, arch=arch, weights_format=fmt, batch_size=2, max_batch=None,
                                                         precision=precision))
    monkeypatch.setitem(sys.modules, "sklearn", None)
    concat_pca_sn.main(concat_pca_sn.build_parser().parse_args(["--root", out, "--models"] + [m[0] for m in models] +
                                                               ["--pca_model", model_path, "--fit_pca", "--pca_fit", "hip", "--dim", str(gold["pca_dim"])]))
    monkeypatch.undo()
    # the fit alone, on the descriptors the HIP path extracted
    per_model = [np.concatenate([v.feature for v in load_features(os.path.join(out, m[0], "train_refs.npz"))]).astype(np.float64) for m in models]
    train = np.concatenate([f / np.linalg.norm(f, axis=1, keepdims=True) for f in per_model], axis=1)
    want, fitted = pca_contract.fit(train, gold["pca_dim"]), load_pca_model(model_path)
    fit_err = (float(np.abs(fitted.components_ - want.components_).max()), float(np.abs(fitted.mean_ - want.mean_).max()))
    extract_query_feats.main(extract_query_feats.build_parser().parse_args(
        ["--split", "test", "--models"] + [f"{arch}:{fmt}:{ckpt}" for _, arch, fmt, ckpt in models] +
        ["--pca_model", model_path, "--zip_prefix", zips, "--input_file", lists["test_query"],
         "--norm_refs", os.path.join(out, "train_refs.npz"), "--output_dir", out, "--workers", "2", "--precision", precision]))
    gt_csv = os.path.join(root, "gt.csv")
    with open(gt_csv, "w") as f:
        f.write("query_id,ref_id,query_start,query_end,ref_start,ref_end\n" + "".join(f"{q},{r},1,3,1,3\n" for q, r in data["gt"]))
    capsys.readouterr()
    entry.main(entry.build_parser().parse_args(["--query_features", os.path.join(out, "test_query_sn.npz"), "--ref_features",
                                                os.path.join(out, "test_refs_sn.npz"), "--output_path", os.path.join(out, "eval"),
                                                "--ground_truth", gt_csv, "--overwrite"]))
    logged = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Candidate uAP:")]
    assert logged, "sscd_baseline did not print the candidate uAP"
    hip = [(c.query_id, c.ref_id, c.score) for c in CandidatePair.read_csv(os.path.join(out, "eval", "candidates.csv"))]
    uap_hip = _uap(hip, data["gt"]).ap
    assert abs(float(logged[-1].split(":")[1]) - uap_hip) < 5e-5

    top = 200
    ref = [(q, r) for q, r in gold["top_candidates"]]
    pos = {(q, r): i for i, (q, r, _) in enumerate(hip)}
    order = [pos[k] for k in ref[:top] if k in pos]
    inversions = sum(1 for i in range(len(order)) for j in range(i + 1, len(order)) if order[i] > order[j])
    gtset = set(data["gt"])
    ranks_hip = [i for i, (q, r, _) in enumerate(hip) if (q, r) in gtset]
    report = (f"[PCA fitted on the device, {precision} operands, small fixture] uAP hip {uap_hip:.6f} vs the reference chain with the exact fit "
              f"{gold['uap']:.6f} (|d| {abs(uap_hip - gold['uap']):.2e}); distance to the reference chain with sklearn's randomized fit "
              f"({gold['uap_sklearn']:.6f}): {abs(uap_hip - gold['uap_sklearn']):.2e}; top-{top}: {inversions} rank inversions of "
              f"{len(order) * (len(order) - 1) // 2} pairs, {top - len(order)} candidates not shared; ground-truth ranks moved: "
              f"{sum(a != b for a, b in zip(gold['gt_ranks'], ranks_hip))} of {len(gold['gt_ranks'])}; model file vs the contract on the same "
              f"descriptors: components {fit_err[0]:.2e}, mean {fit_err[1]:.2e}")
    print(report)
    rep_dir = os.environ.get("VSC_REPORT_DIR") or root          # where the caller keeps reports; the line is printed either way
    os.makedirs(rep_dir, exist_ok=True)
    with open(os.path.join(rep_dir, "uap_e2e_report_pca_fit_hip.txt"), "w") as f:
        f.write(report + "\n")
    assert max(fit_err) <= 1e-5, report
    assert len(hip) == gold["n_candidates"], report
    assert abs(uap_hip - gold["uap"]) <= UAP_ATOL, report
    torch.cuda.synchronize()
