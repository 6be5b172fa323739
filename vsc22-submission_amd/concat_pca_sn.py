"""Reference-side merge of the ensemble's descriptors (reference: infer/concat_pca_sn.py).

    python concat_pca_sn.py --root outputs --models swinv2_v115 swinv2_v107 swinv2_v106 vit_v68 \
        --pca_model ../checkpoints/pca_model.pkl [--fit_pca]

Per feature set (train_refs, test_refs): the per-model descriptors of every video are L2-normalised, concatenated and
mapped to 512-d by the PCA (concat_pca_sn.py:56-68) -> <root>/<set>.npz; then each set is score-normalised against the
other (:71-88) -> <root>/<set>_sn.npz.  Row normalisation and the PCA product run on the GPU (HipOps / HipPCA).
``--score_norm hip`` runs that normalisation on the device (vsc.baseline.score_normalization, device="hip"; the same files).
``--fit_pca`` fits the PCA on the train set first (:42-54).  ``--pca_fit sklearn`` (the default) does it with sklearn on the host
exactly as the reference does and pickles the object; ``--pca_fit hip`` accumulates the moments on the GPU block by block
(vsc_hip/pca_fit.py: fp64 covariance, exact eigendecomposition; no sklearn, no pickle) and writes an ``.npz`` model file.
Without ``--fit_pca`` the model file is loaded (``.npz`` or pickle, src.query_postprocess.load_pca_model)."""
from __future__ import annotations

import argparse
import os

import numpy as np

from src.query_postprocess import HipOps, HipPCA, load_pca_model, save_pca_model
from vsc.baseline.score_normalization import DEVICES as SCORE_NORMS, ScoreNormBank, ref_score_normalize
from vsc.index import VideoFeature
from vsc.storage import load_features, store_features

NK, BETA = 1, 1.2   # concat_pca_sn.py:70-71


def concat_models(per_model_features, ops=HipOps):
    """[{video_id: VideoFeature} per model] -> (video ids in the first model's order, [n_frames, sum dims] per video)."""
    vids = list(per_model_features[0].keys())
    return vids, [np.concatenate([ops.normalize(m[v].feature) for m in per_model_features], axis=1) for v in vids]


BLOCK_ROWS = 1 << 18   # frames per device round trip of merge_set (x 2048 floats of concatenated descriptors = 2 GiB)


def video_blocks(lens, limit):
    """[lo, hi) ranges of consecutive videos holding at most `limit` rows each (a longer video is a block of its own)."""
    lo = 0
    while lo < len(lens):
        hi, rows = lo, 0
        while hi < len(lens) and (hi == lo or rows + lens[hi] <= limit):
            rows += lens[hi]
            hi += 1
        yield lo, hi
        lo = hi


def merge_set(paths, pca_transform, ops=HipOps, block_rows: int = None):
    """Per video: normalise every model's rows, concatenate, PCA (concat_pca_sn.py:56-68).  The reference does this video by video on the
    host; video by video through the GPU it was one host -> device -> host round trip per video and model plus one for the PCA -- 200 k of
    them for the track's 40 k reference videos.  Row normalisation and the PCA product are row-wise, so the videos of a BLOCK go through
    them together (one round trip per model and block, one for the PCA) and are cut apart again: the same per-row arithmetic, the same
    bits (tests/test_gpu_knn.py::test_concat_pca_sn_entry_point compares the two forms)."""
    models = [{vf.video_id: vf for vf in load_features(p)} for p in paths]
    vids = list(models[0].keys())
    lens = [len(models[0][v].feature) for v in vids]
    out = []
    for lo, hi in video_blocks(lens, block_rows or BLOCK_ROWS):
        block = vids[lo:hi]
        cat = np.concatenate([ops.normalize(np.concatenate([m[v].feature for v in block])) for m in models], axis=1)
        reduced = np.asarray(pca_transform(cat))
        cuts = np.cumsum([lens[i] for i in range(lo, hi)])[:-1]
        out.extend(VideoFeature(video_id=v, feature=f, timestamps=models[0][v].timestamps) for v, f in zip(block, np.split(reduced, cuts)))
    return out


def fit_pca_hip(paths, dim, block_rows: int = None):
    """concat_pca_sn.py:42-54 on the HIP path: the training set goes through ``HipPCAFit.partial_fit`` in the video blocks of
    ``merge_set``; each model's rows are normalised on the device and accumulated as a column slab of the block, so the concatenation
    of the whole set never exists as one host array.  -> vsc_hip.pca_fit.FittedPCA"""
    import torch
    from vsc_hip import _lib, ops
    from vsc_hip.pca_fit import HipPCAFit
    _lib.require_device()
    models = [{vf.video_id: vf for vf in load_features(p)} for p in paths]
    vids = list(models[0].keys())
    lens = [len(models[0][v].feature) for v in vids]
    dims = [models[i][vids[0]].feature.shape[1] for i in range(len(models))] if vids else []
    if not vids or sum(lens) <= dim or sum(dims) < dim:
        raise ValueError(f"fitting {dim} components needs more than {dim} rows of at least {dim} features, not {sum(lens)} x {sum(dims)}")
    fit = HipPCAFit(sum(dims))
    for lo, hi in video_blocks(lens, block_rows or BLOCK_ROWS):
        cat = torch.empty((sum(lens[lo:hi]), sum(dims)), dtype=torch.float32, device="cuda")
        col = 0
        for m, d in zip(models, dims):
            rows = np.ascontiguousarray(np.concatenate([m[v].feature for v in vids[lo:hi]]), dtype=np.float32)
            cat[:, col:col + d] = ops.l2_normalize_(torch.from_numpy(rows).cuda())
            col += d
        fit.partial_fit(cat)
    fitted = fit.finalize(dim)
    fit.close()
    return fitted


def main(args):
    sets = ["train_refs", "test_refs"]
    path = lambda model, name: os.path.join(args.root, model, f"{name}.npz")
    pca_fit = getattr(args, "pca_fit", "sklearn")
    if args.fit_pca and pca_fit == "hip":
        if not str(args.pca_model).endswith(".npz"):
            raise SystemExit(f"--pca_fit hip writes its model with numpy: --pca_model must end in .npz, not {args.pca_model!r}")
        fitted = fit_pca_hip([path(m, sets[0]) for m in args.models], args.dim)
        save_pca_model(fitted, args.pca_model)
    elif args.fit_pca:
        from sklearn.decomposition import PCA
        models = [{vf.video_id: vf for vf in load_features(path(m, sets[0]))} for m in args.models]
        fitted = PCA(n_components=args.dim, random_state=2023).fit(np.concatenate(concat_models(models)[1]))
        save_pca_model(fitted, args.pca_model)
    else:
        fitted = load_pca_model(args.pca_model)
    pca = HipPCA(fitted)
    for name in sets:
        store_features(os.path.join(args.root, f"{name}.npz"), merge_set([path(m, name) for m in args.models], pca.transform))
    score_norm = getattr(args, "score_norm", "host")   # main() is also called with namespaces built by hand, from before --score_norm
    if score_norm == "hip":
        # each set is the other's normalisation set: uploaded once, as a handle that serves in both roles
        banks = {name: ScoreNormBank(load_features(os.path.join(args.root, f"{name}.npz"))) for name in sets}
    for name, other in ((sets[1], sets[0]), (sets[0], sets[1])):
        if score_norm == "hip":
            refs, norm = banks[name], banks[other]
        else:
            refs = load_features(os.path.join(args.root, f"{name}.npz"))
            norm = load_features(os.path.join(args.root, f"{other}.npz"))
        store_features(os.path.join(args.root, f"{name}_sn.npz"), ref_score_normalize(refs, norm, nk=NK, beta=BETA, device=score_norm))


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default="./outputs")
    ap.add_argument("--models", nargs="+", default=["swinv2_v115", "swinv2_v107", "swinv2_v106", "vit_v68"])
    ap.add_argument("--pca_model", default="../checkpoints/pca_model.pkl")
    ap.add_argument("--fit_pca", action="store_true")
    ap.add_argument("--pca_fit", choices=["sklearn", "hip"], default="sklearn",
                    help="with --fit_pca: sklearn on the host as the reference (pickle), or the moments on the GPU + exact eigendecomposition "
                         "(vsc_hip/pca_fit.py; --pca_model must end in .npz)")
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--score_norm", choices=SCORE_NORMS, default="host",
                    help="the score normalisation's arithmetic in numpy on the host, or on the device (hip: one upload per set, the "
                         "same <set>_sn.npz)")
    return ap


if __name__ == "__main__":
    main(build_parser().parse_args())
