"""Generates tests/golden/uap_e2e_exact_pca.json: the reference chain of gen_uap_e2e_golden.py (`chain`) on the small fixture's stored
fp32 descriptors with ONE change -- the PCA is fitted exactly (tests/pca_contract.py: float64 covariance, eigh) instead of by sklearn's
default solver, which picks the randomized SVD for this shape (240 x 1024 -> 128) and is approximate.  The yardstick of
tests/test_gpu_pca_fit.py::test_uap_with_the_pca_fitted_on_the_device; recomputed by tests/test_pca_fit_cpu.py.  CPU only, reads
nothing outside the repository:

    python tests/golden/gen_uap_exact_pca_golden.py [--dry]
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "vsc22-submission_amd"), HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import pca_contract  # noqa: E402

OUT = os.path.join(HERE, "uap_e2e_exact_pca.json")
TOP = 200


class ContractPCA:
    """stands where `chain` constructs sklearn's PCA"""

    def __init__(self, n_components, random_state=None):
        self.n_components = n_components

    def fit(self, x):
        self.__dict__.update(vars(pca_contract.fit(x, self.n_components)))
        return self

    def transform(self, x):
        return pca_contract.transform(self, x)


def compute(exact=True):
    """-> dict of what the fixture records (exact=False: sklearn's own fit, for the recorded comparison)"""
    import sklearn.decomposition
    import gen_uap_e2e_golden as G
    from tools import synth_videos
    from vsc.metrics import CandidatePair, average_precision
    g = np.load(G.OUT)
    data = synth_videos.make(int(g["seed"]))
    assert data["fingerprint"] == str(g["fingerprint"])
    saved = sklearn.decomposition.PCA
    if exact:
        sklearn.decomposition.PCA = ContractPCA
    try:
        cands, _, kept, low_var_dim = G.chain(data, [g["desc_swin"], g["desc_vit"]])
    finally:
        sklearn.decomposition.PCA = saved
    ap = average_precision([CandidatePair(q, r, 1.0) for q, r in data["gt"]], [CandidatePair(q, r, float(s)) for q, r, s in cands])
    gtset = set(data["gt"])
    return {"pca_dim": G.PCA_DIM, "uap": float(ap.ap), "n_candidates": len(cands),
            "gt_ranks": [i for i, (q, r, _) in enumerate(cands) if (q, r) in gtset], "low_var_dim": int(low_var_dim),
            "kept_counts": [len(kept[q]) for q, _ in data["queries"]], "top_candidates": [[q, r] for q, r, _ in cands[:TOP]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dry", action="store_true", help="print the numbers, do not write the fixture")
    args = ap.parse_args()
    out, skl = compute(True), compute(False)
    out["uap_sklearn"] = skl["uap"]          # a recorded fact: the same chain with sklearn's default (randomized) fit = uap_e2e.npz's uAP
    out["sklearn_same_low_var_dim"] = skl["low_var_dim"] == out["low_var_dim"]
    out["sklearn_same_kept_counts"] = skl["kept_counts"] == out["kept_counts"]
    print(f"exact fit: uAP {out['uap']:.7f}, {out['n_candidates']} candidates, low-variance dimension {out['low_var_dim']}; "
          f"sklearn's fit: uAP {out['uap_sklearn']:.7f} (difference {out['uap'] - out['uap_sklearn']:+.2e})")
    if not args.dry:
        with open(OUT, "w") as f:
            json.dump(out, f, indent=0)
            f.write("\n")


if __name__ == "__main__":
    main()
