#!/usr/bin/env python
"""PCA fit: the device accumulation (vsc_pca_fit_update_f32), the host eigen-solve and sklearn's fit, on the same synthetic
block of descriptors (tools/synth.py), each timed on its own.

    python tools/pca_fit_bench.py [--rows 262144] [--dim 2048] [--components 512] [--reps 5] [--sklearn-rows 60000] [--out profiles/pca_fit_bench.json]

  device accumulation  one update of --rows x --dim fp32 rows already on the device, device events around the call, warm-up first
                       (the warm-up call also grows the handle's scratch), --reps repeats; the achieved fp64 rate counts the
                       multiply-adds of the UPPER TRIANGLE the contract needs (rows * dim * (dim + 1) / 2, two operations each) --
                       the 128-column tiles on the diagonal compute both halves, which is not counted
  host eigen-solve     numpy.linalg.eigh of the dim x dim float64 covariance + order + sign rule (vsc_hip.pca_fit), host clock
  sklearn              PCA(n_components, random_state=2023).fit on the first --sklearn-rows rows (float32, its default solver),
                       host clock, one run; 0 skips it
Needs a device; writes one JSON document and prints it as one line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vsc22-submission_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--components", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sklearn-rows", type=int, default=60000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from tools import synth
    from vsc_hip import _lib
    from vsc_hip.pca_fit import HipPCAFit, components_from_covariance
    _lib.require_device()
    n, d = args.rows, args.dim
    # descriptors as the fit sees them: a decaying spectrum, rows normalised
    x = np.empty((n, d), dtype=np.float32)
    for i, lo in enumerate(range(0, n, 32768)):          # (generated in slices: the generator works in float64)
        blk = synth.normalish(11 + i, (min(32768, n - lo), d)) * (0.998 ** np.arange(d))
        x[lo:lo + len(blk)] = blk / np.linalg.norm(blk, axis=1, keepdims=True)
    xd = torch.from_numpy(x).cuda()
    fit = HipPCAFit(d)
    fit.partial_fit(xd)                                  # warm-up: code objects, scratch
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(fit._lib.vsc_pca_fit_update_f32(fit._h, _lib.ptr(xd), n, d, _lib.current_stream()))
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    flop = 2.0 * n * d * (d + 1) / 2
    best = min(ms)
    out = dict(rows=n, dim=d, components=args.components, host_threads=os.environ.get("OMP_NUM_THREADS", ""), update_ms=ms, update_ms_best=best,
               update_ms_median=float(np.median(ms)), upper_triangle_flop=flop, fp64_tflops_best=flop / (best * 1e-3) / 1e12,
               fp64_tflops_median=flop / (float(np.median(ms)) * 1e-3) / 1e12, rows_per_s=n / (best * 1e-3), n_samples=fit.n_samples)
    t0 = time.perf_counter()
    cov = fit.covariance()[1].cpu().numpy()
    out["covariance_copy_s"] = time.perf_counter() - t0
    eig = []
    for _ in range(2):
        t0 = time.perf_counter()
        comps, var = components_from_covariance(cov, args.components)
        eig.append(time.perf_counter() - t0)
    out.update(eigh_s=eig, eigh_s_best=min(eig))
    # the accumulated covariance against float64 numpy on a column block (the whole product would take minutes on the host)
    cols = slice(0, 64)
    x64 = x[:, cols].astype(np.float64)
    c64 = x64 - x64.mean(axis=0)
    # the handle has seen the block reps + 1 times: the same second moments, only the divisor differs
    seen = fit.n_samples
    out["cov_check_max_abs"] = float(np.abs(cov[cols, cols] * (seen - 1) / seen - c64.T @ c64 / n).max())
    if args.sklearn_rows:
        from sklearn.decomposition import PCA
        m = min(args.sklearn_rows, n)
        t0 = time.perf_counter()
        p = PCA(n_components=args.components, random_state=2023).fit(x[:m])
        out.update(sklearn_rows=m, sklearn_fit_s=time.perf_counter() - t0, sklearn_solver=p._fit_svd_solver)
    fit.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
