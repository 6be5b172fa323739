"""DP and HV alignment call times (vsc_align_dp_f32 / vsc_align_hv_f32), with TN (vsc_tn_align_f32) on the same pair table for
scale.

    python tools/micro/vta_align_bench.py [--calls 12] [--warmup 3]

Two batches from tools/synth.py: 512 pairs of 60 x 200 and 64 pairs of 300 x 1000; every matrix is noise in [-0.45, 0.05) with
one planted diagonal of 0.45 +- 0.05, used with bias 0.5 (sscd_baseline's score-normalised branch).  Every call is timed on its
own by a pair of device events around it, after `--warmup` untimed calls; a line gives the median, the least and the largest of
`--calls` calls, so the spread is on the line.  A call includes the upload of its pair table (one stream synchronisation).
No host comparison: VCSL's numba code is not part of this project."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vsc22-submission_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools import synth  # noqa: E402
from vsc_hip import _lib, ops  # noqa: E402


def batch(q, r, n, seed):
    m = synth.uniform(seed, (n, q, r), -0.45, 0.05).astype(np.float32)
    jitter = synth.uniform(seed + 1, (n, q), -0.05, 0.05).astype(np.float32)
    rs = np.random.RandomState(seed)
    for p in range(n):
        ln = int(rs.randint(q // 3, q))
        q0, r0 = int(rs.randint(0, q - ln + 1)), int(rs.randint(0, max(1, r - ln)))
        i = np.arange(ln)
        m[p, q0 + i, np.minimum(r0 + i, r - 1)] = np.float32(0.45) + jitter[p, :ln]
    table = np.stack([np.arange(n, dtype=np.int64) * q * r, np.full(n, q), np.full(n, r)], axis=1).astype(np.int64)
    return m.reshape(-1), table


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert args.calls >= 10, "medians of at least 10 calls"
    _lib.require_device()
    dev = torch.device("cuda:0")
    print(f"# {torch.cuda.get_device_name(0)}; ms per call: median [least .. largest] of {args.calls} calls after {args.warmup} warm-up calls")
    for q, r, n in ((60, 200, 512), (300, 1000, 64)):
        flat, table = batch(q, r, n, seed=q * 7 + r)
        flat = torch.from_numpy(flat).to(dev)
        with ops.AlignHandle() as h:
            runs = [
                ("dp  (dp()'s thresholds: min_sim 1, ave_sim 1.3)", lambda: ops.dp_align(flat, table, 0.5, 3, 1.0, 1.3, 4, 10, handle=h)),
                ("dp  (DpVtaModel defaults: min_sim 0, ave_sim 0.3)", lambda: ops.dp_align(flat, table, 0.5, 3, 0.0, 0.3, 4, 10, handle=h)),
                ("hv  (HvVtaModel defaults: 100 peaks)", lambda: ops.hv_align(flat, table, 0.5, 0.0, 0.9, 100, handle=h)),
                ("tn  (sscd_baseline: step 5, top 5, 10 paths)", lambda: ops.tn_align(flat, table, 0.5, 5, 5, 10, 0.2, 4, 0.3)),
            ]
            for name, fn in runs:
                med, lo, hi = timed(fn, args.calls, args.warmup)
                counts = fn()[1].cpu().numpy()
                print(f"{n:4d} pairs of {q} x {r}  {name:52s} {med:9.3f} [{lo:9.3f} .. {hi:9.3f}]  {med / n * 1e3:9.2f} us/pair  "
                      f"{float(counts.mean()):6.2f} boxes/pair", flush=True)


if __name__ == "__main__":
    main()
