"""TN alignment throughput (vsc_tn_align_f32): pairs per second for 512-pair batches at the shapes of the reference's CPU
timings, and a split of the time between the kernel's phases.

    python tools/micro/tn_align.py [--launches 20]

Each matrix is noise in [-0.45, 0.05) with one planted diagonal of 0.45 +- 0.05, used with bias 0.5, tn_max_step 5 and
min_length 4 (sscd_baseline's score-normalised branch).  The kernel is one fused launch, so its phases are split by
difference: `step1/path0` (no regular edges, one round) is phase A (top-K) plus a trivial rest; `path0 - step1/path0` is
phases B + C (edges, ranks) plus one more round's worth of work; `(path10 - path0) / 10` is one path round (D).
One JSON line per shape."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "vsc22-submission_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vsc_hip import _lib, ops  # noqa: E402


def batch(q, r, n, seed):
    rs = np.random.RandomState(seed)
    m = rs.uniform(-0.45, 0.05, size=(n, q, r)).astype(np.float32)
    for p in range(n):
        ln = int(rs.randint(q // 3, q))
        q0, r0 = int(rs.randint(0, q - ln + 1)), int(rs.randint(0, max(1, r - ln)))
        i = np.arange(ln)
        m[p, q0 + i, np.minimum(r0 + i, r - 1)] = 0.45 + rs.uniform(-0.05, 0.05, size=ln).astype(np.float32)
    table = np.stack([np.arange(n, dtype=np.int64) * q * r, np.full(n, q), np.full(n, r)], axis=1).astype(np.int64)
    return m.reshape(-1), table


def timed(fn, launches):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches       # ms per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=512)
    args = ap.parse_args()
    _lib.require_device()
    dev = torch.device("cuda:0")
    for q, r in ((30, 60), (60, 180), (120, 600)):
        flat, table = batch(q, r, args.pairs, seed=q * 7 + r)
        flat = torch.from_numpy(flat).to(dev)
        run = lambda step, path: ops.tn_align(flat, table, 0.5, step, 5, path, 0.2, 4, 0.3)
        t_full = timed(lambda: run(5, 10), args.launches)
        t_one = timed(lambda: run(5, 0), args.launches)
        t_a = timed(lambda: run(1, 0), args.launches)
        counts = run(5, 10)[1].cpu().numpy()
        print(json.dumps(dict(shape=f"{q}x{r}", pairs=args.pairs, ms_per_launch=round(t_full, 3),
                              pairs_per_s=round(args.pairs / t_full * 1e3, 1), us_per_pair=round(t_full / args.pairs * 1e3, 2),
                              phase_ms=dict(topk_A=round(t_a, 3), edges_ranks_BC_plus_round=round(t_one - t_a, 3),
                                            per_round_D=round((t_full - t_one) / 10, 3)),
                              boxes_per_pair=round(float(counts.mean()), 2))), flush=True)


if __name__ == "__main__":
    main()
