"""Times the matching-track segment AP (vsc.metrics.match_metric, csrc/segment_metric.hip) against the naive loop of the contract
(tests/segment_metric_contract.py: the reference's algorithm, its stand-in on the GPU box) at three workloads:

    predictions  pairs  per pair  ground truths
         50 000  5 000        10          5 000
         50 000    500       100          1 500
         30 000    100       300            600

  whole call   wall time of match_metric: packing, upload, the two kernels, the copy back and the host arithmetic (median of 5)
  kernels      vsc_segment_metric_deltas_f64 and the scan of the deltas, device events, after a warm-up (median of 5)
  naive        one run of the contract's naive match_metric on the same lists (one thread)

and checks that both give the same bits.  Writes profiles/segment_metric_bench.json.

    python tools/micro/segment_metric.py [--skip-naive]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "vsc22-submission_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import segment_metric_cases as cases  # noqa: E402
import segment_metric_contract as C  # noqa: E402
from vsc.metrics import Match, match_metric  # noqa: E402
from vsc_hip import segment_metric  # noqa: E402

WORKLOADS = [(5000, 10, 1), (500, 100, 3), (100, 300, 6)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-naive", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_metric_bench.json"))
    args = ap.parse_args()
    rows = []
    for n_pairs, per_pair, n_gt in WORKLOADS:
        gts, preds = cases.workload(n_pairs, n_pairs, per_pair, n_gt)
        G = [Match(q, r, 1.0, *b) for q, r, *b in gts]
        P = [Match(q, r, s, *b) for q, r, s, *b in preds]
        match_metric(G, P)                                           # warm-up
        whole = []
        for _ in range(5):
            t = time.perf_counter()
            got = match_metric(G, P)
            whole.append(time.perf_counter() - t)
        t = time.perf_counter()
        k = segment_metric.pack(G, P)
        pack_s = time.perf_counter() - t
        ops = [torch.from_numpy(a).cuda() for a in (k.pred_boxes, k.pred_ptr, k.pred_rank, k.gt_boxes, k.gt_ptr, k.group_ends)]
        delta_ms, scan_ms = [], []
        with segment_metric.HipSegmentMetric() as h:
            d, _ = h.deltas(*ops[:5])
            h.scan(d, ops[5])
            for _ in range(5):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record()
                d, _ = h.deltas(*ops[:5])
                e[1].record()
                h.scan(d, ops[5])
                e[2].record()
                e[2].synchronize()
                delta_ms.append(e[0].elapsed_time(e[1]))
                scan_ms.append(e[1].elapsed_time(e[2]))
        row = dict(predictions=len(P), pairs=n_pairs, per_pair=per_pair, ground_truths=len(G), tie_groups=int(len(k.group_ends)),
                   whole_call_s=statistics.median(whole), whole_call_runs_s=whole, pack_s=pack_s,
                   deltas_kernel_ms=statistics.median(delta_ms), scan_kernel_ms=statistics.median(scan_ms), ap=got.ap)
        if not args.skip_naive:
            t = time.perf_counter()
            want = C.match_metric(gts, preds)
            row["naive_s"] = time.perf_counter() - t
            row["naive_over_whole_call"] = row["naive_s"] / row["whole_call_s"]
            row["same_bits"] = bool(float(want[0]).hex() == float(got.ap).hex() and
                                    [float(v).hex() for v in want[2]] == [float(v).hex() for v in got.pr_curve.recalls])
        print(json.dumps(row), flush=True)
        rows.append(row)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), workloads=rows), f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
