"""Times the descriptor-track micro-AP (vsc.metrics.average_precision) with device="host" and device="hip" on the case of 200 000
predictions against 8 000 ground-truth pairs (tests/uap_cases.py, the size of a real candidates.csv):

  whole call   wall time of average_precision on the two lists of CandidatePair -- on the hip path: interning the ids, the upload,
               the two entries, the downloads and the host arithmetic (after a warm-up; median, minimum and maximum of the repeats)
  interning    the Python-side part of the hip call alone (vsc_hip.uap.intern_pairs + the score vector)
  entries      vsc_uap_rank_f64 and vsc_uap_curve_f64 alone on resident operands, stream events (median, minimum and maximum)

and checks that the hip path gives the contract's bits.  Writes profiles/uap_bench.txt.

    python tools/micro/uap_bench.py [--repeats 7]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "vsc22-submission_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import uap_cases as cases  # noqa: E402
import uap_contract as C  # noqa: E402
from vsc.metrics import CandidatePair, average_precision  # noqa: E402
from vsc_hip import _lib, uap  # noqa: E402


def spread(values, unit):
    return f"median {statistics.median(values):.3f} {unit}  (min {min(values):.3f}, max {max(values):.3f}, {len(values)} runs)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uap_bench.txt"))
    args = ap.parse_args()
    lib = _lib.require_device()
    case = cases.get(cases.BIG)
    gt, preds = cases.pairs(case, CandidatePair)
    n, g = len(preds), len(gt)
    lines = [f"tools/micro/uap_bench.py on {torch.cuda.get_device_name(0)}: {n} predictions, {g} ground-truth pairs"]
    results = {}
    for device in ("host", "hip"):
        results[device] = average_precision(gt, preds, device=device)                     # warm-up
        runs = []
        for _ in range(args.repeats):
            t = time.perf_counter()
            average_precision(gt, preds, device=device)
            runs.append((time.perf_counter() - t) * 1e3)
        lines.append(f"whole call, device={device:<5} {spread(runs, 'ms')}")
        results[device + "_ms"] = statistics.median(runs)
    runs = []
    for _ in range(args.repeats):
        t = time.perf_counter()
        pk, gk, key_bits = uap.intern_pairs(gt, preds)
        scores = np.fromiter((p.score for p in preds), np.float64, n)
        runs.append((time.perf_counter() - t) * 1e3)
    lines.append(f"interning (host part of hip) {spread(runs, 'ms')}")
    d_scores, d_pk, d_gk = (torch.from_numpy(a).cuda() for a in (scores, pk.view(np.int64), gk.view(np.int64)))
    perm = torch.empty(n, dtype=torch.int64, device="cuda")
    ranked = torch.empty(n, dtype=torch.float64, device="cuda")
    correct = torch.empty(n, dtype=torch.uint8, device="cuda")
    status, counts = torch.empty(4, dtype=torch.int64, device="cuda"), torch.empty(2, dtype=torch.int64, device="cuda")
    sums, curve = torch.empty(2, dtype=torch.float64, device="cuda"), torch.empty((3, n), dtype=torch.float64, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    handle = uap.HipUap(lib)
    rank_ms, curve_ms = [], []
    for i in range(args.repeats + 2):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        handle.rank(P(d_scores), P(d_pk), n, P(d_gk), g, key_bits, P(perm), P(ranked), P(correct), P(status))
        e[1].record()
        handle.curve(P(ranked), P(correct), n, g, P(sums), P(counts), P(curve))
        e[2].record()
        e[2].synchronize()
        if i >= 2:                                                                           # two warm-up rounds
            rank_ms.append(e[0].elapsed_time(e[1]))
            curve_ms.append(e[1].elapsed_time(e[2]))
    handle.close()
    lines.append(f"vsc_uap_rank_f64  (key_bits {key_bits}) {spread(rank_ms, 'ms')}")
    lines.append(f"vsc_uap_curve_f64              {spread(curve_ms, 'ms')}")
    want = C.curve(*C.rank(scores, pk, gk, key_bits)[1:3], g)
    same = bool(np.array_equal(C.bits(sums.cpu().numpy()), C.bits(want[0])) and np.array_equal(counts.cpu().numpy(), want[1]))
    hip, host = results["hip"], results["host"]
    lines.append(f"hip: ap {hip.ap!r} simple_ap {hip.simple_ap!r}; sums and counts equal the contract's bits: {same}")
    lines.append(f"host: ap {host.ap!r} simple_ap {host.simple_ap!r}; |ap difference| {abs(hip.ap - host.ap):.3e}")
    lines.append(f"whole call hip / host: {results['hip_ms'] / results['host_ms']:.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)
    assert same


if __name__ == "__main__":
    main()
