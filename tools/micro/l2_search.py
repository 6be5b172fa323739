"""Exact L2 search on the device against the host form and the inner-product sweep it rides on ("Exact L2 search").

  python tools/micro/l2_search.py [--nq 4096 --nr 262144 --d 512 --k 100 --reps 5] [--out profiles/l2_search_bench.txt]

Whole calls (FlatIPBank.search, numpy in, numpy out) by wall clock around calls that end in a copy to the host; device-resident calls
(ops.knn_l2 / ops.knn_ip on tensors, the bank augmented beforehand) by device events.  The forms are interleaved, one warm-up round,
median of --reps.  Also: the share of rows per path, the direct path's pairs/s on a far-cluster call (every row uncertified), and
range_search at a radius of about 100 hits per query.  Needs an MI355X: there is no fallback.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "vsc22-submission_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def unit(seed, n, d):
    x = np.random.RandomState(seed).standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--nr", type=int, default=262144)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--far-nq", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from vsc.index import METRIC_L2, FlatIPBank
    from vsc_hip import _lib, ops
    _lib.require_device()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def interleaved(forms, timer):
        """forms: {name: callable}; one warm-up round, then --reps rounds in turn -> {name: (median, min, max)}"""
        times = {n: [] for n in forms}
        for rep in range(a.reps + 1):
            for name, fn in forms.items():
                ms, _ = timer(fn)
                if rep:
                    times[name].append(ms)
        return {n: (statistics.median(v), min(v), max(v)) for n, v in times.items()}

    q, r = unit(1, a.nq, a.d), unit(2, a.nr, a.d)
    say(f"# l2_search: {a.nq} x {a.nr}, d = {a.d}, k = {a.k}, unit vectors, median (min .. max) of {a.reps}, ms")
    host, hip = FlatIPBank(a.d, METRIC_L2), FlatIPBank(a.d, METRIC_L2, l2="hip")
    host.add(r)
    hip.add(r)
    res = interleaved({"FlatIPBank.search l2=host": lambda: host.search(q, a.k), "FlatIPBank.search l2=hip": lambda: hip.search(q, a.k)}, wall)
    for name, (med, lo, hi) in res.items():
        say(f"{name:34s} wall   {med:10.2f} ({lo:.2f} .. {hi:.2f})")
    Dh, Ih = host.search(q, a.k)
    D, I = hip.search(q, a.k)
    paths = ops.knn_l2_last_path()
    say(f"rows by path (first probe, wider probe, direct): {paths} of {a.nq}; ids equal to l2=host: {float((I == Ih).mean()):.6f} of the slots, "
        f"max |distance difference| {float(np.abs(D - Dh).max()):.3g}")

    qd, rd = torch.from_numpy(q).to(dev), torch.from_numpy(r).to(dev)
    aug, _, mx = ops.l2_augment(rd)
    res = interleaved({"ops.knn_l2 (bank augmented before)": lambda: ops.knn_l2(qd, rd, a.k, bank=(aug, mx)),
                       "ops.knn_l2 (bank augmented in call)": lambda: ops.knn_l2(qd, rd, a.k),
                       f"ops.knn_ip k = {a.k}": lambda: ops.knn_ip(qd, rd, a.k),
                       f"ops.knn_ip k = {min(max(a.k + 8, 2 * a.k), 1024)} (the probe's ranks)": lambda: ops.knn_ip(qd, rd, min(max(a.k + 8, 2 * a.k), 1024)),
                       "ops.l2_augment(bank)": lambda: ops.l2_augment(rd)}, events)
    for name, (med, lo, hi) in res.items():
        say(f"{name:34s} events {med:10.2f} ({lo:.2f} .. {hi:.2f})")

    radius = float(np.median(D[:, min(a.k, D.shape[1]) - 1]))
    res = interleaved({"FlatIPBank.range_search l2=host": lambda: host.range_search(q, radius),
                       "FlatIPBank.range_search l2=hip": lambda: hip.range_search(q, radius)}, wall)
    n_hits = len(hip.range_search(q, radius)[0])
    for name, (med, lo, hi) in res.items():
        say(f"{name:34s} wall   {med:10.2f} ({lo:.2f} .. {hi:.2f})   radius {radius:.6g}: {n_hits / a.nq:.1f} hits per query")

    # the direct path: a far cluster, where no row is certified
    rng = np.random.RandomState(5)
    centre = rng.standard_normal(16)
    centre *= 200.0 / np.linalg.norm(centre)
    fr = (centre + 1e-2 * rng.standard_normal((a.nr, 16))).astype(np.float32)
    fq = (centre + 1e-2 * rng.standard_normal((a.far_nq, 16))).astype(np.float32)
    fqd, frd = torch.from_numpy(fq).to(dev), torch.from_numpy(fr).to(dev)
    faug, _, fmx = ops.l2_augment(frd)
    res = interleaved({"far cluster d = 16, auto": lambda: ops.knn_l2(fqd, frd, 5, bank=(faug, fmx))}, events)
    auto_paths = ops.knn_l2_last_path()
    with _lib.option("VSC_L2_PATH", "direct"):
        res.update(interleaved({"far cluster d = 16, direct only": lambda: ops.knn_l2(fqd, frd, 5)}, events))
        res.update(interleaved({f"unit d = {a.d}, direct only, {a.far_nq} rows": lambda: ops.knn_l2(qd[:a.far_nq], rd, a.k)}, events))
    for name, (med, lo, hi) in res.items():
        say(f"{name:34s} events {med:10.2f} ({lo:.2f} .. {hi:.2f})   {a.far_nq * a.nr / med / 1e6:.2f} G pairs/s")
    say(f"far cluster rows by path (auto): {auto_paths} of {a.far_nq}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
