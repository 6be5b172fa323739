#!/usr/bin/env python
"""Localisation throughput of the matching track: vsc_match_segments_f32 (one launch over every (map, threshold)) against the
host path (scipy components + sklearn RANSAC), in probability maps per second through all three thresholds.

    python tools/micro/match_segments_bench.py [--maps 512] [--size 224] [--host-maps 32] [--reps 5]

The device figure covers what infer_matching.run(localize="hip") does after the refinement networks: the maps are already on
the device, one launch, segments copied back and turned into rows.  The host figure is measured on the first --host-maps maps
(measured: 6.6 maps/s, 0.15 s per full-size map through the three thresholds) and includes no device -> host copy of the maps.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "vsc22-submission_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=512)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--host-maps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import seg_cases
    from src import matching
    maps = []
    for i in range(args.maps):
        rs = np.random.RandomState(7000 + i)
        case = dict(seed=7000 + i, h=args.size, w=args.size, noise=0.03, specks=12, thick=i % 3,
                    bands=seg_cases._bands(rs, args.size, args.size, 1 + i % 3, seg_cases.SLOPES))
        maps.append(seg_cases.matrix(case))
    rows = [[f"Q{i}", f"R{i}", m, None] for i, m in enumerate(maps)]
    dev = matching._to_device_maps(rows)
    matching.generate_matching_results_hip(dev, seg_cases.PASSES)             # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        hip = matching.generate_matching_results_hip(dev, seg_cases.PASSES)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    # the launch alone (events): what the kernel itself takes
    from vsc_hip import ops
    thr = np.array([p[0] for p in seg_cases.PASSES], np.float32)
    ratio = np.array([p[1] for p in seg_cases.PASSES], np.float64)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ops.match_segments_once(dev.flat, dev.items, thr, ratio, 8)
    e1.record()
    torch.cuda.synchronize()
    kernel_ms = e0.elapsed_time(e1)
    out = dict(maps=args.maps, size=args.size, thresholds=len(seg_cases.PASSES), hip_s=min(times), hip_s_all=times,
               hip_maps_per_s=args.maps / min(times), launch_ms=kernel_ms, segments=[len(r) for r in hip])
    if args.host_maps:
        sub = rows[:args.host_maps]
        t0 = time.perf_counter()
        host = [matching.generate_matching_result(sub, threshold=t, std_ratio=r) for t, r in seg_cases.PASSES]
        t_host = time.perf_counter() - t0
        out.update(host_maps=len(sub), host_s=t_host, host_maps_per_s=len(sub) / t_host, host_segments=[len(r) for r in host])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
