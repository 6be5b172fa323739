"""Score normalisation, host path against device path (vsc.baseline.score_normalization, device="host" / "hip"), at track size:

  ref_score_normalize    1.2 M x 512 references against a 1.2 M-row normalisation set (concat_pca_sn.py, per set)
  query_score_normalize  250 k x 512 query frames, nk = 10, against the same set (infer_matching.py step 1)

Each whole call is timed by the host clock (the calls end in a device -> host copy): median of --runs after a warm-up, both paths in
one process on one box.  The three kernels are timed by device events; vsc_column_var_f32 is also reported per pass as
ns per row and GB/s (two passes over n x d x 4 bytes in one launch).  The results of the two paths are compared bit for bit.
Needs an MI355X; writes --out (profiles/score_norm_bench.json).

    python tools/micro/score_norm.py [--rows 1200000] [--query_rows 250000] [--dim 512] [--runs 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "vsc22-submission_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FRAMES_PER_VIDEO = 30


def video_set(prefix, rows, d, seed):
    """videos of 30 frames as load_features hands them out: consecutive views of one float32 array"""
    from vsc.index import VideoFeature
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((rows, d), dtype=np.float32)
    base *= rng.uniform(0.5, 1.5, d).astype(np.float32)
    stamps = np.arange(rows, dtype=np.float32)
    cuts = list(range(0, rows, FRAMES_PER_VIDEO)) + [rows]
    return [VideoFeature(video_id=f"{prefix}{i:07d}", timestamps=stamps[lo:hi], feature=base[lo:hi]) for i, (lo, hi) in enumerate(zip(cuts, cuts[1:]))]


def timed(fn, runs):
    fn()                                                     # warm-up: library, scratch, allocator
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def event_ms(fn, runs):
    fn()
    out = []
    for _ in range(runs):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        out.append(start.elapsed_time(end))
    return out


def same_bits(a, b):
    return len(a) == len(b) and all(x.feature.shape == y.feature.shape and x.feature.tobytes() == y.feature.tobytes() for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_200_000)
    ap.add_argument("--query_rows", type=int, default=250_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_norm_bench.json"))
    args = ap.parse_args()
    from vsc.baseline import score_normalization as sn
    from vsc_hip import _lib, ops
    _lib.require_device()
    d = args.dim
    refs, noise = video_set("R1", args.rows, d, 1), video_set("R2", args.rows, d, 2)
    queries = video_set("Q", args.query_rows, d, 3)
    scores = {q.video_id: 1.0 for q in queries}
    result = {"device": torch.cuda.get_device_name(0), "rows": args.rows, "query_rows": args.query_rows, "dim": d, "runs": args.runs,
              "frames_per_video": FRAMES_PER_VIDEO, "whole_calls": {}, "kernels": {}}

    def record(name, host_fn, hip_fn):
        keep = {}
        host_s = timed(lambda: keep.__setitem__("host", host_fn()), args.runs)
        hip_s = timed(lambda: keep.__setitem__("hip", hip_fn()), args.runs)
        entry = {"host_runs_s": host_s, "hip_runs_s": hip_s, "host_s": statistics.median(host_s), "hip_s": statistics.median(hip_s),
                 "same_bits": same_bits(keep["host"], keep["hip"])}
        entry["host_over_hip"] = entry["host_s"] / entry["hip_s"]
        result["whole_calls"][name] = entry
        print(name, json.dumps(entry), flush=True)

    record("ref_score_normalize", lambda: sn.ref_score_normalize(refs, noise, nk=1, beta=1.2),
           lambda: sn.ref_score_normalize(refs, noise, nk=1, beta=1.2, device="hip"))
    dim = sn.low_variance_dim(noise, device="hip")
    record("query_score_normalize_nk10", lambda: sn.query_score_normalize(queries, noise, scores, 0.001, dim, nk=10, beta=1.5),
           lambda: sn.query_score_normalize(queries, noise, scores, 0.001, dim, nk=10, beta=1.5, device="hip"))
    # the hip call, split: where its time goes
    t0 = time.perf_counter()
    x = torch.from_numpy(sn.host_rows(refs)).cuda()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    out = ops.score_norm_rows(x, dim, True, 1)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    host = out.cpu().numpy()
    t3 = time.perf_counter()
    result["hip_ref_call_parts_s"] = {"upload": t1 - t0, "rows_kernel": t2 - t1, "download": t3 - t2, "bytes_each_way": int(host.nbytes)}
    del host

    n = args.rows
    var_ms = event_ms(lambda: ops.column_var(x), args.runs)
    ms = statistics.median(var_ms)
    result["kernels"]["vsc_column_var_f32"] = {"n": n, "d": d, "ms_runs": var_ms, "ms": ms, "ns_per_row_per_pass": ms * 1e6 / (2 * n),
                                               "GB_per_s": 2 * n * d * 4 / (ms * 1e-3) / 1e9, "passes": 2}
    rows_ms = event_ms(lambda: ops.score_norm_rows(x, dim, True, 1, out=out), args.runs)
    ms = statistics.median(rows_ms)
    result["kernels"]["vsc_score_norm_rows_f32"] = {"n": n, "d": d, "ms_runs": rows_ms, "ms": ms, "GB_per_s": 2 * n * d * 4 / (ms * 1e-3) / 1e9}
    topk = torch.rand((args.query_rows, 10), dtype=torch.float32, device="cuda")
    bias_ms = event_ms(lambda: ops.score_norm_bias(topk, 10, 1.5), args.runs)
    result["kernels"]["vsc_score_norm_bias_f32"] = {"nq": args.query_rows, "nk": 10, "ms_runs": bias_ms, "ms": statistics.median(bias_ms)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result["kernels"]), flush=True)


if __name__ == "__main__":
    main()
