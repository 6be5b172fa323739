"""Times the query post-processing of one group of videos (src/query_postprocess.py: process_query_group) with the near-duplicate
frame filter on the host (``frame_filter="host"``: the similarity matrices are downloaded and filtered in numpy) and on the device
(``"hip"``: vsc_frame_filter_f32), in one process, on seeded descriptors that are already on the device:

  (a) 100 videos x 40 frames x 1 view       the regime tools/ensemble_bench.py times
  (b) 8 videos x 600 frames x 3 views       1 800 rows per video, about a third of them near-duplicates of other rows

Both paths are warmed up, then run alternately; a host clock around each call, which ends in its final device -> host copy; median,
minimum and maximum of the repeats.  The two results are asserted equal (final descriptors by bits, timestamps, per-model features).
The stage stands alone here: in run_query_videos it runs behind the next group's encoder launches.  Writes
profiles/frame_filter_bench.txt.

    python tools/micro/frame_filter_bench.py [--repeats 7]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "vsc22-submission_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from src import query_postprocess as Q  # noqa: E402
from vsc_hip import _lib  # noqa: E402

DIMS = (256, 256, 256, 256)       # four backbones
OUT_DIM = 512


def descriptors(rng, rows, dups):
    """[rows, sum(DIMS)] float32; `dups` rows are scaled copies of other rows plus 3 % of noise (cosine ~0.9995, not equal)"""
    d = sum(DIMS)
    x = rng.normal(size=(rows, d)).astype(np.float32)
    for dst, src in zip(rng.permutation(rows)[:dups], rng.integers(0, rows, dups)):
        if dst != src:
            noise = rng.normal(size=d).astype(np.float32)
            x[dst] = x[src] * np.float32(rng.uniform(0.5, 2.0)) + noise * np.float32(0.03 * np.linalg.norm(x[src]) / np.linalg.norm(noise))
    return x


def workload(seed, videos, frames, views, dup_share):
    rng = np.random.default_rng(seed)
    rows = frames * views
    full = [descriptors(rng, rows, int(rows * dup_share)) for _ in range(videos)]
    cuts = np.cumsum((0,) + DIMS)
    subs = [[torch.from_numpy(np.ascontiguousarray(x[:, lo:hi])).cuda() for x in full] for lo, hi in zip(cuts[:-1], cuts[1:])]
    return [f"Q{i:06d}" for i in range(videos)], subs, [np.arange(frames) for _ in range(videos)], [1.0] * videos


def same(a, b):
    ok = a[2] == b[2]
    for x, y in zip(a[0], b[0]):
        ok = ok and x.feature.shape == y.feature.shape and np.array_equal(x.feature.view(np.uint32), y.feature.view(np.uint32))
        ok = ok and np.array_equal(x.timestamps, y.timestamps)
    for px, py in zip(a[1], b[1]):
        ok = ok and all(np.array_equal(x.feature, y.feature) for x, y in zip(px, py))
    return bool(ok)


def spread(values):
    return f"median {statistics.median(values):8.2f} ms  (min {min(values):.2f}, max {max(values):.2f}, {len(values)} runs)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_filter_bench.txt"))
    args = ap.parse_args()
    assert args.repeats >= 5
    _lib.require_device()

    class Fitted:
        mean_ = np.linspace(-0.01, 0.01, sum(DIMS)).astype(np.float32)
        components_ = (np.random.default_rng(1).normal(size=(OUT_DIM, sum(DIMS))) / 8.0).astype(np.float32)
        whiten = False

    pca = Q.HipPCA(Fitted)
    lines = [f"tools/micro/frame_filter_bench.py on {torch.cuda.get_device_name(0)}: process_query_group, {len(DIMS)} models x {DIMS[0]} dims, "
             f"PCA to {OUT_DIM}"]
    for tag, shape in (("a", (100, 40, 1, 0.1)), ("b", (8, 600, 3, 1.0 / 3.0))):
        ids, subs, stamps, scores = workload(7, *shape)
        run = lambda ff: Q.process_query_group(ids, subs, stamps, scores, pca.transform, 0, frame_filter=ff)     # noqa: E731
        results = {ff: run(ff) for ff in Q.FRAME_FILTERS}                                   # warm-up of both
        equal = same(results["host"], results["hip"])
        times = {ff: [] for ff in Q.FRAME_FILTERS}
        for _ in range(args.repeats):
            for ff in Q.FRAME_FILTERS:                                                      # alternately
                torch.cuda.synchronize()
                t = time.perf_counter()
                out = run(ff)
                times[ff].append((time.perf_counter() - t) * 1e3)
                equal = equal and same(out, results["host"])
        rows = shape[1] * shape[2]
        kept = sum(len(f.feature) for f in results["hip"][0])
        lines.append(f"({tag}) {shape[0]} videos x {shape[1]} frames x {shape[2]} views (L = {rows}), kept {kept} of {shape[0] * rows} rows; "
                     f"hip equals host: {equal}")
        for ff in Q.FRAME_FILTERS:
            lines.append(f"({tag})   frame_filter={ff:<5} {spread(times[ff])}")
        lines.append(f"({tag})   hip / host: {statistics.median(times['hip']) / statistics.median(times['host']):.3f}")
        assert equal, f"workload ({tag}): the two paths differ"
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
