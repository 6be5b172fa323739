#!/usr/bin/env python
"""Steps 3 and 4 of the matching track with the candidate maps on the host (the default) and on the device (--maps hip), on
identical synthetic inputs: feature building + classification, and feature building + refinement.

    python tools/micro/match_maps_bench.py [--candidates 4096] [--refine-candidates 4096] [--reps 3] [--out profiles/match_maps_bench.json]

4 096 candidates (64 query videos x 64 reference videos), a third of the queries with three views, video lengths 20 .. 400,
random-weight networks (tests/cnn_synth.py; the time of a convolution does not depend on its weights).  Every figure is a host
clock around work that ends in a device synchronise, after a warm-up of both paths; the two paths alternate.  `network_s` is
the networks alone on canvases that are already on the device (what either path cannot go below); `kernels` are
vsc_match_maps_f32 calls alone, from device events, with the bytes they write.  Needs a GPU; prints and writes one JSON object."""
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


def _unit_rows(rs, n, d):
    x = rs.randn(n, d).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def synthetic(candidates, d, seed=9):
    rs = np.random.RandomState(seed)
    nq = int(round(candidates ** 0.5))
    nr = (candidates + nq - 1) // nq
    query, ref, len_map = {}, {}, {}
    for k in range(nq):
        frames, views = int(rs.randint(20, 401)), 3 if k % 3 == 0 else 1
        query[f"Q{k:06d}"], len_map[f"Q{k:06d}"] = _unit_rows(rs, frames * views, d), frames
    for k in range(nr):
        ref[f"R{k:06d}"] = _unit_rows(rs, int(rs.randint(20, 401)), d)
    cands = [(q, r, np.float32(0.5)) for q in query for r in ref][:candidates]
    return query, ref, len_map, cands


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def kernel_ms(query, ref, len_map, cands, resolution, with_transpose, reps):
    """vsc_match_maps_f32 alone on the similarities of `cands` (already on the device): best of `reps`, device events."""
    import torch
    from src import matching
    from vsc_hip import ops
    shapes = [matching._map_shape(query, ref, c, len_map, resolution) for c in cands]
    banks = matching._Banks(query, ref, cands)
    pairs = banks.pairs.copy()
    pairs[:, 1], pairs[:, 3] = [s[0] for s in shapes], [s[1] for s in shapes]
    flat, off = ops.pair_similarity(torch.from_numpy(banks.q_bank).cuda(), torch.from_numpy(banks.r_bank).cuda(), pairs)
    items = np.stack([off[:-1], pairs[:, 1], pairs[:, 3], [s[2] for s in shapes]], axis=1)
    out = torch.empty((len(cands) * (2 if with_transpose else 1), resolution, resolution, 3), dtype=torch.float32, device="cuda")
    ops.match_maps(flat, items, resolution, with_transpose, out=out)
    best = float("inf")
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.match_maps(flat, items, resolution, with_transpose, out=out)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    multi = sum(s[0] * s[1] for s in shapes if s[0] > s[2])
    return dict(items=len(cands), resolution=resolution, with_transpose=int(with_transpose), ms=best, bytes_written=out.numel() * 4,
                bytes_read_view_choice=multi * 4, write_gb_per_s=out.numel() * 4 / best / 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=4096)
    ap.add_argument("--refine-candidates", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--refine-reps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_maps_bench.json"))
    args = ap.parse_args()
    import torch
    import cnn_synth
    from src import matching
    from vsc_hip import _lib, cnn
    _lib.require_device()
    cls_models, refine_models = matching.load_match_models([cnn_synth.mobilenetv3_small_state(40), cnn_synth.mobilenetv3_small_state(41)],
                                                           [cnn_synth.hrnet_refine_state(33), cnn_synth.hrnet_refine_state(34)], "cuda")
    query, ref, len_map, cands = synthetic(args.candidates, args.dim)
    refine_cands = cands[:: max(1, len(cands) // max(args.refine_candidates, 1))][:args.refine_candidates]

    def cls_host(c):
        feats, infos = matching.generate_candidates_classfiy_feature(query, ref, c, len_map)
        return matching.match_classify(cls_models, feats, [(q, r) for q, r, _ in infos])

    def cls_hip(c):
        return matching.classify_candidates_hip(cls_models, query, ref, c, len_map)

    def refine_host(c):
        return matching.match_refine(refine_models, matching.generate_matching_feature(query, ref, len_map, c), device_maps=True)

    def refine_hip(c):
        return matching.refine_candidates_hip(refine_models, query, ref, len_map, c, device_maps=True)

    warm = cands[:: max(1, len(cands) // 48)][:48]
    for fn in (cls_host, cls_hip, refine_host, refine_hip):
        fn(warm)
    out = dict(candidates=len(cands), refine_candidates=len(refine_cands), dim=args.dim, multi_view_share=1 / 3, lengths=[20, 400],
               step3=dict(host_s=[], hip_s=[]), step4=dict(host_s=[], hip_s=[]))
    for _ in range(args.reps):
        t, hip = timed(lambda: cls_hip(cands))
        out["step3"]["hip_s"].append(t)
        t, host = timed(lambda: cls_host(cands))
        out["step3"]["host_s"].append(t)
        assert hip == host, "the two paths disagree"
    for _ in range(args.refine_reps):
        t, hip = timed(lambda: refine_hip(refine_cands))
        out["step4"]["hip_s"].append(t)
        t, host = timed(lambda: refine_host(refine_cands))
        out["step4"]["host_s"].append(t)
        assert hip.ids == host.ids and torch.equal(hip.flat, host.flat), "the two paths disagree"
        del hip, host
    # the networks alone, on canvases that are already on the device
    group = cands[:matching.MATCH_CLS_BATCH // 2]
    feature, _ = matching._device_canvases(query, ref, group, len_map, matching.MATCH_CLS_RESOLUTION[0], True)
    cnn.match_classify_probability(cls_models, feature)
    t, _ = timed(lambda: [cnn.match_classify_probability(cls_models, feature) for _ in range(4)])
    out["step3"]["network_s"] = t / 4 * (2 * len(cands) / feature.shape[0])
    del feature
    feature, _ = matching._device_canvases(query, ref, refine_cands[:64], len_map, matching.MATCH_REFINE_RESOLUTION[0], False)
    t, _ = timed(lambda: [cnn.match_refine_probability(refine_models, feature[lo:lo + 16]) for lo in range(0, feature.shape[0], 16)])
    out["step4"]["network_s"] = t * len(refine_cands) / feature.shape[0]
    del feature
    for step in ("step3", "step4"):
        s = out[step]
        s["host_best_s"], s["hip_best_s"] = min(s["host_s"]), min(s["hip_s"])
        s["ratio"] = s["host_best_s"] / s["hip_best_s"]
        s["host_feeding_s"], s["hip_feeding_s"] = s["host_best_s"] - s["network_s"], s["hip_best_s"] - s["network_s"]
    out["kernels"] = [kernel_ms(query, ref, len_map, cands[:1024], 160, True, 5),
                      kernel_ms(query, ref, len_map, refine_cands[:1024], 224, False, 5)]
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
