"""CandidateGeneration.query at a synthetic scale of the descriptor track's eval step (sscd_baseline.search: global_k = 1200 per query
video): [n_q_videos] x 20 frames against [n_r_videos] x 25 frames of 512-d descriptors.   (run on the GPU box)
    python tools/micro/candidates_bench.py [n_q_videos] [n_r_videos] [--selection host|hip]
--selection: where the global top-k is cut and grouped (CandidateGeneration(selection=)); the probe sweep is timed on its own
(device events around a second, identical FlatIPBank.search_device call) so that the line shows its share of the query."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "vsc22-submission_amd")); sys.path.insert(0, ROOT)
import numpy as np, torch
from tools import synth
from vsc.candidates import CandidateGeneration, MaxScoreAggregation
from vsc.index import VideoFeature
argv = list(sys.argv[1:])
selection = "host"
if "--selection" in argv:
    at = argv.index("--selection")
    selection = argv[at + 1]
    del argv[at:at + 2]
nqv = int(argv[0]) if len(argv) > 0 else 2000
nrv = int(argv[1]) if len(argv) > 1 else 10000
rng = np.random.default_rng(0)


def vids(prefix, n, frames, seed):
    x = rng.standard_normal((n * frames, 512), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return [VideoFeature(video_id=f"{prefix}{i:06d}", feature=x[i * frames:(i + 1) * frames], timestamps=np.arange(frames, dtype=np.float32)) for i in range(n)]


refs, queries = vids("R", nrv, 25, 1), vids("Q", nqv, 20, 2)
for i in range(0, nqv, 10):      # every tenth query video holds copies of reference frames: true matches far above the noise
    queries[i].feature[:5] = refs[(7 * i) % nrv].feature[:5]
t0 = time.perf_counter()
cg = CandidateGeneration(refs, MaxScoreAggregation(), selection=selection)
cg.index.index.device_bank()                                        # the bank upload belongs to the index, not to the query
torch.cuda.synchronize()
t1 = time.perf_counter()
cands = cg.query(queries, global_k=1200 * nqv, limit=25 * nqv)      # what sscd_baseline.search asks for
torch.cuda.synchronize()
t2 = time.perf_counter()
# the stages again, each on its own between device events: the probe (VideoIndex's own k' rule) and, for `hip`, the two selection
# entries on that probe -- which of them the query's time outside the sweep belongs to
from vsc.index import probe_size
from vsc_hip import ops
feats = np.concatenate([q.feature for q in queries])
bank = cg.index.index
want = min(1200 * nqv, len(feats) * bank.ntotal)
kk = probe_size(1200 * nqv, len(feats), bank.ntotal)
q_dev = bank._device_queries(feats)


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return out, ev[0].elapsed_time(ev[1]) / 1000.0


(D, I), sweep = timed(lambda: ops.knn_ip(q_dev, bank.device_bank(), kk))
stages = ""
if selection == "hip":
    (rows, ids, _), t_sel = timed(lambda: ops.global_topk(D, I, want))
    q_video = torch.from_numpy(np.repeat(np.arange(nqv, dtype=np.int32), 20)).cuda()
    r_video = torch.from_numpy(np.repeat(np.arange(nrv, dtype=np.int32), 25)).cuda()
    _, t_grp = timed(lambda: ops.pair_first_hits(rows, ids, q_video, r_video, nrv, 25 * nqv))
    stages = f", global_topk of {D.numel()} entries {1e3 * t_sel:.2f} ms, pair_first_hits of {rows.numel()} hits {1e3 * t_grp:.2f} ms"
print(f"selection {selection}: {nqv} x 20 query frames, {nrv} x 25 reference frames, global_k {1200 * nqv}, probe k' {kk}: index {t1 - t0:.2f} s, "
      f"query {t2 - t1:.3f} s of which sweep {sweep:.3f} s ({100 * sweep / (t2 - t1):.0f} %){stages} -> {len(cands)} candidate pairs, best {cands[0].score:.4f}")
