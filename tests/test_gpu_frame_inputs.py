"""Model-input frame resizing on the device (csrc/frame_inputs.hip, ops.frame_inputs, ``--resize hip`` of both extraction entry
points): the entry through ctypes on every case of tests/frame_inputs_cases.py -- 56 x 8 -> 16 x 4096 (64 column tiles, a vertical
support that whole-row bands could not hold), the vertical-first shape (two-pass path) and 360 x 640 frames to the ensemble's sizes
included -- between 0xFF guard bands at dword-aligned and at odd
addresses, against the executable contract (tests/frame_inputs_contract.py) and against the loader workers' Pillow transforms, bit
for bit; the refusals; one repeat run at a workload shape; and both entry points with ``--resize hip`` against ``host``, byte for
byte."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import frame_inputs_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p


@pytest.fixture(scope="module")
def dev():
    from vsc_hip import _lib
    _lib.require_device()
    return torch.device("cuda:0")


def run_entry(frames, targets, dev, guard=512, fill=0xFF, handle="own", n=None):
    """one vsc_frame_inputs_u8 call on the null stream, every output in one arena between guard bands of `guard` bytes of 0xFF
    -> (rc, [host output per target], guards intact)"""
    from vsc_hip import _lib
    lib = _lib.load()
    frames = np.ascontiguousarray(frames, np.uint8)
    nf, h, w = frames.shape[:3]
    t = np.ascontiguousarray(np.asarray(targets, np.int32).reshape(-1, 10))
    sizes = [nf * max(int(r[8]), 0) * max(int(r[9]), 0) * 3 for r in t]
    arena = torch.full((sum(sizes) + guard * (len(t) + 1) + frames.size + guard,), 0xFF, dtype=torch.uint8, device=dev)
    at, spans = guard, []
    for s in sizes:
        spans.append((at, at + s))
        at += s + guard
    f_at = at                                                  # the frames follow, at the same kind of address
    arena[f_at:f_at + frames.size] = torch.from_numpy(frames.reshape(-1).copy()).to(dev)
    for a, b in spans:
        arena[a:b] = fill
    base = arena.data_ptr()
    ptrs = (P * max(len(t), 1))(*[base + a for a, _ in spans])
    hd = P()
    _lib.check(lib.vsc_frame_inputs_create(None, ctypes.byref(hd)))
    try:
        rc = lib.vsc_frame_inputs_u8(hd if handle == "own" else handle, P(base + f_at), nf if n is None else n, h, w, t.ctypes.data, len(t), ptrs)
    finally:
        lib.vsc_frame_inputs_destroy(hd)                        # host state only: what is enqueued does not refer to it
    torch.cuda.synchronize()
    host = arena.cpu().numpy()
    intact, lo = True, 0
    for a, b in spans:
        intact = intact and bool((host[lo:a] == 0xFF).all())
        lo = b
    intact = intact and bool((host[lo:f_at] == 0xFF).all()) and bool((host[f_at + frames.size:] == 0xFF).all())
    intact = intact and np.array_equal(host[f_at:f_at + frames.size], frames.reshape(-1))
    return rc, [host[a:b].reshape(nf, max(int(r[8]), 0), max(int(r[9]), 0), 3) for (a, b), r in zip(spans, t)], intact


@pytest.mark.parametrize("guard", [512, 509])
@pytest.mark.parametrize("name", cases.names(gpu=True))
def test_entry_equals_contract_and_pillow(dev, name, guard):
    from vsc_hip import _lib
    c = cases.get(name)
    rc, outs, intact = run_entry(c["frames"], c["targets"], dev, guard=guard)
    assert rc == 0, _lib.load().vsc_last_error()
    assert intact, "a guard band or the input was written"
    wk = cases.workers(name)
    for t, (got, want, pil) in enumerate(zip(outs, cases.contract(name), cases.pillow(name))):
        bad = int((got != want).sum())
        print(f"{name} target {t} {c['targets'][t]}: {got.size} bytes, {bad} differ from the contract")
        assert np.array_equal(got, want), (name, t, bad, np.argwhere(got != want)[:4].tolist())
        assert np.array_equal(got, pil), (name, t, "differs from Pillow")
        if wk is not None:
            assert np.array_equal(got, wk[t]), (name, t, "differs from the loader worker's transform")


def test_boxes_equal_resize_bicubic(dev):
    """5 frames of 37 x 53, the boxes (3, 30, 5, 40) and the whole frame to 17 x 17: vsc_resize_bicubic_u8's output"""
    from vsc_hip import ops
    c = cases.get("37x53_boxes_17")
    frames = torch.from_numpy(c["frames"].copy()).to(dev)
    want = ops.resize_bicubic(frames, [t[:4] for t in c["targets"]], 17).cpu().numpy().reshape(2, 5, 17, 17, 3)
    got = ops.frame_inputs(frames, c["targets"])
    for t in range(2):
        assert np.array_equal(got[t].cpu().numpy(), want[t]), t


def test_refusals_write_nothing(dev):
    c = cases.get("37x53_sq17_sq24_clip24")
    good = (0, 37, 0, 53, 17, 17, 0, 0, 17, 17)

    def refused(targets, **kw):
        rc, outs, intact = run_entry(c["frames"], targets, dev, fill=0x5A, **kw)
        assert rc != 0, targets
        assert intact and all((o == 0x5A).all() for o in outs), "a refused call wrote"

    refused([good], handle=None)
    refused([good], n=-1)
    for bad in ((0, 38, 0, 53) + good[4:], (0, 37, 5, 5) + good[4:], good[:4] + (4097, 17, 0, 0, 17, 17), good[:4] + (17, 0, 0, 0, 17, 0),
                good[:6] + (1, 0, 17, 17), good[:6] + (0, 0, 17, 18), good[:6] + (0, -1, 17, 17)):
        refused([bad])
        refused([good, bad])                       # a bad target after a good one: nothing launched
    from vsc_hip import _lib
    lib = _lib.load()
    out = torch.full((2 * 17 * 17 * 3,), 0x5A, dtype=torch.uint8, device=dev)
    frames = torch.from_numpy(c["frames"].copy()).to(dev)
    t = np.asarray([good], np.int32)
    hd = P()
    _lib.check(lib.vsc_frame_inputs_create(None, ctypes.byref(hd)))
    assert lib.vsc_frame_inputs_u8(hd, P(frames.data_ptr()), 2, 37, 53, t.ctypes.data, 1, (P * 1)(None)) != 0      # a null output
    assert lib.vsc_frame_inputs_u8(hd, P(frames.data_ptr()), 0, 37, 53, t.ctypes.data, 1, (P * 1)(out.data_ptr())) == 0
    assert lib.vsc_frame_inputs_u8(hd, P(frames.data_ptr()), 2, 37, 53, None, 0, None) == 0
    lib.vsc_frame_inputs_destroy(hd)
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())
    rc, outs, intact = run_entry(c["frames"], c["targets"], dev)     # and the entry still works
    assert rc == 0 and intact and all(np.array_equal(g, w) for g, w in zip(outs, cases.contract("37x53_sq17_sq24_clip24")))


def test_workload_shape_repeats_and_equals_pillow(dev):
    """40 frames of 720 x 1280 to {256, 384, CLIP 224} through ops.frame_inputs on a side stream, three runs: the same bits, and
    frames 0 and 39 are Pillow's"""
    from src.dataset import clip_target, square_target
    from vsc_hip import ops
    rng = np.random.default_rng(7)
    frames = rng.integers(0, 256, (40, 720, 1280, 3), dtype=np.uint8)
    frames[39] = cases.pattern(720, 1280)
    targets = [square_target(720, 1280, 256), square_target(720, 1280, 384), clip_target(720, 1280, 224)]
    fd = torch.from_numpy(frames).to(dev)
    side = torch.cuda.Stream()
    runs = []
    for _ in range(3):
        with torch.cuda.stream(side):
            outs = ops.frame_inputs(fd, targets)
        side.synchronize()
        runs.append([o.cpu().numpy() for o in outs])
    for r in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(r, runs[0])), "two runs differ"
    for i in (0, 39):
        for t, tg in enumerate(targets):
            assert np.array_equal(runs[0][t][i], cases.pillow_target(frames[i], tg)), (i, t)


# ---- the entry points -------------------------------------------------------------------------------------------------------------------
def _npz(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def assert_same_npz(a, b):
    """the same arrays under the same names: dtype, shape and every byte (an .npz member carries a time stamp, its array does not)"""
    a, b = _npz(a), _npz(b)
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def _tiny_videos(prefix, start):
    """videos of 48 x 64, 64 x 48 and 40 x 40 frames, and one whose frames have two sizes (resized by the worker in every mode)"""
    rng = np.random.default_rng(start)
    shapes = [[(48, 64)] * 5, [(64, 48)] * 4, [(40, 40)] * 3, [(48, 64), (40, 40), (48, 64)]]
    return {f"{prefix}{start + i:06d}": [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in video] for i, video in enumerate(shapes)}


def _setup(tmp_path, prefix):
    from test_gpu_uap_e2e import GOLD, _checkpoints, _pca_pickle
    from test_gpu_view_preprocess import _write_zips
    g = np.load(GOLD)
    root = str(tmp_path)
    videos = _tiny_videos(prefix, 400001)
    zips = os.path.join(root, "zips")
    _write_zips(zips, videos)
    ids = os.path.join(root, "ids.txt")
    with open(ids, "w") as f:
        f.write("\n".join(videos) + "\n")
    pca_path = os.path.join(root, "pca_model.pkl")
    _pca_pickle(g, pca_path)
    return root, zips, ids, _checkpoints(g, root), pca_path, videos


def test_extract_ref_feats_resize_hip_writes_the_same_file(tmp_path):
    import extract_ref_feats as E
    root, zips, ids, models, _, videos = _setup(tmp_path, "R")
    _, arch, fmt, ckpt = models[1]                    # the ViT preset: one backbone, two runs (each starts the loader's four workers)
    out = {}
    for mode in ("host", "hip"):
        out[mode] = os.path.join(root, f"{arch}_{mode}")
        E.main(E.build_parser().parse_args(["--save_file", out[mode], "--zip_prefix", zips, "--input_file", ids, "--checkpoint_path", ckpt,
                                            "--arch", arch, "--weights_format", fmt, "--batch_size", "2", "--resize", mode]))
    assert_same_npz(out["hip"] + ".npz", out["host"] + ".npz")
    assert len(_npz(out["hip"] + ".npz")["features"]) == sum(len(v) for v in videos.values())


def test_extract_query_feats_resize_hip_writes_the_same_files(tmp_path):
    """--resize hip against host, and --preprocess hip --resize hip against --preprocess hip: every per-model file and the final one"""
    import extract_query_feats as E
    root, zips, ids, models, pca_path, _ = _setup(tmp_path, "Q")
    spec = [f"{arch}:{fmt}:{ckpt}" for _, arch, fmt, ckpt in models]
    keys = [os.path.split(ckpt)[-1].split(".")[0] for _, _, _, ckpt in models]

    def run(name, *extra):
        out = os.path.join(root, name)
        E.main(E.build_parser().parse_args(["--split", "test", "--models"] + spec + ["--pca_model", pca_path, "--zip_prefix", zips, "--input_file", ids,
                                                                                      "--output_dir", out, "--workers", "0", *extra]))
        return out

    for host, hip in ((run("host"), run("hip", "--resize", "hip")),
                      (run("views_host", "--preprocess", "hip"), run("views_hip", "--preprocess", "hip", "--resize", "hip"))):
        for key in keys:
            assert_same_npz(os.path.join(hip, key, "test_query.npz"), os.path.join(host, key, "test_query.npz"))
        assert_same_npz(os.path.join(hip, "test_query_sn.npz"), os.path.join(host, "test_query_sn.npz"))


def test_run_query_videos_makes_the_scorer_input_on_the_device():
    """run_query_videos(resize="hip") with a scorer (the tiny CLIP tower and video-score head), with and without views: the raw frames
    alone give the encoders' and the scorer's inputs, and the results equal those of the Pillow-made inputs bit for bit"""
    from PIL import Image
    from src.dataset import CLIP_MEAN, CLIP_STD, clip_transform_u8, vit_transform_u8
    from src.image_preprocess import HipResize, HipViews
    from src.query_pipeline import RAW_KEY, VideoScorer, run_query_videos
    from tools import synth
    from vsc_hip.config import get_config
    from vsc_hip.encoder import HipEncoder
    from vsc_hip.video_score import VideoScoreHead
    from vsc_hip.vsm_config import get_vsm_config
    dev = torch.device("cuda", 0)
    cfg, ccfg = get_config("tiny"), get_config("tiny_clip")
    vcfg = get_vsm_config("tiny_vsm", feat_dim=ccfg.width)
    enc = [(HipEncoder(cfg, synth.encoder_weights(7, cfg), max_batch=8, l2_normalize=True), cfg.image_size)]
    clip = HipEncoder(ccfg, synth.encoder_weights(8, ccfg), max_batch=8, u8_mean=CLIP_MEAN, u8_std=CLIP_STD)
    scorer = VideoScorer(clip, VideoScoreHead(vcfg, synth.vsm_weights(9, vcfg)), dev)
    size, csize = cfg.image_size, ccfg.image_size
    rng = np.random.default_rng(3)
    raws = {"Q500001": rng.integers(0, 256, (6, 90, 160, 3), dtype=np.uint8), "Q500002": rng.integers(0, 256, (3, 100, 70, 3), dtype=np.uint8)}
    stamps = lambda n: np.stack([np.arange(n, dtype=np.float32), np.arange(n, dtype=np.float32) + 1.0], axis=1)     # noqa: E731
    vit, ct = vit_transform_u8(size, size), clip_transform_u8(csize)
    host = [(v, {size: torch.stack([vit(Image.fromarray(f)) for f in fr]), VideoScorer.KEY: torch.stack([ct(Image.fromarray(f)) for f in fr])},
             stamps(len(fr))) for v, fr in raws.items()]
    raw = [(v, {RAW_KEY: torch.from_numpy(fr)}, stamps(len(fr))) for v, fr in raws.items()]
    pca = lambda x: x[:, :32]     # noqa: E731
    for views in (None, HipViews(dev)):
        s_host, s_hip = {}, {}
        if views is None:
            want = run_query_videos(host, enc, pca, s_host, dev, scorer=scorer, score_threshold=0.0)
        else:       # the views of the host path come from its own upload; the scorer input is the workers'
            want = run_query_videos([(v, {RAW_KEY: r[RAW_KEY], VideoScorer.KEY: h[1][VideoScorer.KEY]}, st) for (v, r, st), h in zip(raw, host)],
                                    enc, pca, s_host, dev, scorer=scorer, score_threshold=0.0, views=views)
        got = run_query_videos(raw, enc, pca, s_hip, dev, scorer=scorer, score_threshold=0.0, views=views, resize=HipResize(dev, clip_size=csize))
        assert s_hip == s_host and len(s_hip) == 2
        for a, b in zip(got[0], want[0]):
            assert a.video_id == b.video_id and np.array_equal(a.feature, b.feature) and np.array_equal(a.timestamps, b.timestamps)
        for pa, pb in zip(got[1], want[1]):
            assert all(np.array_equal(x.feature, y.feature) for x, y in zip(pa, pb))
    with pytest.raises(ValueError):
        run_query_videos(raw, enc, pca, {}, dev, resize="gpu")
