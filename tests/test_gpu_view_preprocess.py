"""Query view preprocessing on the MI355X: vsc_frame_var_u8 bit-identical to numpy, vsc_canny_count_u8 equal to the numpy
restatement (tests/canny_cpu.py), vsc_resize_bicubic_u8 bit-identical to PIL, detect_views equal to the reference's decisions
(tests/golden/view_preprocess.json), and extract_query_feats --preprocess hip end to end."""
import io
import json
import os
import pickle
import sys
from zipfile import ZipFile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import canny_cpu  # noqa: E402
import view_cases  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(HERE, "golden", "view_preprocess.json")


def _dev(a):
    import torch
    from vsc_hip import _lib
    _lib.require_device()
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cases():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (2, 1, 7), (5, 37, 53), (21, 13, 1), (300, 17, 29), (21, 720, 1280)])
def test_frame_var_is_bit_identical_to_numpy(n, h, w):
    from vsc_hip import ops
    frames = np.random.default_rng(n * 1000 + h).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    got = ops.frame_var(_dev(frames)).cpu().numpy()
    want = np.stack(frames).var(axis=0).sum(-1)
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_canny_count_equals_the_restatement():
    from vsc_hip import ops
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, (4, 64, 80, 3), dtype=np.uint8)
    smooth = np.clip(rng.normal(128, 60, (3, 48, 40, 3)), 0, 255).astype(np.uint8)
    smooth[:, 10:30, 12:25] = 250                       # strong rectangles on a noisy background: weak chains join them
    for frames, idx in ((noise, [0, 1, 2, 3]), (noise, [3, 3, 0]), (smooth, [2, 0, 1]), (noise[:, :1, :9], [0, 1]),
                        (noise[:, :2, :5], [1, 2]), (noise[:, :7, :1], [0, 3]), (noise[:, :1, :1], [2])):
        d = _dev(frames)
        got = ops.canny_count(d, idx).cpu().numpy()
        assert np.array_equal(got, canny_cpu.canny_count(frames, idx)), (frames.shape, idx)
        assert np.array_equal(got, ops.canny_count(d, idx).cpu().numpy())     # labels may differ between runs, counts do not
    assert not ops.canny_count(_dev(noise), []).cpu().numpy().any()


def _weighted_count(frames, idx):
    """canny_cpu.canny_count for index lists that repeat frames: each distinct frame's edges once, times its multiplicity"""
    out = np.zeros(frames.shape[1:3], np.uint16)
    for i, k in zip(*np.unique(np.asarray(idx), return_counts=True)):
        out += (canny_cpu.canny(frames[i]) > 0).astype(np.uint16) * np.uint16(k)
    return out


def test_canny_count_across_several_chunks():
    """more than 32 sampled frames (chunks of 32 + the rest), and 1080p frames, where the 2^25-pixel scratch budget gives chunks of
    16: later chunks' frame offsets, the per-chunk reuse of the scratch and the accumulation into the output"""
    from vsc_hip import ops
    rng = np.random.default_rng(11)
    small = rng.integers(0, 256, (40, 24, 30, 3), dtype=np.uint8)
    idx = list(range(40)) + [5, 5, 39, 0]
    got = ops.canny_count(_dev(small), idx).cpu().numpy()
    assert np.array_equal(got, _weighted_count(small, idx))
    blocks = np.kron(rng.integers(0, 256, (2, 68, 120, 3)), np.ones((1, 16, 16, 1), np.int64))[:, :1080]
    big = np.clip(blocks + rng.integers(-40, 41, blocks.shape), 0, 255).astype(np.uint8)
    idx = [0, 1] * 8 + [1, 0, 0]          # 19 samples: chunks of 16 and 3
    got = ops.canny_count(_dev(big), idx).cpu().numpy()
    assert np.array_equal(got, _weighted_count(big, idx))


def test_maps_and_views_match_the_fixture():
    from src.image_preprocess import canny_frames, detect_views
    from vsc_hip import ops
    for case in _cases():
        frames = view_cases.frames(case)
        d = _dev(frames)
        idx = canny_frames(len(frames))
        var, count = ops.view_maps(d, idx)
        assert view_cases.digest(var) == case["var_digest"], case["name"]
        assert view_cases.digest(count) == case["count_digest"], case["name"]
        changed, boxes = detect_views(d)
        assert (changed, [list(b) for b in boxes]) == (case["changed"], case["boxes"]), case["name"]


def _pil(frame, box, size):
    from PIL import Image
    y0, y1, x0, x1 = box
    return np.asarray(Image.fromarray(np.ascontiguousarray(frame[y0:y1, x0:x1])).resize((size, size), Image.BICUBIC))


def test_resize_is_bit_identical_to_pil():
    from vsc_hip import ops
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, (3, 301, 517, 3), dtype=np.uint8)
    frames[1] = np.clip(rng.normal(128, 80, (301, 517, 3)), 0, 255).astype(np.uint8)
    d = _dev(frames)
    boxes = [(0, 1, 0, 1), (5, 6, 10, 300), (0, 301, 200, 201), (100, 130, 40, 77), (7, 300, 3, 516), (0, 301, 0, 517),
             (250, 301, 400, 517), (13, 96, 1, 2), (0, 301, 300, 302), (0, 200, 50, 52)]   # 301 > 2 x 100 rows: vertical pass first
    for size in (256, 384, 17, 1):
        got = ops.resize_bicubic(d, boxes, size).cpu().numpy()
        assert got.shape == (len(boxes) * 3, size, size, 3)
        for b, box in enumerate(boxes):
            for i in range(3):
                assert np.array_equal(got[b * 3 + i], _pil(frames[i], box, size)), (box, size, i)


def test_resize_through_many_table_lengths():
    """more than a thousand distinct crop lengths in one process: every coefficient table stays valid while calls keep adding
    new ones (the tables are never freed)"""
    from vsc_hip import ops
    frames = np.random.default_rng(4).integers(0, 256, (1, 1200, 9, 3), dtype=np.uint8)
    d = _dev(frames)
    for length in range(1, 1101):
        got = ops.resize_bicubic(d, [(0, length, 0, 9), (length, 1200, 0, 9)], 5)
        if length % 157 == 1:
            got = got.cpu().numpy()
            assert np.array_equal(got[0], _pil(frames[0], (0, length, 0, 9), 5)), length
            assert np.array_equal(got[1], _pil(frames[0], (length, 1200, 0, 9), 5)), length


@pytest.mark.parametrize("size", [256, 384])
def test_whole_frame_resize_equals_vit_transform(size):
    from PIL import Image
    from src.dataset import vit_transform_u8
    from vsc_hip import ops
    frames = np.random.default_rng(size).integers(0, 256, (2, 360, 640, 3), dtype=np.uint8)
    got = ops.resize_bicubic(_dev(frames), [(0, 360, 0, 640)], size).cpu().numpy()
    t = vit_transform_u8(size, size)
    for i in range(2):
        assert np.array_equal(got[i], t(Image.fromarray(frames[i])).numpy())


def _write_zips(root, videos):
    from PIL import Image
    for vid, frames in videos.items():
        d = os.path.join(root, vid[-2:])
        os.makedirs(d, exist_ok=True)
        with ZipFile(os.path.join(d, f"{vid}.zip"), "w") as z:
            for i, f in enumerate(frames):
                buf = io.BytesIO()
                Image.fromarray(f).save(buf, format="PNG")      # lossless: the decoded frames are the recipe's frames
                z.writestr(f"{i:04d}.png", buf.getvalue())


def test_extract_query_feats_with_hip_views(tmp_path):
    """--preprocess hip: each model's features equal the --preprocess none code path fed the PIL-made views of the reference's
    boxes, and a plain video's rows equal the --preprocess none run's"""
    import torch
    import extract_query_feats as E
    from src.model_zoo import DEFAULT_PRECISION, load_encoder
    from src.query_pipeline import run_query_videos
    from src.query_postprocess import HipPCA
    from vsc.storage import load_features
    from test_gpu_uap_e2e import GOLD, _checkpoints, _pca_pickle
    g = np.load(GOLD)
    root = str(tmp_path)
    cases = {c["name"]: c for c in _cases()}
    names = {"Q300001": "letterbox", "Q300002": "stack2_vertical", "Q300003": "plain"}
    videos = {vid: view_cases.frames(cases[name]) for vid, name in names.items()}
    zips = os.path.join(root, "zips")
    _write_zips(zips, videos)
    ids = os.path.join(root, "ids.txt")
    with open(ids, "w") as f:
        f.write("\n".join(names) + "\n")
    models = _checkpoints(g, root)
    pca_path = os.path.join(root, "pca_model.pkl")
    _pca_pickle(g, pca_path)
    spec = [f"{arch}:{fmt}:{ckpt}" for _, arch, fmt, ckpt in models]
    outs = {}
    for mode in ("hip", "none"):
        outs[mode] = os.path.join(root, "out_" + mode)
        E.main(E.build_parser().parse_args(["--split", "test", "--models"] + spec + ["--pca_model", pca_path, "--zip_prefix", zips,
                                            "--input_file", ids, "--output_dir", outs[mode], "--workers", "0", "--preprocess", mode]))

    def rows(mode, key):
        return {f.video_id: f for f in load_features(os.path.join(outs[mode], key, "test_query.npz"))}

    keys = [os.path.split(ckpt)[-1].split(".")[0] for _, _, _, ckpt in models]
    # the none path fed the PIL-made views of the reference's boxes
    encoders = [load_encoder(arch, fmt, ckpt, None, precision=DEFAULT_PRECISION) for _, arch, fmt, ckpt in models]
    sizes = list(dict.fromkeys(s for _, s in encoders))
    items = []
    for vid, name in names.items():
        fr, boxes = videos[vid], cases[name]["boxes"]
        n = len(fr)
        stamps = np.stack([np.arange(n, dtype=np.float32), np.arange(n, dtype=np.float32) + 1.0], axis=1)
        made = {s: torch.from_numpy(np.stack([_pil(f, b, s) for b in boxes for f in fr])) for s in sizes}
        items.append((vid, made, np.tile(stamps, (len(boxes), 1))))
    with open(pca_path, "rb") as f:
        pca = HipPCA(pickle.load(f))
    _, per_model = run_query_videos(items, encoders, pca.transform, {}, torch.device("cuda", 0))
    for i, key in enumerate(keys):
        got = rows("hip", key)
        for vid, pm in zip(names, per_model):
            assert len(got[vid].feature) == len(cases[names[vid]]["boxes"]) * len(videos[vid])
            assert np.array_equal(got[vid].feature, pm[i].feature), (key, vid)
            assert np.array_equal(got[vid].timestamps, pm[i].timestamps), (key, vid)
        plain_none = rows("none", key)["Q300003"]
        assert np.array_equal(got["Q300003"].feature, plain_none.feature) and np.array_equal(got["Q300003"].timestamps, plain_none.timestamps)
    finals = {m: {f.video_id: f for f in load_features(os.path.join(outs[m], "test_query_sn.npz"))} for m in outs}
    assert np.array_equal(finals["hip"]["Q300003"].feature, finals["none"]["Q300003"].feature)
