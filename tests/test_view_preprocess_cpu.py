"""Query view preprocessing on the CPU: the numpy Canny restatement on hand-derived cases, the host decisions of
src/image_preprocess.py against the reference's outcomes (tests/golden/view_preprocess.json), and the view-row bookkeeping of
run_query_videos / extract_query_feats with fake encoders and a fake detector."""
import io
import json
import os
import sys
from zipfile import ZipFile

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import canny_cpu  # noqa: E402
import view_cases  # noqa: E402
from src.image_preprocess import canny_frames, decide_views  # noqa: E402
from src.query_pipeline import RAW_KEY, run_query_videos  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "view_preprocess.json")


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def _gray(a):
    """a 2-D uint8 array as a 3-channel image with equal channels"""
    return np.repeat(np.asarray(a, np.uint8)[:, :, None], 3, axis=2)


# ---- the Canny restatement ---------------------------------------------------------------------------------------------------

def test_canny_vertical_step_keeps_the_left_column_of_equal_maxima():
    """dark | bright at columns 2 | 3: both columns have |dx| = 4 * 200 = 800 > 400; horizontal NMS keeps m > left && m >= right,
    so column 2 survives and column 3 (not > its left neighbour) does not"""
    img = np.zeros((7, 7), np.uint8)
    img[:, 3:] = 200
    mag, dx, dy = canny_cpu.gradient(_gray(img))
    assert (mag[:, 2] == 800).all() and (mag[:, 3] == 800).all() and (dy == 0).all()
    edges = canny_cpu.canny(_gray(img)) > 0
    want = np.zeros((7, 7), bool)
    want[:, 2] = True
    assert np.array_equal(edges, want)


def test_canny_horizontal_step_keeps_the_upper_row():
    img = np.zeros((7, 7), np.uint8)
    img[3:, :] = 200
    edges = canny_cpu.canny(_gray(img)) > 0
    want = np.zeros((7, 7), bool)
    want[2, :] = True
    assert np.array_equal(edges, want)


@pytest.mark.parametrize("anti", [False, True])
def test_canny_diagonal_steps(anti):
    """x + y >= 9 bright: dx = dy = 3v on the last dark and the first bright diagonal (m = 6v), s = +1, so NMS compares with the
    up-left / down-right pixels -- two diagonals away, m = 0 or 2v -- and keeps both: a two-pixel-wide edge.  x - y >= 1 bright:
    dx > 0 > dy, s = -1 (up-right / down-left), the same by symmetry."""
    n, v = 9, 200
    yy, xx = np.mgrid[0:n, 0:n]
    d = (xx - yy) if anti else (xx + yy)
    first = 1 if anti else n
    img = np.where(d >= first, v, 0)
    mag, dx, dy = canny_cpu.gradient(_gray(img))
    on = (d == first - 1) | (d == first)
    inner = (yy > 0) & (yy < n - 1) & (xx > 0) & (xx < n - 1)
    assert (mag[on & inner] == 6 * v).all() and (mag[(np.abs(d - first + 0.5) == 1.5) & inner] == 2 * v).all()
    assert ((dx[on & inner] ^ dy[on & inner]) < 0).all() == anti
    edges = canny_cpu.canny(_gray(img)) > 0
    assert np.array_equal(edges[inner], on[inner])


def test_canny_thresholds_are_strict():
    """m > floor(low) enters NMS; m > floor(high) is strong; a lone weak pixel is not an edge"""
    mag = np.zeros((3, 3), np.int32)
    dx = np.zeros((3, 3), np.int32)
    dy = np.zeros((3, 3), np.int32)
    for m, weak, strong in ((50, False, False), (51, True, False), (400, True, False), (401, False, True)):
        mag[1, 1], dx[1, 1] = m, m
        w, s = canny_cpu.nms(mag, dx, dy, 50, 400)
        assert (w[1, 1], s[1, 1]) == (weak, strong), m
        assert w.sum() + s.sum() == weak + strong
    w, s = canny_cpu.nms(mag, dx, dy, 50.9, 401.5)          # thresholds are floored: 401 > 401 is false
    assert w[1, 1] and not s[1, 1]


def test_canny_channel_tie_goes_to_the_lower_channel():
    """at (2, 2) channel 0 has a vertical edge (dx = 4v) and channel 1 a horizontal one (dy = 4v): equal |dx| + |dy|"""
    v = 100
    img = np.zeros((6, 6, 3), np.uint8)
    img[:, 3:, 0] = v
    img[3:, :, 1] = v
    mag, dx, dy = canny_cpu.gradient(img)
    assert (mag[2, 2], dx[2, 2], dy[2, 2]) == (4 * v, 4 * v, 0)
    mag, dx, dy = canny_cpu.gradient(img[:, :, [1, 0, 2]])
    assert (mag[2, 2], dx[2, 2], dy[2, 2]) == (4 * v, 0, 4 * v)


def test_canny_border_is_replicated():
    """a flat image has zero gradient everywhere, border included (zero padding would give 4 * value at the border); a 1-row image
    sees its own row above and below"""
    mag, _, _ = canny_cpu.gradient(np.full((5, 4, 3), 170, np.uint8))
    assert (mag == 0).all()
    row = np.array([[0, 0, 150, 150]], np.uint8)
    mag, dx, dy = canny_cpu.gradient(_gray(row))
    assert dx.tolist() == [[0, 600, 600, 0]] and (dy == 0).all()


def test_canny_hysteresis_joins_diagonally_and_drops_isolated_weak_chains():
    weak = np.zeros((6, 6), bool)
    strong = np.zeros((6, 6), bool)
    weak[0, 0] = weak[0, 1] = True        # joined to the strong pixel only through the diagonal (0, 1) - (1, 2)
    strong[1, 2] = True
    weak[4, 0:4] = True                   # no strong pixel in its component
    edges = canny_cpu.hysteresis(weak, strong)
    want = np.zeros((6, 6), bool)
    want[0, 0] = want[0, 1] = want[1, 2] = True
    assert np.array_equal(edges, want)


# ---- the reference's decisions -----------------------------------------------------------------------------------------------

def test_fixture_covers_the_cases():
    doc = _fixture()
    names = [c["name"] for c in doc["cases"]]
    assert names == [c["name"] for c in view_cases.cases()]
    assert sum(c["changed"] for c in doc["cases"]) >= 10 and sum(not c["changed"] for c in doc["cases"]) >= 4
    assert any(len(c["boxes"]) == 3 for c in doc["cases"]) and any(c["n"] > 20 for c in doc["cases"])


@pytest.mark.parametrize("name", [c["name"] for c in view_cases.cases()])
def test_maps_and_decisions_match_the_reference(name):
    case = next(c for c in _fixture()["cases"] if c["name"] == name)
    frames = view_cases.frames(case)
    assert view_cases.digest(frames) == case["frames_digest"]
    idx = canny_frames(len(frames))
    var = canny_cpu.frame_var(frames)
    assert view_cases.digest(var) == case["var_digest"]
    count = canny_cpu.canny_count(frames, idx)
    assert view_cases.digest(count) == case["count_digest"] and len(idx) == case["m"]
    changed, boxes = decide_views(var, count, len(idx), len(frames))
    assert changed == case["changed"]
    assert [list(b) for b in boxes] == case["boxes"]


def test_edge_line_cases_reach_the_multi_piece_line_cuts(monkeypatch):
    """the edge_lines_* cases split at sharp edge lines, not static bands: split_imgs' cut_h / cut_w return several pieces, and the
    fixture pins the reference's far-end-first order of the views (cut_w before cut_h when the frame is wider than tall)"""
    import src.image_preprocess as ip
    pieces = []
    real = ip._line_cuts
    monkeypatch.setattr(ip, "_line_cuts", lambda *a: pieces.append(real(*a)) or pieces[-1])
    for case in (c for c in _fixture()["cases"] if c["name"].startswith("edge_lines_")):
        pieces.clear()
        frames = view_cases.frames(case)
        idx = canny_frames(len(frames))
        changed, boxes = decide_views(canny_cpu.frame_var(frames), canny_cpu.canny_count(frames, idx), len(idx), len(frames))
        assert max(len(p) for p in pieces) == len(case["panels"]) >= 2, case["name"]
        assert changed and [list(b) for b in boxes] == case["boxes"]
        starts = [b[0] if case["size"][0] >= case["size"][1] else b[2] for b in case["boxes"]]
        assert starts == sorted(starts, reverse=True), case["name"]        # far end first


def test_canny_frames_follow_the_reference_sampling():
    for n in range(0, 3000):
        want = list(range(n)) if n <= 20 else [int(np.round(i)) for i in np.arange(0, n, n / 20)]
        assert canny_frames(n) == want


def test_fewer_than_five_frames_stay_whole():
    case = next(c for c in view_cases.cases() if c["name"] == "letterbox")
    frames = view_cases.frames(case)[:4]
    var, count = canny_cpu.frame_var(frames), canny_cpu.canny_count(frames, range(4))
    assert decide_views(var, count, 4, 4) == (False, [(0, 160, 0, 200)])


# ---- view rows through the pipeline ------------------------------------------------------------------------------------------

class _NumpyOps:
    @staticmethod
    def normalize(x):
        x = np.asarray(x, np.float32)
        return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)

    @staticmethod
    def self_similarity(x):
        return x @ x.T

    @staticmethod
    def similarity(a, b):
        return a @ b.T


class _FakeEncoder:
    """uint8 frames [S, s, s, 3] -> [S, dim]: per-frame channel means through a fixed projection (frame-independent)"""

    def __init__(self, dim, seed):
        self.proj = torch.from_numpy(np.random.default_rng(seed).standard_normal((3, dim)).astype(np.float32))

    def __call__(self, frames):
        return frames.float().mean(dim=(1, 2)) @ self.proj + frames.float()[:, 0, 0, :1]


def _crop_resize(frames, boxes, size):
    from PIL import Image
    return torch.from_numpy(np.stack([np.asarray(Image.fromarray(f[y0:y1, x0:x1]).resize((size, size), Image.BICUBIC))
                                      for y0, y1, x0, x1 in boxes for f in frames]))


class _FakeViews:
    """the HipViews interface on the CPU: fixed boxes per video (by frame height), PIL crop + resize"""

    def __init__(self, boxes_by_height):
        self.boxes_by_height, self.calls = boxes_by_height, []

    def __call__(self, raw, sizes):
        frames = raw.numpy()
        boxes = self.boxes_by_height[frames.shape[1]]
        self.calls.append((frames.shape, tuple(sizes)))
        return boxes, {s: _crop_resize(frames, boxes, s) for s in sizes}


def test_views_become_view_major_rows():
    rng = np.random.default_rng(3)
    raw_a = rng.integers(0, 256, (5, 40, 50, 3), dtype=np.uint8)       # two views
    raw_b = rng.integers(0, 256, (4, 30, 30, 3), dtype=np.uint8)       # one view, whole frame
    mixed = {8: torch.from_numpy(rng.integers(0, 256, (3, 8, 8, 3), dtype=np.uint8)),       # frames of different sizes: resized on the
             12: torch.from_numpy(rng.integers(0, 256, (3, 12, 12, 3), dtype=np.uint8))}    # host, not preprocessed
    stamps = lambda n: np.stack([np.arange(n, dtype=np.float32), np.arange(n, dtype=np.float32) + 1], axis=1)   # noqa: E731
    boxes = {40: [(0, 20, 0, 50), (20, 40, 5, 45)], 30: [(0, 30, 0, 30)]}
    videos = [("Q1", {RAW_KEY: torch.from_numpy(raw_a)}, stamps(5)), ("Q2", {RAW_KEY: torch.from_numpy(raw_b)}, stamps(4)),
              ("Q3", mixed, stamps(3))]
    enc = [(_FakeEncoder(6, 1), 8), (_FakeEncoder(4, 2), 12)]
    pca = lambda x: x[:, :5] * 2.0       # noqa: E731
    views = _FakeViews(boxes)
    finals, per_model = run_query_videos(videos, enc, pca, {}, torch.device("cpu"), ops=_NumpyOps, chunk=4, views=views)
    assert views.calls == [((5, 40, 50, 3), (8, 12)), ((4, 30, 30, 3), (8, 12))]

    # the same videos with the views made beforehand, through the plain path
    made = [("Q1", {s: _crop_resize(raw_a, boxes[40], s) for s in (8, 12)}, np.tile(stamps(5), (2, 1))),
            ("Q2", {s: _crop_resize(raw_b, boxes[30], s) for s in (8, 12)}, stamps(4)), ("Q3", mixed, stamps(3))]
    want_finals, want_pm = run_query_videos(made, enc, pca, {}, torch.device("cpu"), ops=_NumpyOps, chunk=4)
    assert [len(pm[0].feature) for pm in per_model] == [10, 4, 3]
    assert np.array_equal(per_model[0][0].timestamps, np.concatenate([stamps(5), stamps(5)]))      # view-major
    for got, want in zip(per_model, want_pm):
        for g, w in zip(got, want):
            assert np.array_equal(g.feature, w.feature) and np.array_equal(g.timestamps, w.timestamps)
    for g, w in zip(finals, want_finals):
        assert np.array_equal(g.feature, w.feature) and np.array_equal(g.timestamps, w.timestamps)
    # view 2 of Q1 really is the second crop: its rows equal encoding that crop alone
    alone = enc[0][0](_crop_resize(raw_a, boxes[40][1:], 8)).numpy()
    assert np.array_equal(per_model[0][0].feature[5:], _NumpyOps.normalize(alone))


def test_preprocess_defaults_to_none():
    import extract_query_feats as E
    args = E.build_parser().parse_args(["--models", "a:b:c", "--pca_model", "p", "--input_file", "i"])
    assert args.preprocess == "none"
    assert E.build_parser().parse_args(["--models", "a:b:c", "--pca_model", "p", "--input_file", "i", "--preprocess", "hip"]).preprocess == "hip"
    with pytest.raises(SystemExit):
        E.build_parser().parse_args(["--models", "a:b:c", "--pca_model", "p", "--input_file", "i", "--preprocess", "cv2"])


def test_query_videos_keep_full_resolution_frames_with_hip(tmp_path):
    """--preprocess hip: the zip's own resolution under RAW_KEY next to the CLIP frames; frames of different sizes are resized on the
    host as with none (the reference's np.stack fails on them and leaves the video unprocessed)"""
    from PIL import Image
    import extract_query_feats as E
    rng = np.random.default_rng(0)
    shapes = {"Q200001": [(40, 60)] * 3, "Q200002": [(40, 60), (30, 60)]}
    arrays = {}
    for vid, sz in shapes.items():
        d = tmp_path / vid[-2:]
        d.mkdir(exist_ok=True)
        arrays[vid] = [rng.integers(0, 255, s + (3,), dtype=np.uint8) for s in sz]
        with ZipFile(d / f"{vid}.zip", "w") as z:
            for i, a in enumerate(arrays[vid]):
                buf = io.BytesIO()
                Image.fromarray(a).save(buf, format="PNG")
                z.writestr(f"{i:04d}.png", buf.getvalue())
    items = {v[0]: v for v in E.zip_videos(list(shapes), str(tmp_path), [16, 24], with_clip=True, preprocess="hip")}
    _, frames, stamps = items["Q200001"]
    assert sorted(frames, key=str) == sorted([RAW_KEY, "clip"], key=str)
    assert np.array_equal(frames[RAW_KEY].numpy(), np.stack(arrays["Q200001"])) and frames["clip"].shape == (3, 224, 224, 3)
    assert stamps.tolist() == [[0, 1], [1, 2], [2, 3]]
    _, frames, _ = items["Q200002"]
    assert RAW_KEY not in frames and frames[16].shape == (2, 16, 16, 3) and frames[24].shape == (2, 24, 24, 3)
