"""vsc_frame_inputs_u8 without a GPU: the numpy contract (tests/frame_inputs_contract.py) equals Pillow's resize(...).crop(...) on
every case of tests/frame_inputs_cases.py and the loader workers' vit_transform_u8 / clip_transform_u8 where a target restates
one; clip_target / square_target give the workers' geometry; the entry points' --resize option parses and refuses."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "vsc22-submission_amd"))

import frame_inputs_cases as cases  # noqa: E402
import frame_inputs_contract as C  # noqa: E402
from src import dataset  # noqa: E402


@pytest.mark.parametrize("name", cases.names(gpu=True))
def test_contract_equals_pillow(name):
    want = cases.pillow(name)
    got = cases.contract(name)
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == np.uint8, (name, t)
        assert np.array_equal(g, w), (name, t, int((g != w).sum()))
    wk = cases.workers(name)
    if wk is not None:
        for t, (g, w) in enumerate(zip(got, wk)):
            assert np.array_equal(g, w), (name, t, "differs from the loader worker's transform")


def test_saturating_pattern_clips_on_both_sides():
    """the pattern frame does what it is there for: both passes of a downscale produce sums below 0 and above 255"""
    f = cases.get("37x53_sq17_sq24_clip24")["frames"][-1]

    def sums(img, inp, out):       # unclipped results of a pass along axis 0
        xmin, cnt, kk = C.coeffs(inp, out)
        return np.stack([(1 << 21) + np.tensordot(kk[o, :cnt[o]], img[xmin[o]:xmin[o] + cnt[o]].astype(np.int64), axes=(0, 0)) for o in range(out)]) >> 22
    acc = sums(f.transpose(1, 0, 2), 53, 17)
    assert acc.min() < 0 and acc.max() > 255
    mid = np.clip(acc, 0, 255).astype(np.uint8).transpose(1, 0, 2)
    acc = sums(mid, 37, 17)
    assert acc.min() < 0 and acc.max() > 255


def test_target_geometry_equals_the_worker_transforms():
    """for all h, w in 1..64 and sizes 3, 24, 32: the window of clip_target is the crop clip_transform_u8 takes of the image it
    resizes to, and square_target is vit_transform_u8's whole-frame resize"""
    from PIL import Image

    class Spy:
        """a stand-in image that records the resize and crop it is asked for"""
        def __init__(self, w, h, log):
            self.size, self.log = (w, h), log

        def convert(self, mode):
            return self

        def resize(self, size, resample):
            assert resample == Image.BICUBIC
            self.log.append(("resize", tuple(size)))
            return Spy(size[0], size[1], self.log)

        def crop(self, box):
            self.log.append(("crop", tuple(box)))
            return self

        def __array__(self, dtype=None, copy=None):
            return np.zeros((self.size[1], self.size[0], 3), np.uint8)

    for size in (3, 24, 32):
        clip, vit = dataset.clip_transform_u8(size), dataset.vit_transform_u8(size, size)
        for h in range(1, 65):
            for w in range(1, 65):
                log = []
                clip(Spy(w, h, log))
                (_, (nw, nh)), (_, (left, top, right, bottom)) = log
                assert dataset.clip_target(h, w, size) == (0, h, 0, w, nh, nw, top, left, bottom - top, right - left), (h, w, size)
                assert 0 <= top and top + size <= nh and 0 <= left and left + size <= nw, (h, w, size)
                log = []
                vit(Spy(w, h, log))
                assert log == [("resize", (size, size))]
                assert dataset.square_target(h, w, size) == (0, h, 0, w, size, size, 0, 0, size, size)


def test_clip_offsets_round_half_to_even():
    assert dataset.clip_target(23, 24, 24)[4:8] == (24, 25, 0, 0)      # difference 1 -> 0
    assert dataset.clip_target(8, 9, 24)[4:8] == (24, 27, 0, 2)        # 3 -> 2
    assert dataset.clip_target(24, 29, 24)[4:8] == (24, 29, 0, 2)      # 5 -> 2
    assert dataset.clip_target(9, 31, 24)[4:8] == (24, 82, 0, 29)
    assert dataset.clip_target(31, 9, 24)[4:8] == (82, 24, 29, 0)


def test_resize_option_values():
    assert dataset.RESIZES == ("host", "hip")
    assert dataset.check_resize("host") == "host" and dataset.check_resize("hip") == "hip"
    for bad in ("gpu", "", None, "HIP"):
        with pytest.raises(ValueError):
            dataset.check_resize(bad)


def test_entry_points_parse_and_refuse_resize():
    import argparse

    import extract_query_feats
    import extract_ref_feats
    for mod in (extract_ref_feats, extract_query_feats):
        ap = mod.build_parser()
        required = ["--checkpoint_path", "x"] if mod is extract_ref_feats else ["--models", "a:b:c", "--pca_model", "p", "--input_file", "i"]
        assert ap.parse_args(required).resize == "host"
        assert ap.parse_args(required + ["--resize", "hip"]).resize == "hip"
        with pytest.raises(SystemExit):
            ap.parse_args(required + ["--resize", "gpu"])
        assert mod.resize_of(argparse.Namespace()) == "host"            # a hand-built namespace from before the option
        assert mod.resize_of(argparse.Namespace(resize="hip")) == "hip"
        with pytest.raises(ValueError):
            mod.resize_of(argparse.Namespace(resize="gpu"))


def test_run_query_videos_refuses_resize_values():
    import torch
    from src.query_pipeline import run_query_videos
    with pytest.raises(ValueError):
        run_query_videos([], [], lambda x: x, {}, torch.device("cpu"), resize="gpu")
    with pytest.raises(ValueError):
        run_query_videos([], [], lambda x: x, {}, torch.device("cpu"), resize="hip")      # needs a GPU device
    assert run_query_videos([], [], lambda x: x, {}, torch.device("cpu"), resize="host") == ([], [])


def test_loaders_hand_over_decoded_frames(tmp_path):
    """--resize hip: the workers only decode -- raw uint8 frames at the zip's resolution and nothing else; a video whose frames
    differ in size is resized by Pillow in the worker, as with host"""
    import io
    from zipfile import ZipFile

    import extract_query_feats as E
    from PIL import Image
    from src.query_pipeline import RAW_KEY
    rng = np.random.default_rng(0)
    videos = {"Q100001": [rng.integers(0, 256, (40, 60, 3), dtype=np.uint8) for _ in range(3)],
              "Q100002": [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((40, 60), (30, 30))]}
    for vid, fr in videos.items():
        d = tmp_path / vid[-2:]
        d.mkdir(exist_ok=True)
        with ZipFile(d / f"{vid}.zip", "w") as z:
            for i, f in enumerate(fr):
                buf = io.BytesIO()
                Image.fromarray(f).save(buf, format="PNG")
                z.writestr(f"{i:04d}.png", buf.getvalue())
    items = list(E.zip_videos(list(videos), str(tmp_path), [16, 24], with_clip=True, workers=0, resize="hip"))
    assert set(items[0][1]) == {RAW_KEY} and np.array_equal(items[0][1][RAW_KEY].numpy(), np.stack(videos["Q100001"]))
    host = list(E.zip_videos(list(videos), str(tmp_path), [16, 24], with_clip=True, workers=0))
    assert set(items[1][1]) == set(host[1][1]) == {16, 24, "clip"}
    assert all(np.array_equal(items[1][1][k].numpy(), host[1][1][k].numpy()) for k in host[1][1])
    with pytest.raises(ValueError):
        E.zip_videos(list(videos), str(tmp_path), [16], resize="gpu")
    t = dataset.vit_transform_u8(16, 16)
    data = dataset.ZipFrames(list(videos), str(tmp_path), t, raw=True)
    batch = dataset.raw_collate([data[0], data[1]])
    assert batch[0][1] == "Q100001" and np.array_equal(batch[0][0].numpy(), np.stack(videos["Q100001"]))
    assert np.array_equal(batch[1][0].numpy(), dataset.ZipFrames(list(videos), str(tmp_path), t)[1][0].numpy()) and batch[1][0].shape == (2, 16, 16, 3)
