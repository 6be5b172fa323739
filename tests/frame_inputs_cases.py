"""Case table of vsc_frame_inputs_u8, shared by tests/test_frame_inputs_cpu.py (contract == Pillow), tests/test_frame_inputs_emulated.py
(kernel source on the CPU == contract) and tests/test_gpu_frame_inputs.py (device == contract == Pillow).  A case is frames uint8
[n, h, w, 3] -- seeded random frames and, last, one saturating pattern (hard 0 / 255 stripes along rows and columns, one stripe
width per channel, so that both passes overshoot and clip on both sides) -- and target rows (y0, y1, x0, x1, out_h, out_w, top, left,
crop_h, crop_w).  References are computed once per process."""
import functools
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "vsc22-submission_amd"))

import frame_inputs_contract as C  # noqa: E402
from src.dataset import clip_target, clip_transform_u8, square_target, vit_transform_u8  # noqa: E402


def pattern(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([255 * (((x // s) % 2) == ((y // s) % 2)) for s in (1, 5, 11)], axis=-1).astype(np.uint8)


def frames(name, n, h, w):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    f = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    f[-1] = pattern(h, w)
    return f


def whole(h, w, out_h, out_w, top=0, left=0, crop_h=None, crop_w=None):
    return (0, h, 0, w, out_h, out_w, top, left, out_h if crop_h is None else crop_h, out_w if crop_w is None else crop_w)


# name -> (n, h, w, targets, {"worker": [...]} or None): "worker" names the loader function each target restates, if any
_TABLE = {}


def _add(name, n, h, w, targets, workers=None, gpu_only=False):
    _TABLE[name] = dict(n=n, h=h, w=w, targets=[tuple(int(v) for v in t) for t in targets], workers=workers, gpu_only=gpu_only)


for _h, _w in ((37, 53), (53, 37)):     # the CLIP window starts at column / row 5
    _add(f"{_h}x{_w}_sq17_sq24_clip24", 2, _h, _w, [square_target(_h, _w, 17), square_target(_h, _w, 24), clip_target(_h, _w, 24)],
         [("vit", 17), ("vit", 24), ("clip", 24)])
for _h, _w in ((9, 31), (31, 9)):       # an upscale to 82, window offset 29: a byte offset that is not dword-aligned
    _add(f"{_h}x{_w}_clip24", 2, _h, _w, [clip_target(_h, _w, 24)], [("clip", 24)])
_add("24x24_identity", 2, 24, 24, [square_target(24, 24, 24)], [("vit", 24)])
for _h, _w in ((23, 24), (8, 9), (24, 29)):     # half-even crop offsets 0, 2, 2
    _add(f"{_h}x{_w}_clip24", 2, _h, _w, [clip_target(_h, _w, 24)], [("clip", 24)])
for _h, _w in ((1, 5), (5, 1)):
    _add(f"{_h}x{_w}_clip3", 2, _h, _w, [clip_target(_h, _w, 3)], [("clip", 3)])
_add("1x1_to_4x4", 2, 1, 1, [whole(1, 1, 4, 4)])
_add("200x7_sq16", 2, 200, 7, [square_target(200, 7, 16)], [("vit", 16)])            # every tap set clamped, support wider than the image
_add("203x2_sq8_vertical_first", 2, 203, 2, [square_target(203, 2, 8)], [("vit", 8)])
_add("64x48_rect_window", 2, 64, 48, [whole(64, 48, 31, 29, 3, 2, 23, 19)])            # a prime row count against the band height
_add("20x150_to_12x99_two_tiles", 2, 20, 150, [whole(20, 150, 12, 99)])             # more than one tile of output columns; 297-byte rows
_add("20x150_window_of_12x140", 2, 20, 150, [whole(20, 150, 12, 140, 1, 3, 10, 131)])  # three tiles, the last of 3 columns
_add("37x53_boxes_17", 5, 37, 53, [(3, 30, 5, 40, 17, 17, 0, 0, 17, 17), (0, 37, 0, 53, 17, 17, 0, 0, 17, 17)])
_add("90x160_three_targets", 3, 90, 160, [square_target(90, 160, 32), square_target(90, 160, 48), clip_target(90, 160, 28)],
     [("vit", 32), ("vit", 48), ("clip", 28)])
# (vertical support 15 rows) x 4096 x 3 bytes = 180 KiB: no band of whole rows would fit the LDS (64 column tiles do); too many
# lanes for the emulation.  On the device the two-pass path is reached by the vertical-first case above.
_add("56x8_to_16x4096_two_pass", 2, 56, 8, [whole(56, 8, 16, 4096)], gpu_only=True)
# a downscale by 192: 769 taps, a tile's rows of the horizontal table alone are 64 x 771 x 4 bytes = 193 KiB: the two-pass path
_add("2x12288_to_2x64_two_pass", 2, 2, 12288, [whole(2, 12288, 2, 64)], gpu_only=True)
_add("360x640_256_384_clip224", 2, 360, 640, [square_target(360, 640, 256), square_target(360, 640, 384), clip_target(360, 640, 224)],
     [("vit", 256), ("vit", 384), ("clip", 224)], gpu_only=True)


def names(gpu=False):
    return [n for n, c in _TABLE.items() if gpu or not c["gpu_only"]]


@functools.lru_cache(maxsize=None)
def get(name):
    c = dict(_TABLE[name])
    c["frames"] = frames(name, c["n"], c["h"], c["w"])
    c["frames"].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def contract(name):
    c = get(name)
    out = C.frame_inputs(c["frames"], c["targets"])
    for o in out:
        o.setflags(write=False)
    return out


def pillow_target(frame, target):
    from PIL import Image
    y0, y1, x0, x1, out_h, out_w, top, left, crop_h, crop_w = target
    img = Image.fromarray(np.ascontiguousarray(frame[y0:y1, x0:x1])).resize((out_w, out_h), Image.BICUBIC)
    return np.asarray(img.crop((left, top, left + crop_w, top + crop_h)), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def pillow(name):
    c = get(name)
    return [np.stack([pillow_target(f, t) for f in c["frames"]]) for t in c["targets"]]


def worker(frame, kind, size):
    """what the loader workers compute for one decoded frame"""
    from PIL import Image
    fn = vit_transform_u8(size, size) if kind == "vit" else clip_transform_u8(size)
    return fn(Image.fromarray(np.ascontiguousarray(frame))).numpy()


@functools.lru_cache(maxsize=None)
def workers(name):
    c = get(name)
    if not c["workers"]:
        return None
    return [np.stack([worker(f, kind, size) for f in c["frames"]]) for kind, size in c["workers"]]
