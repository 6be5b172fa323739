"""The cases of the tests of vsc_jpeg_decode_split_u8 (CPU contract, emulated kernels, GPU entry): files written at test time by
Pillow's encoder, as in jpeg_decode_cases.py -- the smallest frames at which each piece of the split can go wrong.  ``MARKER``
frames carry restart intervals (name -> (file, markers expected)), ``SUBSTREAM`` frames none (name -> file; cut at 64 raw bytes in
the tests).  Everything is computed once per process and must not be modified."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import jpeg_decode_cases as cases  # noqa: E402
from jpeg_decode_cases import encode, noise, picture  # noqa: E402
from vsc_hip import jpeg  # noqa: E402

ITEM_BYTES = (1, 300, 1 << 30)     # every interval an item; several intervals per item; one item
SUB_BYTES = 64


@functools.lru_cache(maxsize=None)
def marker():
    """name -> (bytes, number of RSTn in the scan)"""
    return {
        "24x40_420_every_mcu": (encode(picture(50, 24, 40), "420", restart_marker_blocks=1), 5),
        "40x56_420_interval_5": (encode(picture(51, 40, 56), "420", restart_marker_blocks=5), 2),
        "40x56_422_interval_5": (encode(picture(52, 40, 56), "422", restart_marker_blocks=5), 3),
        "40x56_444_q90_interval_3": (encode(picture(53, 40, 56), "444", 90, restart_marker_blocks=3), 11),
        "40x56_gray_interval_2": (encode(picture(54, 40, 56, gray=True), restart_marker_blocks=2), 17),
        "16x16_interval_9": (encode(picture(55, 16, 16), "420", restart_marker_blocks=9), 0),
        "1x1_interval_1": (encode(picture(56, 1, 1), "420", restart_marker_blocks=1), 0),
        "noise_q100_every_mcu": (encode(noise(71, 33, 47), "420", 100, restart_marker_blocks=1), 8),
    }


@functools.lru_cache(maxsize=None)
def substream():
    """name -> bytes: frames without restart interval"""
    f = cases.files
    return {
        "37x53_420": f("37x53_420")[0], "37x53_422": f("37x53_422")[0], "37x53_444": f("37x53_444")[0], "37x53_gray": f("37x53_gray")[0],
        "noise_q75": f("noise_q75")[0], "checker_q100[0]": f("checker_q100")[0], "checker_q100[1]": f("checker_q100")[1],
        "37x53_optimize[0]": f("37x53_optimize")[0], "37x53_optimize[1]": f("37x53_optimize")[1],
        "shorter_than_a_substream": f("4x4_420")[0],
    }


def all_files():
    out = {k: v[0] for k, v in marker().items()}
    out.update(substream())
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """the frame as jpeg_decode_contract decodes it (which the CPU test holds against Pillow)"""
    import jpeg_decode_contract
    return jpeg_decode_contract.decode(all_files()[name])


@functools.lru_cache(maxsize=None)
def mixed():
    """one call: marker frames, sub-stream frames, a one-component frame and a 1 x 1 frame"""
    m, s = marker(), substream()
    return (m["40x56_420_interval_5"][0], s["37x53_444"], m["40x56_gray_interval_2"][0], s["37x53_gray"], m["1x1_interval_1"][0], cases.files("1x1_420")[0],
            s["checker_q100[0]"], m["noise_q100_every_mcu"][0], s["shorter_than_a_substream"])


@functools.lru_cache(maxsize=None)
def mixed_reference():
    import jpeg_decode_contract
    return tuple(jpeg_decode_contract.decode(f) for f in mixed())


def call(file_list, first_offset=0, gap=0, restarts=None):
    """jpeg_decode_cases.call plus the CSR of marker offsets (int64 ptr, int32 off); ``restarts``: {frame: offsets} overrides"""
    data, rows, tables, out_len, outs = cases.call(file_list, first_offset, gap)
    records = [jpeg.parse(f) for f in file_list]
    ptr, off = jpeg.restart_rows(file_list, records)
    if restarts:
        lists = [off[ptr[i]:ptr[i + 1]].tolist() for i in range(len(file_list))]
        for i, v in restarts.items():
            lists[i] = list(v)
        ptr = np.zeros(len(lists) + 1, np.int64)
        np.cumsum([len(v) for v in lists], out=ptr[1:])
        off = np.asarray([x for v in lists for x in v], np.int32)
    return data, rows, tables, out_len, outs, ptr, off
