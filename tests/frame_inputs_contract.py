"""Executable contract of vsc_frame_inputs_u8 (include/vsc_hip.h): the windowed two-pass 8-bit bicubic resample in numpy, restated
per axis from Pillow's algorithm -- coefficients in float64 per (in length, out length), normalised, rounded half away from zero
to 22 fractional bits; per pass the integer sum of taps from 1 << 21, shifted down and clipped to uint8; horizontal pass first
(vertical first for a box more than 100 times taller than wide that shrinks in height); only the rows and columns that the window
reads are computed.  tests/test_frame_inputs_cpu.py pins it against Pillow's resize(...).crop(...)."""
import functools
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2


def bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@functools.lru_cache(maxsize=None)
def coeffs(inp: int, out: int):
    """-> (first tap [out], tap count [out], weights int64 [out, ksize]) of a box (0, inp) -> out"""
    scale = inp / out
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    xmin, cnt, kk = np.zeros(out, np.int64), np.zeros(out, np.int64), np.zeros((out, ksize), np.int64)
    ss = 1.0 / filterscale
    for xx in range(out):
        center = 0.0 + (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), inp) - lo
        k = [bicubic((x + lo - center + 0.5) * ss) for x in range(hi)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        xmin[xx], cnt[xx] = lo, hi
        for x, v in enumerate(k):
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    return xmin, cnt, kk


def resample_rows(img, inp: int, out: int, first: int, count: int, origin: int = 0):
    """Output rows [first, first + count) of resampling a length-``inp`` row axis to ``out``; row 0 of ``img`` (uint8 [rows, cols,
    3]) is source row ``origin``.  (Columns: transpose before and after.)"""
    xmin, cnt, kk = coeffs(inp, out)
    src = img.astype(np.int64)
    res = np.empty((count,) + img.shape[1:], np.uint8)
    for j in range(count):
        o = first + j
        lo, c = int(xmin[o]) - origin, int(cnt[o])
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(kk[o, :c], src[lo:lo + c], axes=(0, 0))
        res[j] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return res


def resample_cols(img, inp, out, first, count, origin=0):
    return resample_rows(img.transpose(1, 0, 2), inp, out, first, count, origin).transpose(1, 0, 2)


def vertical_first(hc: int, wc: int, out_h: int) -> bool:
    return hc > wc * 100 and out_h < hc


def window(frame, target):
    """One frame uint8 [h, w, 3], one target row -> uint8 [crop_h, crop_w, 3]"""
    y0, y1, x0, x1, out_h, out_w, top, left, crop_h, crop_w = (int(v) for v in target)
    box = frame[y0:y1, x0:x1]
    hc, wc = box.shape[:2]
    if crop_h == 0 or crop_w == 0:
        return np.empty((crop_h, crop_w, 3), np.uint8)
    hx, hcnt, _ = coeffs(wc, out_w)
    vx, vcnt, _ = coeffs(hc, out_h)
    xlo, xhi = int(hx[left]), int(hx[left + crop_w - 1] + hcnt[left + crop_w - 1])     # box columns the window reads
    ylo, yhi = int(vx[top]), int(vx[top + crop_h - 1] + vcnt[top + crop_h - 1])         # box rows
    if vertical_first(hc, wc, out_h):
        mid = resample_rows(box[:, xlo:xhi], hc, out_h, top, crop_h)
        res = resample_cols(mid, wc, out_w, left, crop_w, origin=xlo)
    else:
        mid = resample_cols(box[ylo:yhi], wc, out_w, left, crop_w)
        res = resample_rows(mid, hc, out_h, top, crop_h, origin=ylo)
    return np.ascontiguousarray(res)


def frame_inputs(frames, targets):
    """frames uint8 [n, h, w, 3], targets [k, 10] -> list of uint8 [n, crop_h, crop_w, 3]"""
    frames = np.asarray(frames, np.uint8)
    out = []
    for t in np.asarray(targets, np.int64).reshape(-1, 10):
        out.append(np.stack([window(f, t) for f in frames]) if len(frames) else np.empty((0, int(t[8]), int(t[9]), 3), np.uint8))
    return out
