"""numpy restatement of the Canny contract of vsc_canny_count_u8 (include/vsc_hip.h): OpenCV 4.x's non-IPP Canny for 3-channel
8-bit input, as the reference calls it (``cv2.Canny(frame, 50, 400) > 0``, infer/src/image_preprocess.py:263).

It is written from OpenCV's published algorithm, not pinned against cv2 (not installed where the fixtures are made).  Hysteresis
uses ``scipy.ndimage.label`` with 8-connectivity -- a different algorithm from the kernel's union-find."""
from __future__ import annotations

import numpy as np

TG22 = 13573     # tan(22.5 deg) in Q15


def sobel(img: np.ndarray):
    """uint8 [H, W, C] -> (dx, dy) int32 [H, W, C]: 3x3 Sobel, replicated border (CV_16S range)"""
    p = np.pad(img.astype(np.int32), ((1, 1), (1, 1), (0, 0)), mode="edge")
    dx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    dy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    return dx, dy


def gradient(img: np.ndarray):
    """-> (mag, dx, dy) int32 [H, W]: per pixel the channel with the largest |dx| + |dy| (ties: the lower channel)"""
    if img.ndim == 2:
        img = img[:, :, None]
    dx, dy = sobel(img)
    mags = np.abs(dx) + np.abs(dy)
    c = np.argmax(mags, axis=-1)[..., None]          # first maximum = lower channel on a tie
    return (np.take_along_axis(mags, c, -1)[..., 0], np.take_along_axis(dx, c, -1)[..., 0],
            np.take_along_axis(dy, c, -1)[..., 0])


def nms(mag, dx, dy, low: float, high: float):
    """-> (weak, strong) bool [H, W] after the magnitude threshold and fixed-point non-maximum suppression"""
    low, high = int(np.floor(low)), int(np.floor(high))
    h, w = mag.shape
    m = np.zeros((h + 2, w + 2), np.int64)       # magnitude outside the image counts as 0
    m[1:-1, 1:-1] = mag
    c = m[1:-1, 1:-1]
    ax, ay = np.abs(dx).astype(np.int64), np.abs(dy).astype(np.int64) << 15
    tg22x = ax * TG22
    tg67x = tg22x + (ax << 16)
    horiz = ay < tg22x
    vert = ~horiz & (ay > tg67x)
    diag = ~horiz & ~vert
    neg = (dx.astype(np.int64) ^ dy.astype(np.int64)) < 0       # s = -1: up-right / down-left, else up-left / down-right
    keep_h = (c > m[1:-1, :-2]) & (c >= m[1:-1, 2:])
    keep_v = (c > m[:-2, 1:-1]) & (c >= m[2:, 1:-1])
    keep_d = np.where(neg, (c > m[:-2, 2:]) & (c > m[2:, :-2]), (c > m[:-2, :-2]) & (c > m[2:, 2:]))
    keep = (c > low) & ((horiz & keep_h) | (vert & keep_v) | (diag & keep_d))
    strong = keep & (c > high)
    return keep & ~strong, strong


def hysteresis(weak, strong):
    """edge = weak or strong pixel whose 8-connected component of weak | strong holds a strong pixel"""
    from scipy import ndimage
    fg = weak | strong
    labels, n = ndimage.label(fg, structure=np.ones((3, 3), bool))
    if n == 0:
        return np.zeros(fg.shape, bool)
    has_strong = np.zeros(n + 1, bool)
    has_strong[labels[strong]] = True
    has_strong[0] = False
    return has_strong[labels]


def canny(img: np.ndarray, low: float = 50, high: float = 400) -> np.ndarray:
    """uint8 [H, W, 3] -> uint8 [H, W] with 255 at edges (cv2.Canny's output convention)"""
    mag, dx, dy = gradient(img)
    weak, strong = nms(mag, dx, dy, low, high)
    return hysteresis(weak, strong).astype(np.uint8) * 255


def canny_count(frames, idx, low: float = 50, high: float = 400) -> np.ndarray:
    """vsc_canny_count_u8 on the CPU: per pixel, the number of frames[idx] where canny() marks an edge -> uint16 [H, W]"""
    out = None
    for i in idx:
        e = (canny(np.asarray(frames[i]), low, high) > 0).astype(np.uint16)
        out = e if out is None else out + e
    return out


def frame_var(frames) -> np.ndarray:
    """the reference's variance map (image_preprocess.py:255-256): float64 [H, W]"""
    return np.stack([np.asarray(f) for f in frames]).var(axis=0).sum(-1)
