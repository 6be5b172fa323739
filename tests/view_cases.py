"""Seeded synthetic query videos for the view preprocessing (border removal and split views, src/image_preprocess.py).

A case is a small JSON-able recipe; ``frames(case)`` rebuilds its uint8 frames [n, H, W, 3] bit for bit.  Moving panels change
colour from frame to frame (high variance, smooth inside, so few interior edges); borders and separating bands are static.  The
fixture tests/golden/view_preprocess.json stores the recipes, digests and the reference's decisions, never frames."""
from __future__ import annotations

import hashlib

import numpy as np


def _panel(rng, n, h, w, edges=False, levels=(150, 241)):
    """moving content: a per-frame colour in [levels) over a slow gradient, light noise; ``edges``: plus a drifting dark square"""
    t = np.arange(n, dtype=np.float64)[:, None, None, None]
    base = rng.integers(levels[0], levels[1], size=(n, 1, 1, 3)).astype(np.float64)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    grad = 12.0 * np.sin(2 * np.pi * (xx / max(w, 1) + yy / max(2 * h, 1))[None, :, :, None] + t / 5.0)
    img = base + grad + rng.integers(-2, 3, size=(n, h, w, 3))
    if edges and h >= 12 and w >= 12:
        s = max(4, min(h, w) // 5)
        for i in range(n):
            y0 = (3 * i) % max(1, h - s)
            x0 = (5 * i) % max(1, w - s)
            img[i, y0:y0 + s, x0:x0 + s] = 30.0
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _static(rng, h, w, level=20, texture=False):
    """a static background: flat, or a smooth low-contrast texture (no Canny edges of its own)"""
    if not texture:
        return np.full((h, w, 3), level, np.uint8)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    tex = level + 15.0 * np.sin(xx / 9.0)[:, :, None] * np.array([1.0, 0.7, 0.4]) + 10.0 * np.cos(yy / 11.0)[:, :, None]
    return np.clip(np.rint(tex), 0, 255).astype(np.uint8)


def frames(case) -> np.ndarray:
    """uint8 [n, H, W, 3] of a recipe: a static background of (H, W) with moving panels pasted at their boxes"""
    rng = np.random.default_rng(case["seed"])
    n, (h, w) = case["n"], case["size"]
    bg = _static(rng, h, w, case.get("level", 20), case.get("texture", False))
    out = np.broadcast_to(bg, (n, h, w, 3)).copy()
    levels = case.get("levels", [[150, 241]] * len(case["panels"]))
    for (y0, y1, x0, x1), lv in zip(case["panels"], levels):
        out[:, y0:y1, x0:x1] = _panel(rng, n, y1 - y0, x1 - x0, case.get("edges", False), lv)
    return out


def digest(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def _case(name, seed, n, size, panels, **kw):
    return dict(name=name, seed=seed, n=n, size=list(size), panels=[list(p) for p in panels], **kw)


def cases():
    """every recipe of the fixture, in a fixed order"""
    c = []
    c.append(_case("letterbox", 1, 12, (160, 200), [(20, 140, 0, 200)]))
    c.append(_case("pillarbox", 2, 12, (150, 220), [(0, 150, 30, 190)]))
    c.append(_case("picture_in_picture", 3, 10, (180, 240), [(40, 150, 50, 200)], level=70, texture=True))
    c.append(_case("stack2_vertical", 4, 8, (210, 180), [(0, 100, 0, 180), (110, 210, 0, 180)]))
    c.append(_case("stack2_horizontal", 5, 8, (160, 250), [(0, 160, 0, 120), (0, 160, 130, 250)]))
    c.append(_case("stack3_vertical", 6, 8, (310, 150), [(0, 100, 0, 150), (105, 205, 0, 150), (210, 310, 0, 150)]))
    c.append(_case("stack3_horizontal", 7, 8, (140, 330), [(0, 140, 0, 100), (0, 140, 110, 210), (0, 140, 220, 330)]))
    c.append(_case("border_and_stack", 8, 9, (260, 200), [(30, 130, 0, 200), (140, 230, 0, 200)]))
    c.append(_case("plain", 9, 12, (144, 176), [(0, 144, 0, 176)], edges=True))
    c.append(_case("plain_smooth", 10, 7, (120, 160), [(0, 120, 0, 160)]))
    c.append(_case("three_frames", 11, 3, (160, 200), [(20, 140, 0, 200)]))
    c.append(_case("letterbox_n21", 12, 21, (120, 160), [(16, 104, 0, 160)]))
    c.append(_case("letterbox_n57", 13, 57, (96, 128), [(12, 84, 0, 128)]))
    c.append(_case("letterbox_n43", 14, 43, (96, 128), [(12, 84, 0, 128)]))
    c.append(_case("crop_under_20", 15, 8, (100, 160), [(40, 55, 0, 160)]))
    # the height scan ends with start != 0 and no view (the band at rows 40-50 is too close to the top); the width scan then
    # starts from that row index instead of 0 and loses the left panel
    c.append(_case("height_scan_leaves_start", 16, 8, (120, 230),
                   [(0, 40, 0, 100), (0, 40, 110, 230), (50, 120, 0, 100), (50, 120, 110, 230)]))
    c.append(_case("pip_in_stack", 17, 8, (220, 200), [(0, 100, 0, 200), (130, 190, 40, 160)], level=20))
    c.append(_case("tiny_1px", 18, 6, (1, 9), [(0, 1, 0, 9)]))
    # stacked views that touch, one bright and one dark in turn: no static band between them, only a sharp edge line on every
    # frame -- split_imgs' edge-line cuts (cut_h when h >= w, cut_w first when w > h), which emit the views from the far end back
    bright, dark = [200, 241], [20, 61]
    c.append(_case("edge_lines_3_vertical", 19, 8, (300, 120), [(0, 100, 0, 120), (100, 200, 0, 120), (200, 300, 0, 120)],
                   levels=[bright, dark, bright]))
    c.append(_case("edge_lines_3_horizontal", 20, 8, (110, 300), [(0, 110, 0, 95), (0, 110, 95, 200), (0, 110, 200, 300)],
                   levels=[dark, bright, dark]))
    c.append(_case("edge_lines_2_vertical", 21, 9, (190, 150), [(0, 95, 0, 150), (95, 190, 0, 150)], levels=[dark, bright]))
    return c
