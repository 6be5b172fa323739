"""Query frame preprocessing: static-border removal and split views (reference: infer/src/image_preprocess.py, ``image_process``
and the ``remove_edges`` / ``split_imgs`` / ``clean_imgs`` it calls; applied to every query video by infer/src/dataset.py:82-88).

The reference crops and splits the frames themselves.  Here the decisions are taken on the two per-video maps they depend on --
the per-pixel variance over all frames and the Canny edge frequency over up to 20 sampled frames -- and come out as boxes
``(y0, y1, x0, x1)`` in frame coordinates, in the reference's view order.  The GPU computes the maps (``detect_views``:
vsc_frame_var_u8 and vsc_canny_count_u8) and cuts and resizes the views (vsc_resize_bicubic_u8); only the decisions run here --
or, with ``decisions="hip"``, on the device too (vsc_view_decide_f64: the same arithmetic on the maps where the kernels wrote
them, so that only the boxes come back).

Every threshold, scan order and quirk is the reference's, on the same numpy slices of the same maps, so the floating-point
results match too.  Where the reference raises inside its ``try`` (frames of different sizes, a sample index past the last
frame), the video is unchanged."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

Box = Tuple[int, int, int, int]          # y0, y1, x0, x1 (half-open, frame coordinates)

MIN_FRAMES = 5          # clean_imgs: fewer frames -> unchanged
CANNY_SAMPLES = 20      # image_process: Canny runs on ~20 evenly spaced frames of a longer video
CANNY_LOW, CANNY_HIGH = 50, 400
MIN_SIDE = 20           # clean_imgs: a cut under 20 px on a side leaves the region as it was
MIN_VIEW = 80           # clean_imgs -> split_imgs(min_size=80)
GAP = 5                 # split_imgs: width of the static band that separates two stacked views
# where the decisions run: "host" (decide_views in numpy on the downloaded maps, the default) or "hip" (vsc_view_decide_f64)
VIEW_DECISIONS = ("host", "hip")


def canny_frames(n: int) -> Optional[List[int]]:
    """Indices of the frames the reference runs Canny on (image_process:259-261): all of them up to 20, else the float range
    ``np.arange(0, n, n / 20)`` rounded half to even.  Should rounding of the float range give a 21st sample that rounds to ``n``,
    the reference indexes past its list and its ``try`` returns the video unchanged -- None here.  (numpy 2.2 gives exactly 20
    samples for every n from 21 to 200 000.)"""
    if n <= CANNY_SAMPLES:
        return list(range(n))
    idx = [int(np.round(i)) for i in np.arange(0, n, n / CANNY_SAMPLES)]
    return None if idx[-1] >= n else idx


def _static_side(var_p, edge_p, edge_at) -> bool:
    """remove_edges: the band beyond a candidate edge line is a static border"""
    level = np.median(var_p) + var_p.mean()
    calm = edge_p.mean() < 0.0225
    return bool((level < 75 and calm) or (level < 250 and calm and edge_at > 0.65))


def _trim(var_p, edge_p, size: int) -> Tuple[int, int]:
    """remove_edges along one axis: (first, end) kept, from the per-line variance and edge profiles of the region"""
    lines = [i for i in np.where(edge_p > 0.125 + edge_p.mean())[0] if i not in (0, size - 1)]
    first, end = 0, size
    for i in lines:
        if i - first < 5:
            continue
        extra = round((i - first) * 0.3)
        if _static_side(var_p[first:i - extra], edge_p[first:i - extra], edge_p[i]):
            first = i + 1
    for i in reversed(lines):
        if end - i < 5:
            continue
        extra = round((end - i) * 0.3)
        if _static_side(var_p[i + extra:end], edge_p[i + extra:end], edge_p[i]):
            end = i
    return first, end


def _borders(var, avg) -> Tuple[int, int, int, int]:
    """remove_edges -> the kept (y0, y1, x0, x1) inside the region"""
    threshold = min(max(np.quantile(avg, 0.95), 0.2), avg.mean() + 0.35)
    edges = (avg > threshold).astype(np.float32)
    h, w = var.shape
    y0, y1 = _trim(var.mean(1), edges.mean(1), h)
    x0, x1 = _trim(var.mean(0), edges.mean(0), w)
    return y0, y1, x0, x1


def _bands(profile, size: int, start: int, min_size: int) -> Tuple[List[Tuple[int, int]], int]:
    """split_imgs' scan of one axis: pieces that end at a static band, and where the scan's last piece started"""
    half = GAP // 2
    pieces, inside = [], False
    # profile[i:i + GAP].mean() for every i at once, in numpy's own order for a 5-element sum (sequential) and division
    p = np.asarray(profile, dtype=np.float64)
    n = max(size - GAP, 0)
    levels = ((((p[0:n] + p[1:n + 1]) + p[2:n + 2]) + p[3:n + 3]) + p[4:n + 4]) / GAP
    for i, level in enumerate(levels.tolist()):
        if not inside and (level > 0.1 or i - start > 50):
            inside = True
        elif inside and level < 0.1:
            if i + half - start > min_size:
                pieces.append((start, i + half))
            inside = False
            start = i + half
    return pieces, start


def _line_cuts(lines: Sequence[int], size: int, min_size: int) -> List[Tuple[int, int]]:
    """split_imgs' cut_h / cut_w: pieces between strong edge lines, from the far end back"""
    pieces, end = [], size
    for i in lines:
        if end - i > min_size:
            pieces.append((i, end))
            end = i
    if pieces and end > min_size:
        pieces.append((0, end))
    return pieces


def _split(var, avg, min_size: int) -> Optional[List[Box]]:
    """split_imgs -> boxes inside the region, or None when it stays whole"""
    h, w = var.shape
    rows, start = _bands(var.mean(1), h, 0, min_size)
    if rows or start != 0:
        if h - start > min_size:
            rows.append((start, h))
        if rows:
            return [(a, b, 0, w) for a, b in rows]
    # the reference's width scan starts from where the height scan left `start`
    cols, start = _bands(var.mean(0), w, start, min_size)
    if cols or start != 0:
        if w - start > min_size:
            cols.append((start, w))
        if cols:
            return [(0, h, a, b) for a, b in cols]
    threshold = min(max(np.quantile(avg, 0.95), 0.2), avg.mean() + 0.3)
    edges = (avg > threshold).astype(np.float32)
    level = 0.45 + edges.mean()
    row_lines = list(np.where(edges.mean(1) > level)[0])[::-1]
    col_lines = list(np.where(edges.mean(0) > level)[0])[::-1]
    by_rows = lambda: [(a, b, 0, w) for a, b in _line_cuts(row_lines, h, min_size)]     # noqa: E731
    by_cols = lambda: [(0, h, a, b) for a, b in _line_cuts(col_lines, w, min_size)]     # noqa: E731
    for cut in ((by_cols, by_rows) if w > h else (by_rows, by_cols)):
        pieces = cut()
        if pieces:
            return pieces
    return None


def _clean(var, avg, box: Box, n: int) -> List[Box]:
    """clean_imgs on the region ``box`` of the maps -> its views"""
    if n < MIN_FRAMES:
        return [box]
    y0, y1, x0, x1 = box
    b0, b1, a0, a1 = _borders(var[y0:y1, x0:x1], avg[y0:y1, x0:x1])
    cut = (y0 + b0, y0 + b1, x0 + a0, x0 + a1)
    if min(b1 - b0, a1 - a0) < MIN_SIDE:
        return [box]
    pieces = _split(var[cut[0]:cut[1], cut[2]:cut[3]], avg[cut[0]:cut[1], cut[2]:cut[3]], MIN_VIEW)
    if pieces is None or (len(pieces) == 1 and (pieces[0][1] - pieces[0][0], pieces[0][3] - pieces[0][2]) == (b1 - b0, a1 - a0)):
        return [cut]
    views = []
    for p0, p1, q0, q1 in pieces:
        views.extend(_clean(var, avg, (cut[0] + p0, cut[0] + p1, cut[2] + q0, cut[2] + q1), n))
    return views


def decide_views(var: np.ndarray, count: np.ndarray, m: int, n: int) -> Tuple[bool, List[Box]]:
    """image_process on the maps of one video of ``n`` frames: ``var`` float64 [H, W] (np.stack(frames).var(0).sum(-1)) and
    ``count`` [H, W], the number of the ``m`` sampled frames where Canny marks an edge.  -> (changed, boxes): the views in the
    reference's order, or (False, [whole frame])."""
    h, w = var.shape
    whole = (0, h, 0, w)
    if n < MIN_FRAMES:
        return False, [whole]
    avg = np.asarray(count).astype(np.float64) / m
    with np.errstate(all="ignore"):
        views = _clean(np.asarray(var, dtype=np.float64), avg, whole, n)
    if len(views) > 1 or (views[0][1] - views[0][0], views[0][3] - views[0][2]) != (h, w):
        return True, views
    return False, [whole]


def detect_views(frames_dev, decisions: str = "host") -> Tuple[bool, List[Box]]:
    """The views of one video whose uint8 frames [n, H, W, 3] are on the GPU: one vsc_frame_var_u8 and one vsc_canny_count_u8
    launch, one device -> host copy of both maps, then ``decide_views``.  ``decisions="hip"``: the maps stay where the kernels
    wrote them, one vsc_view_decide_f64 launch follows and one copy of the boxes, their count and the status comes back; a video
    the kernel leaves to the host (status 1: more views or pending regions than it holds) or cannot take (a side above its limit)
    goes through the host path.  Launch and device errors propagate."""
    if decisions not in VIEW_DECISIONS:
        raise ValueError(f"decisions must be one of {VIEW_DECISIONS}, not {decisions!r}")
    n, h, w = (int(s) for s in frames_dev.shape[:3])
    whole = (0, h, 0, w)
    idx = canny_frames(n)
    if n < MIN_FRAMES or idx is None:
        return False, [whole]
    from vsc_hip import ops
    if decisions == "hip" and max(h, w) <= ops.VIEW_DECIDE_MAX_SIDE:
        var, count = ops.view_maps_dev(frames_dev, idx, CANNY_LOW, CANNY_HIGH)
        k = ops.VIEW_DECIDE_MAX_VIEWS
        out = _flat_i32(ops.view_decide(var, count, [(0, 0, h, w, len(idx), n)], k)).cpu().numpy()
        if out[4 * k + 1] == 0:
            views = [tuple(int(v) for v in out[4 * i:4 * i + 4]) for i in range(int(out[4 * k]))]
            return (len(views) > 1 or views[0] != whole), views
        return decide_views(var.cpu().numpy(), count.cpu().numpy(), len(idx), n)
    var, count = ops.view_maps(frames_dev, idx, CANNY_LOW, CANNY_HIGH)
    return decide_views(var, count, len(idx), n)


def _flat_i32(parts):
    """the int32 device tensors of one call as one flat tensor: one device -> host copy instead of three"""
    import torch
    return torch.cat([p.reshape(-1) for p in parts])


class HipViews:
    """``run_query_videos(views=HipViews(device))`` for ``--preprocess hip``: uploads a video's full-resolution uint8 frames,
    ``detect_views`` on them, then one vsc_resize_bicubic_u8 per encoder input size -> (boxes, {size: uint8 [k * n, size, size, 3]
    on the device}).  The work runs on a side stream, so the host's wait for the two maps does not wait for the encoders queued
    on the caller's stream; the caller's stream is ordered behind the resized views.  ``decisions``: "host" or "hip", as
    ``detect_views`` takes it."""

    def __init__(self, device, decisions: str = "host"):
        import torch
        if decisions not in VIEW_DECISIONS:
            raise ValueError(f"decisions must be one of {VIEW_DECISIONS}, not {decisions!r}")
        self.decisions = decisions
        self.device = torch.device(device)
        self.stream = torch.cuda.Stream(device=self.device)

    def on_device(self, frames, sizes):
        """the views of frames that are on the device already, on the current stream"""
        from vsc_hip import ops
        _, boxes = detect_views(frames, self.decisions)
        return boxes, {size: ops.resize_bicubic(frames, boxes, size) for size in sizes}

    def __call__(self, raw, sizes):
        import torch
        main = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self.stream):
            boxes, out = self.on_device(raw.to(self.device), sizes)
        main.wait_stream(self.stream)
        for t in out.values():
            t.record_stream(main)
        return boxes, out


class HipResize:
    """``--resize hip``: every model input of a video from its decoded frames, on the device.  ``resizer(raw, sizes)`` uploads the
    uint8 frames [n, H, W, 3] once -- through a pinned buffer with a non-blocking copy -- and one vsc_frame_inputs_u8 call makes the
    encoder input of every size (vit_transform_u8's resize) and, with ``clip_key``, the video-score input (clip_transform_u8(224))
    -> (None, {size or clip_key: uint8 [n, s, s, 3] on the device}).  With ``views`` (a HipViews: ``--preprocess hip``) the views
    are made as HipViews makes them, from the same uploaded frames, and the call returns their boxes; only the video-score input
    then comes from vsc_frame_inputs_u8.  The work runs on a side stream, as in HipViews; the caller's stream is ordered behind
    the results."""

    def __init__(self, device, clip_size: int = 224):
        import torch
        self.device = torch.device(device)
        self.clip_size = clip_size
        self.stream = torch.cuda.Stream(device=self.device)
        self.pinned = None
        self.copied = torch.cuda.Event()      # the last copy out of the pinned buffer is done
        self.used = False

    def upload(self, raw):
        """host frames -> device, on the current stream; the pinned buffer grows to the largest video seen"""
        import torch
        if raw.is_cuda:
            return raw
        raw = raw.contiguous()
        if self.used:
            self.copied.synchronize()
        if self.pinned is None or self.pinned.numel() < raw.numel():
            self.pinned = torch.empty(raw.numel(), dtype=torch.uint8).pin_memory()
        staged = self.pinned[:raw.numel()].view(raw.shape)
        staged.copy_(raw)
        frames = torch.empty(raw.shape, dtype=torch.uint8, device=self.device)
        frames.copy_(staged, non_blocking=True)
        self.copied.record(torch.cuda.current_stream(self.device))
        self.used = True
        return frames

    def __call__(self, raw, sizes, views=None, clip_key=None):
        import torch
        from src.dataset import clip_target, square_target
        from vsc_hip import ops
        main = torch.cuda.current_stream(self.device)
        if raw.is_cuda:
            self.stream.wait_stream(main)     # frames made on the caller's stream
        with torch.cuda.stream(self.stream):
            frames = self.upload(raw)
            h, w = int(frames.shape[1]), int(frames.shape[2])
            boxes, out, keys, targets = None, {}, [], []
            if views is not None:
                boxes, out = views.on_device(frames, sizes)
            else:
                keys, targets = list(sizes), [square_target(h, w, size) for size in sizes]
            if clip_key is not None:
                keys.append(clip_key)
                targets.append(clip_target(h, w, self.clip_size))
            if targets:
                out.update(zip(keys, ops.frame_inputs(frames, targets)))
        main.wait_stream(self.stream)
        for t in out.values():
            t.record_stream(main)
        return boxes, out


class HipDecode:
    """``--decode hip``: the jpg files of a loader batch decoded on the device.  ``decoder(videos)`` takes the batch's BytesVideo
    items (src.dataset), copies their bytes into one pinned buffer, uploads it with one non-blocking copy on a side stream and
    decodes every frame of every video with one vsc_jpeg_decode_u8 call -> per video uint8 [S, H, W, 3] on the device, bit for bit
    what Pillow gives the workers; HipResize and HipViews take them as they are.  The per-frame status comes back with one small
    copy that waits for the side stream only.  A video with a frame whose scan the kernel gave up on is decoded by Pillow here,
    in the main process, as a whole (host frames; Pillow raises or decodes leniently as it does in the workers) and a warning
    names it.  The caller's stream is ordered behind the results.
    ``split`` (``--decode_split``: "none", "markers", "substreams" or "all"): frames are decoded in parallel inside, at their
    restart markers and / or as self-synchronising sub-streams (vsc_jpeg_decode_split_u8: the same bytes and status).
    ``scans`` (``--decode_scans``: "host" or "hip"): with "hip" the videos may hold frames of several scans (vsc_hip.jpeg.ScanFrame:
    progressive, one scan per component, Huffman table ids 0 .. 3).  A batch that holds one goes through
    vsc_jpeg_decode_scans_u8, single-scan frames included; with ``split`` the single-scan frames are cut as before in a call of
    their own and the others follow in a second call, one wave each."""

    def __init__(self, device, split="none", scans="host"):
        import torch
        from src.dataset import check_decode_scans, check_decode_split
        self.split = check_decode_split(split)
        self.scans = check_decode_scans(scans)
        self.device = torch.device(device)
        self.stream = torch.cuda.Stream(device=self.device)
        self.pinned = None
        self.copied = torch.cuda.Event()      # the last copy out of the pinned buffer is done
        self.used = False

    def __call__(self, videos):
        import io
        import warnings

        import torch
        from PIL import Image
        from src.dataset import decode_rgb
        from vsc_hip import jpeg, ops
        if not videos:
            return []
        sets = jpeg.TableSets()
        several = any(isinstance(r, jpeg.ScanFrame) for v in videos for r in v.records)
        assert not several or self.scans == "hip", "a video with frames of several scans reached a decoder made with scans='host'"
        rows, spans, at_bytes, at_out = [], [], 0, 0
        records, file_at, out_at = [], [], []
        for v in videos:
            n, h, w = v.shape
            if several:
                records += list(v.records)
                file_at += (v.offsets[:-1] + at_bytes).tolist()
                out_at += [at_out + i * h * w * 3 for i in range(n)]
            else:
                rows.append(jpeg.frame_rows(v.records, (v.offsets[:-1] + at_bytes).tolist(), [at_out + i * h * w * 3 for i in range(n)], sets))
            spans.append((at_out, n, h, w))
            at_bytes += int(v.data.numel())
            at_out += n * h * w * 3
        main = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self.stream):
            if self.used:
                self.copied.synchronize()
            if self.pinned is None or self.pinned.numel() < at_bytes:
                self.pinned = torch.empty(at_bytes, dtype=torch.uint8).pin_memory()
            at = 0
            for v in videos:
                self.pinned[at:at + v.data.numel()].copy_(v.data)
                at += int(v.data.numel())
            data = torch.empty(at_bytes, dtype=torch.uint8, device=self.device)
            data.copy_(self.pinned[:at_bytes], non_blocking=True)
            self.copied.record(torch.cuda.current_stream(self.device))
            self.used = True
            restarts = jpeg.concat_restart_rows([v.restarts for v in videos]) if self.split != "none" else None
            if not several:
                out, status = ops.jpeg_decode(data, np.concatenate(rows), sets.array(), at_out, restarts=restarts, split=self.split)
                status = status.cpu().numpy()          # waits for this stream only
            else:
                # with a split the single-scan frames keep it, in a call of their own; every other frame, or without a split every frame, is one wave
                one = [i for i, r in enumerate(records) if isinstance(r, jpeg.Frame)] if self.split != "none" else []
                rest = sorted(set(range(len(records))) - set(one))
                out = torch.empty(at_out, dtype=torch.uint8, device=self.device)
                status = np.zeros(len(records), np.int32)
                first_status = None
                if one:
                    rptr = np.concatenate([[0], np.cumsum(np.diff(restarts[0])[one])]).astype(np.int64)
                    roff = np.concatenate([restarts[1][restarts[0][i]:restarts[0][i + 1]] for i in one]).astype(np.int32)
                    r1 = jpeg.frame_rows([records[i] for i in one], [file_at[i] for i in one], [out_at[i] for i in one], sets)
                    _, first_status = ops.jpeg_decode(data, r1, sets.array(), at_out, out=out, restarts=(rptr, roff), split=self.split)
                wide = jpeg.ScanTableSets()
                r2, srows, sptr = jpeg.scan_rows([records[i] for i in rest], [file_at[i] for i in rest], [out_at[i] for i in rest], wide)
                _, st = ops.jpeg_decode(data, r2, wide.array(), at_out, out=out, scans=(srows, sptr))
                status[rest] = st.cpu().numpy()        # waits for this stream only
                if first_status is not None:
                    status[one] = first_status.cpu().numpy()
        main.wait_stream(self.stream)
        out.record_stream(main)
        frames, first = [], 0
        for v, (at, n, h, w) in zip(videos, spans):
            bad = np.flatnonzero(status[first:first + n])
            first += n
            if len(bad):
                warnings.warn(f"--decode hip: frame {int(bad[0])} of a video of {n} frames has a damaged scan (status {int(status[first - n + bad[0]])}); "
                              "the video is decoded on the host")
                frames.append(torch.from_numpy(np.stack([decode_rgb(Image.open(io.BytesIO(f))) for f in v.files()])))
            else:
                frames.append(out[at:at + n * h * w * 3].view(n, h, w, 3))
        return frames
