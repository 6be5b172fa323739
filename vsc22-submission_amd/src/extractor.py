"""Frame -> descriptor extraction loop (reference: infer/src/extractor.py:9-38).

`model` is anything with the reference's call shape -- here a vsc_hip.encoder.HipEncoder.
A batch is (frames [B,S,3,H,W] padded, mask [B,S], video_ids) exactly as D_vsc.collate_fn
builds it (infer/src/dataset.py:145-153).

The reference encodes loader batch by loader batch (two videos: ~100 frames per call, a synchronous pageable upload in front and a
device -> host copy behind every one).  Here the valid frames of consecutive loader batches are collected, on the host, into groups of
>= `group_frames` frames (4 096: the ragged last chunk of a group is then a percent of it) and go through `src.query_pipeline.encode_group`: pinned staging + a copy stream, encoder calls of the
backbone's aligned chunk, one device -> host copy per group.  A frame's descriptor does not depend on WHICH frames share its call, but
the encoders choose kernels by a call's row count (Swin-V2's 512-wide stage: the one-launch second half from 77 frames per chunk on, GEMM
launches below; the ViT's persistent GEMMs need more tiles than CUs) and the two forms round in different orders: the same frame in a
large and in a small call agrees to rounding-order noise (measured <= 2e-4 with bf16 operands, <= 4e-5 with fp16:
tests/test_gpu_swin.py::test_a_frame_alone_and_inside_a_full_chunk), not bit for bit."""
from __future__ import annotations

from typing import Iterable, List, Tuple

import numpy as np
import torch


def extract_vsc_feat(model, batches: Iterable, device, group_frames: int = 4096) -> Tuple[List[str], np.ndarray, np.ndarray]:
    def videos():
        for frames, mask, video_id in batches:
            mask = mask.bool()
            counts = mask.sum(dim=1).tolist()
            yield [(v, frames[b][:int(c)] if bool(mask[b, :int(c)].all()) else frames[b][mask[b]])   # (the collate pads at the end: a view, no copy)
                   for b, (v, c) in enumerate(zip(video_id, counts))]
    return _extract(model, videos(), device, group_frames)


def extract_vsc_feat_raw(model, batches: Iterable, device, image_size: int, resizer, group_frames: int = 4096, decoder=None):
    """``extract_vsc_feat`` for ``--resize hip``: a loader batch is a list of (frames, video_id) as the workers decoded them, uint8
    [S, H, W, 3] at the zip's own resolution (``src.dataset.raw_collate``).  Every video is uploaded and resized to the encoder's
    input by one vsc_frame_inputs_u8 call (``resizer``: src.image_preprocess.HipResize) and the groups are encoded from device
    tensors.  Groups close at the same loader batches and hold the same frames in the same order as with host resizing, so the
    same frames share the same encoder calls.  A video the worker already resized (its frames differ in size) arrives as uint8
    [S, image_size, image_size, 3] and goes through from the host.
    ``decoder`` (``--decode hip``: src.image_preprocess.HipDecode): the batch's videos that arrive as compressed bytes
    (src.dataset.BytesVideo) are decoded on the device first, all of them in one vsc_jpeg_decode_u8 call."""
    from src.dataset import BytesVideo

    def videos():
        for batch in batches:
            packed = [i for i, (frames, _) in enumerate(batch) if isinstance(frames, BytesVideo)]
            if packed:
                if decoder is None:
                    raise ValueError("the loader yields compressed videos (raw='bytes') and there is no decoder")
                batch = list(batch)
                for i, frames in zip(packed, decoder([batch[i][0] for i in packed])):
                    batch[i] = (frames, batch[i][1])
            out = []
            for frames, v in batch:
                if frames.shape[0] and tuple(frames.shape[1:3]) != (image_size, image_size):
                    frames = resizer(frames, [image_size])[1][image_size]
                out.append((v, frames))
            yield out
    return _extract(model, videos(), device, group_frames)


def extract_cnn_feat(model, batches: Iterable, device) -> Tuple[List[str], np.ndarray, np.ndarray]:
    """``extract_vsc_feat`` for a CNN encoder (vsc_hip.cnn_encoder.CnnHipEncoder), whose frames keep their own H x W: a loader
    batch is a list of (frames, video_id) (``src.dataset.raw_collate``), frames a uint8 tensor [S, H, W, 3] or -- the transforms keep
    the aspect ratio, so the frames of one video may differ in size -- a list of S tensors [H_i, W_i, 3].  All frames of a batch are
    encoded per (H, W), one call per distinct size, and come back in the loader's order.  Same outputs as ``extract_vsc_feat``."""
    feats, vids, stamps = [], [], []
    for batch in batches:
        sizes = {}
        for i, (frames, _) in enumerate(batch):
            for j, f in enumerate(frames):
                sizes.setdefault(tuple(f.shape[:2]), []).append((i, j))
        outs = [[None] * len(frames) for frames, _ in batch]
        for where in sizes.values():
            desc = model(torch.stack([batch[i][0][j] for i, j in where]).to(device, non_blocking=True)).cpu().numpy()
            for row, (i, j) in zip(desc, where):
                outs[i][j] = row
        for i, (frames, v) in enumerate(batch):
            c = len(frames)
            vids.extend([v] * c)
            stamps.append(np.arange(c))
            if c:
                feats.append(np.stack(outs[i]))
    if not stamps:
        return [], np.zeros((0, 0), np.float32), np.zeros((0,), np.int64)
    if not feats:
        return vids, np.zeros((0, 0), np.float32), np.concatenate(stamps)
    return vids, np.concatenate(feats), np.concatenate(stamps)


def _extract(model, batches: Iterable, device, group_frames: int) -> Tuple[List[str], np.ndarray, np.ndarray]:
    """batches yields one list of (video_id, valid frames) per loader batch"""
    from src.query_pipeline import encode_group
    feats, vids, stamps = [], [], []
    group, have = [], 0
    pending = None      # the previous group's descriptors, still on the device

    def collect():
        nonlocal pending
        if pending is not None:
            feats.append(torch.cat(pending).cpu().numpy() if len(pending) > 1 else pending[0].cpu().numpy())
            pending = None

    def flush():
        # One group of look-ahead (round 6): a group's uploads and launches are QUEUED here (device tensors back, no wait); its descriptors
        # are copied back when the next group has been queued behind it -- so the loader's next batches are collated while this group is
        # encoded, instead of behind it.  On the CPU (host-logic tests with fake encoders) nothing is asynchronous and nothing changes.
        nonlocal group, have, pending
        if group:
            on_gpu = torch.device(device).type == "cuda"
            outs = encode_group([model], group, device, as_numpy=not on_gpu)[0]
            collect()
            if on_gpu:
                pending = [o for o in outs if o.shape[0] > 0]
            else:
                feats.extend(outs)
        group, have = [], 0

    for batch in batches:
        for v, f in batch:
            c = int(f.shape[0])
            vids.extend([v] * c)
            stamps.append(np.arange(c))
            if c:
                group.append(f)
                have += c
        if have >= group_frames:
            flush()
    flush()
    collect()
    if not stamps:
        return [], np.zeros((0, 0), np.float32), np.zeros((0,), np.int64)
    if not feats:
        return vids, np.zeros((0, 0), np.float32), np.concatenate(stamps)
    return vids, np.concatenate(feats), np.concatenate(stamps)
