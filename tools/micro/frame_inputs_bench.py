"""Model-input frame resizing on the device, measured (run on the GPU box; DESIGN.md 4.18 quotes the output):
      python tools/micro/frame_inputs_bench.py [--kernel] [--e2e] [--videos N] > profiles/frame_inputs_bench.txt
(a) --kernel: 40 whole frames at 360p / 720p / 1080p.  The yardstick is vsc_resize_bicubic_u8 (two launches per size through an
    HBM intermediate) for the targets 256 + 384; against it one vsc_frame_inputs_u8 call with {256, 384} and one with {256, 384,
    CLIP 224}.  Device events around every call, the same input for every launch, the variants interleaved round by round, the
    median of ROUNDS rounds.  Source bytes read per second = targets x frame bytes / time, against the chip's 6.3 TB/s copy rate.
(b) --e2e: run_query_videos through the reference's ensemble (tools/ensemble_bench.py: synthetic weights) on 40-frame 720p videos
    whose decoded frames are in memory: resize="host" -- a DataLoader with 6 workers resizing with Pillow to 256, 384 and the
    CLIP input, as extract_query_feats.py does -- against resize="hip", where the workers hand the decoded frames over.  And the
    reference-side loop (extract_vsc_feat / extract_vsc_feat_raw, one Swin-V2-B/256, 4 workers) the same way."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (os.path.join(ROOT, "vsc22-submission_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np
import torch

ROUNDS = 9
COPY_RATE = 6.3e12


def kernel_bench(dev):
    from src.dataset import clip_target, square_target
    from vsc_hip import ops
    print(f"(a) kernel time, 40 frames, median of {ROUNDS} interleaved rounds, device events")
    for name, (h, w) in (("360p", (360, 640)), ("720p", (720, 1280)), ("1080p", (1080, 1920))):
        frames = torch.from_numpy(np.random.default_rng(h).integers(0, 256, (40, h, w, 3), dtype=np.uint8)).to(dev)
        outs = {s: torch.empty((40, s, s, 3), dtype=torch.uint8, device=dev) for s in (256, 384, 224)}
        t2 = [square_target(h, w, 256), square_target(h, w, 384)]
        t3 = t2 + [clip_target(h, w, 224)]
        box = [(0, h, 0, w)]

        def two_pass():
            ops.resize_bicubic(frames, box, 256, out=outs[256])
            ops.resize_bicubic(frames, box, 384, out=outs[384])

        variants = {"resize_bicubic 256+384 (two-pass)": (two_pass, 2),
                    "frame_inputs {256, 384}": (lambda: ops.frame_inputs(frames, t2, outs=[outs[256], outs[384]]), 2),
                    "frame_inputs {256, 384, CLIP 224}": (lambda: ops.frame_inputs(frames, t3, outs=[outs[256], outs[384], outs[224]]), 3)}
        for fn, _ in variants.values():
            fn()
        torch.cuda.synchronize()
        want = {s: o.clone() for s, o in outs.items()}
        times = {k: [] for k in variants}
        for _ in range(ROUNDS):
            for k, (fn, _) in variants.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[k].append(a.elapsed_time(b))
        assert all(torch.equal(outs[s], want[s]) for s in (256, 384)), "the variants disagree"
        base = statistics.median(times["resize_bicubic 256+384 (two-pass)"])
        for k, (_, targets) in variants.items():
            ms = statistics.median(times[k])
            rate = targets * frames.numel() / (ms * 1e-3)
            print(f"  {name} {k:36s} {ms:8.3f} ms (min {min(times[k]):.3f}, max {max(times[k]):.3f})  {ms / base:5.2f} x two-pass  "
                  f"{rate / 1e12:5.2f} TB/s of source bytes = {100 * rate / COPY_RATE:4.1f} % of the copy rate")


class _Decoded(torch.utils.data.Dataset):
    """videos whose decoded frames are in memory; the worker resizes them with Pillow (host) or hands them over (hip)"""

    def __init__(self, n_videos, frames, sizes, with_clip, resize, ref_size=None):
        self.n, self.frames, self.sizes, self.with_clip, self.resize, self.ref_size = n_videos, frames, sizes, with_clip, resize, ref_size

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        from PIL import Image
        from src.dataset import clip_transform_u8, vit_transform_u8
        from src.query_pipeline import RAW_KEY, VideoScorer
        vid, n = f"Q{i:06d}", len(self.frames)
        if self.ref_size is not None:
            if self.resize == "hip":
                return torch.from_numpy(self.frames), vid
            t = vit_transform_u8(self.ref_size, self.ref_size)
            return torch.stack([t(Image.fromarray(f)) for f in self.frames]), vid
        stamps = np.stack([np.arange(n, dtype=np.float32), np.arange(n, dtype=np.float32) + 1.0], axis=1)
        if self.resize == "hip":
            return vid, {RAW_KEY: torch.from_numpy(self.frames)}, stamps
        images = [Image.fromarray(f) for f in self.frames]
        out = {s: torch.stack([vit_transform_u8(s, s)(im) for im in images]) for s in self.sizes}
        if self.with_clip:
            out[VideoScorer.KEY] = torch.stack([clip_transform_u8(224)(im) for im in images])
        return vid, out, stamps


def e2e_bench(dev, n_videos):
    from src.dataset import collate_fn, raw_collate
    from src.extractor import extract_vsc_feat, extract_vsc_feat_raw
    from src.image_preprocess import HipResize
    from src.query_pipeline import run_query_videos
    from src.query_postprocess import HipPCA
    from tools import ensemble_bench
    m = ensemble_bench.build(dev, "fp16")
    encoders = [(s, 256) for s in m["swins"]] + [(m["vit"], 384)]
    pca = HipPCA(ensemble_bench._Fitted)
    frames = np.random.default_rng(1).integers(0, 256, (40, 720, 1280, 3), dtype=np.uint8)
    total = n_videos * 40
    print(f"(b) end to end, {n_videos} videos of 40 decoded 720p frames in memory ({frames.nbytes / 1e6:.0f} MB each), 16 host CPUs")
    warm = torch.utils.data.DataLoader(_Decoded(2, frames, [256, 384], True, "host"), batch_size=1, collate_fn=lambda b: b[0])
    run_query_videos(warm, encoders, pca.transform, {}, dev, scorer=m["scorer"])      # first-use costs stay out of the timed runs
    for resize in ("host", "hip"):
        data = _Decoded(n_videos, frames, [256, 384], True, resize)
        loader = torch.utils.data.DataLoader(data, batch_size=1, shuffle=False, num_workers=6, collate_fn=lambda b: b[0], prefetch_factor=4)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_query_videos(loader, encoders, pca.transform, {}, dev, scorer=m["scorer"], resize=resize)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"  query ensemble  resize={resize:4s} {total / dt:8.1f} frames/s ({dt:.2f} s)" +
              (f"  {total * frames[0].nbytes / dt / 1e9:.2f} GB/s of decoded frames through the loader and the upload" if resize == "hip" else ""))
    # the loader alone: the decoded frames from 6 workers to this process, nothing done with them
    loader = torch.utils.data.DataLoader(_Decoded(n_videos, frames, [256, 384], True, "hip"), batch_size=1, shuffle=False, num_workers=6,
                                         collate_fn=lambda b: b[0], prefetch_factor=4)
    t0 = time.perf_counter()
    got = sum(len(v[2]) for v in loader)
    dt = time.perf_counter() - t0
    print(f"  loader alone, resize=hip (decoded frames cross from the workers to the main process): {got / dt:8.1f} frames/s = "
          f"{got * frames[0].nbytes / dt / 1e9:.2f} GB/s")
    # ... and the first read of every received video: its copy into a pinned buffer, which is what HipResize.upload does first
    from src.query_pipeline import RAW_KEY
    pinned = torch.empty(frames.size, dtype=torch.uint8).pin_memory()
    loader = torch.utils.data.DataLoader(_Decoded(n_videos, frames, [256, 384], True, "hip"), batch_size=1, shuffle=False, num_workers=6,
                                         collate_fn=lambda b: b[0], prefetch_factor=4)
    spent, t_all = [], time.perf_counter()
    for v in loader:
        t0 = time.perf_counter()
        pinned.view(v[1][RAW_KEY].shape).copy_(v[1][RAW_KEY])
        spent.append(time.perf_counter() - t0)
    t_all = time.perf_counter() - t_all
    print(f"  loader + first read of each received video into pinned memory: {total / t_all:8.1f} frames/s; the copy alone "
          f"{statistics.median(spent) * 1e3:.1f} ms per video (median; max {max(spent) * 1e3:.1f}) = {frames.nbytes / statistics.median(spent) / 1e9:.2f} GB/s")
    # the upload alone: one video through HipResize's pinned buffer, no kernels behind it
    rz = HipResize(dev)
    raw = torch.from_numpy(frames)
    with torch.cuda.stream(rz.stream):
        rz.upload(raw)
        rz.stream.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            rz.upload(raw)
        rz.stream.synchronize()
    dt = (time.perf_counter() - t0) / 5
    print(f"  upload alone (pageable -> pinned memcpy on one thread, then the copy): {dt * 1e3:.1f} ms per video = {raw.numel() / dt / 1e9:.2f} GB/s "
          f"= {40 / dt:.0f} frames/s per uploading thread")
    swin = m["swins"][0]
    for resize in ("host", "hip"):
        data = _Decoded(n_videos, frames, [256], False, resize, ref_size=256)
        loader = torch.utils.data.DataLoader(data, batch_size=2, num_workers=4, collate_fn=raw_collate if resize == "hip" else collate_fn)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if resize == "hip":
            extract_vsc_feat_raw(swin, loader, dev, 256, HipResize(dev))
        else:
            extract_vsc_feat(swin, loader, dev)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"  reference loop (Swin-V2-B/256, 4 workers)  resize={resize:4s} {total / dt:8.1f} frames/s ({dt:.2f} s)")


if __name__ == "__main__":
    from vsc_hip import _lib
    _lib.require_device()
    dev = torch.device("cuda:0")
    both = "--kernel" not in sys.argv and "--e2e" not in sys.argv
    if both or "--kernel" in sys.argv:
        kernel_bench(dev)
    if both or "--e2e" in sys.argv:
        n = int(sys.argv[sys.argv.index("--videos") + 1]) if "--videos" in sys.argv else 24
        e2e_bench(dev, n)
