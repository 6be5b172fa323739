"""JPEG frame decoding on the device, measured (run on the GPU box; DESIGN.md 4.19 quotes the output):
      python tools/micro/jpeg_decode_bench.py [--kernel] [--pillow] [--e2e] [--videos N] > profiles/jpeg_decode_bench.txt
      python tools/micro/jpeg_decode_bench.py --split > profiles/jpeg_split_bench.txt
Input: synthetic frames (tools/synth.py: structured_frames, eight distinct frames per setting, repeated to fill a call) at 720p and
360p, encoded by Pillow at quality 75 and 90 in 4:2:0.
(a) --kernel: one vsc_jpeg_decode_u8 call of 40, 256 and 1024 frames.  Device events around every call, the same input for every
    launch, the variants -- the whole call, its scan + IDCT launch alone, its upsample + colour launch alone (VSC_JPEG_STAGES) --
    interleaved round by round, the median of ROUNDS rounds.  The output of the timed call is asserted equal to Pillow's.
(b) --pillow: the yardstick, Pillow's decode of the same files (Image.open(...).convert("RGB") and the array, as the loader workers
    do) in one process and in six worker processes.
(c) --e2e: run_query_videos through the reference's ensemble (tools/ensemble_bench.py: synthetic weights) on 40-frame 720p videos
    whose jpg files are in memory, with 6 loader workers: decode and resize on the host, resize on the device, decode and resize on
    the device.
(d) --split: one vsc_jpeg_decode_split_u8 call of 40, 256 and 1024 frames on the files of (a) and on the same frames written with
    a restart marker behind every MCU row.  Sub-streams: sub_bytes over 512, 1024, 2048, 4096 and rounds over 1, 2, 3; restart
    markers: item_bytes over 1024, 4096, 16384.  Every round runs vsc_jpeg_decode_u8 (one wave per frame) and then every setting on
    the same input; device events, the median of ROUNDS rounds; every setting's output is asserted equal to Pillow's and its
    vsc_jpeg_decode_stats are printed.  Pillow in six worker processes on the same files comes first."""
import io
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (os.path.join(ROOT, "vsc22-submission_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np
import torch

ROUNDS = 9
DISTINCT = 8
SHAPES = (("720p", 720, 1280), ("360p", 360, 640))
QUALITIES = (75, 90)


def jpg_files(h, w, quality, n=DISTINCT, **save):
    """n distinct synthetic frames of h x w as jpg files (4:2:0; ``save``: further arguments of Pillow's encoder) and Pillow's
    decode of each"""
    from PIL import Image
    from tools import synth
    x = synth.structured_frames(h * 31 + quality, n, types.SimpleNamespace(image_size=w, channels=3))[:, :, :h]      # [n, 3, h, w] in [-1, 1)
    u8 = np.clip(np.round((x.transpose(0, 2, 3, 1) + 1.0) * 127.5), 0, 255).astype(np.uint8)
    files = []
    for f in u8:
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, "JPEG", quality=quality, subsampling=2, **save)
        files.append(buf.getvalue())
    return files, [np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files]


def kernel_bench(dev):
    from vsc_hip import _lib, jpeg, ops
    print(f"(a) one vsc_jpeg_decode_u8 call, median of {ROUNDS} interleaved rounds, device events; {DISTINCT} distinct frames repeated")
    for name, h, w in SHAPES:
        for q in QUALITIES:
            files, pil = jpg_files(h, w, q)
            want = torch.from_numpy(np.stack(pil)).to(dev)
            for n in (40, 256, 1024):
                data, offsets, records = jpeg.pack([files[i % DISTINCT] for i in range(n)])
                assert all(isinstance(r, jpeg.Frame) for r in records)
                sets = jpeg.TableSets()
                rows = jpeg.frame_rows(records, offsets[:-1].tolist(), [i * h * w * 3 for i in range(n)], sets)
                tables, out_len = sets.array(), n * h * w * 3
                dd = torch.from_numpy(data).to(dev)
                out = torch.empty(out_len, dtype=torch.uint8, device=dev)
                variants = {"whole call": None, "scan + IDCT": 1, "upsample + colour": 2}
                ops.jpeg_decode(dd, rows, tables, out_len, out=out)
                torch.cuda.synchronize()
                times = {k: [] for k in variants}
                for _ in range(ROUNDS):
                    for k, stages in variants.items():
                        _lib.set_option("VSC_JPEG_STAGES", stages)
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        _, status = ops.jpeg_decode(dd, rows, tables, out_len, out=out)
                        b.record()
                        b.synchronize()
                        times[k].append(a.elapsed_time(b))
                _lib.set_option("VSC_JPEG_STAGES", None)
                out.fill_(0)
                _, status = ops.jpeg_decode(dd, rows, tables, out_len, out=out)
                frames = out.view(n, h, w, 3)
                assert int(status.abs().sum()) == 0 and all(torch.equal(frames[i], want[i % DISTINCT]) for i in range(n)), "the output is not Pillow's"
                for k in variants:
                    ms = statistics.median(times[k])
                    print(f"  {name} q{q} {n:5d} frames ({len(data) / n / 1e3:6.1f} kB each) {k:18s} {ms:9.3f} ms (min {min(times[k]):.3f}, max {max(times[k]):.3f})  "
                          f"{n / ms * 1e3:9.1f} frames/s  {len(data) / ms / 1e6:7.3f} GB/s compressed  {out_len / ms / 1e6:8.2f} GB/s of RGB")
                del dd, out
            del want


def _decode_all(files):
    from PIL import Image
    return sum(int(np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))[0, 0, 0]) for f in files)


SPLIT_KINDS = (("no restart markers", {}), ("a marker every MCU row", {"restart_marker_rows": 1}))


def split_bench(dev):
    from vsc_hip import jpeg, ops
    print(f"(d) one vsc_jpeg_decode_split_u8 call against one vsc_jpeg_decode_u8 call on the same input, median of {ROUNDS} interleaved rounds, device events; "
          f"{DISTINCT} distinct frames repeated; statistics = (frames cut at markers, cut into sub-streams, wanted cut but one item, items launched)")
    for name, h, w in SHAPES:
        for q in QUALITIES:
            for kind, save in SPLIT_KINDS:
                files, pil = jpg_files(h, w, q, **save)
                want = torch.from_numpy(np.stack(pil)).to(dev)
                if save:
                    variants = {f"markers, item_bytes {ib:5d}": {"mode": "markers", "item_bytes": ib} for ib in (1024, 4096, 16384)}
                else:
                    variants = {f"sub-streams, sub_bytes {sb:4d}, rounds {r}": {"mode": "substreams", "sub_bytes": sb, "rounds": r}
                                for sb in (512, 1024, 2048, 4096) for r in (1, 2, 3)}
                for n in (40, 256, 1024):
                    chosen = [files[i % DISTINCT] for i in range(n)]
                    data, offsets, records = jpeg.pack(chosen)
                    sets = jpeg.TableSets()
                    rows = jpeg.frame_rows(records, offsets[:-1].tolist(), [i * h * w * 3 for i in range(n)], sets)
                    restarts = jpeg.restart_rows(chosen, records)
                    tables, out_len = sets.array(), n * h * w * 3
                    dd = torch.from_numpy(data).to(dev)
                    out = torch.empty(out_len, dtype=torch.uint8, device=dev)
                    frames = out.view(n, h, w, 3)
                    stats = {}
                    for k, split in variants.items():              # first use, and the check of every setting
                        out.fill_(0)
                        _, status = ops.jpeg_decode(dd, rows, tables, out_len, out=out, restarts=restarts, split=split)
                        stats[k] = ops.jpeg_decode_stats()
                        assert int(status.abs().sum()) == 0 and all(torch.equal(frames[i], want[i % DISTINCT]) for i in range(n)), f"{k}: the output is not Pillow's"
                    ops.jpeg_decode(dd, rows, tables, out_len, out=out)
                    torch.cuda.synchronize()
                    times = {k: [] for k in ["one wave per frame"] + list(variants)}
                    for _ in range(ROUNDS):
                        for k in times:
                            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            a.record()
                            if k in variants:
                                ops.jpeg_decode(dd, rows, tables, out_len, out=out, restarts=restarts, split=variants[k])
                            else:
                                ops.jpeg_decode(dd, rows, tables, out_len, out=out)
                            b.record()
                            b.synchronize()
                            times[k].append(a.elapsed_time(b))
                    base = statistics.median(times["one wave per frame"])
                    for k in times:
                        ms = statistics.median(times[k])
                        print(f"  {name} q{q} {kind}: {n:5d} frames ({len(data) / n / 1e3:6.1f} kB each) {k:38s} {ms:9.3f} ms (min {min(times[k]):.3f}, max {max(times[k]):.3f})  "
                              f"{n / ms * 1e3:9.1f} frames/s  x{base / ms:6.2f} of one wave per frame" + (f"  statistics {stats[k]}" if k in stats else ""))
                    sys.stdout.flush()
                    del dd, out, frames
                del want


def pillow_bench(kinds=(("", {}),)):
    import multiprocessing as mp
    print("(b) Pillow's decode of the same files on this box's CPUs (Image.open(...).convert('RGB') -> array)")
    for kind, save, name, h, w, q in [(kind, save, name, h, w, q) for kind, save in kinds for name, h, w in SHAPES for q in QUALITIES]:
        files, _ = jpg_files(h, w, q, **save)
        reps = 10 if h >= 720 else 40
        work = files * reps
        _decode_all(files)
        t0 = time.perf_counter()
        _decode_all(work)
        one = len(work) / (time.perf_counter() - t0)
        with mp.get_context("fork").Pool(6) as pool:
            pool.map(_decode_all, [files] * 6)
            t0 = time.perf_counter()
            pool.map(_decode_all, [work] * 6)
            six = 6 * len(work) / (time.perf_counter() - t0)
        print(f"  {name} q{q}{', ' + kind if kind else ''}: one process {one:8.1f} frames/s, six worker processes {six:8.1f} frames/s ({h * w * 3 * six / 1e9:.2f} GB/s of RGB)")


class _Zipped(torch.utils.data.Dataset):
    """videos whose jpg files are in memory: the worker decodes and resizes (host), only decodes (resize) or hands the files on (decode)"""

    def __init__(self, n_videos, files, sizes, mode):
        self.n, self.files, self.sizes, self.mode = n_videos, files, sizes, mode

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        from PIL import Image
        from src.dataset import bytes_video, clip_transform_u8, decode_rgb, vit_transform_u8
        from src.query_pipeline import RAW_KEY, VideoScorer
        vid, n = f"Q{i:06d}", len(self.files)
        stamps = np.stack([np.arange(n, dtype=np.float32), np.arange(n, dtype=np.float32) + 1.0], axis=1)
        if self.mode == "decode":
            return vid, {RAW_KEY: bytes_video(self.files)}, stamps
        images = [Image.open(io.BytesIO(f)).convert("RGB") for f in self.files]
        if self.mode == "resize":
            return vid, {RAW_KEY: torch.from_numpy(np.stack([decode_rgb(im) for im in images]))}, stamps
        out = {s: torch.stack([vit_transform_u8(s, s)(im) for im in images]) for s in self.sizes}
        out[VideoScorer.KEY] = torch.stack([clip_transform_u8(224)(im) for im in images])
        return vid, out, stamps


def e2e_bench(dev, n_videos):
    from src.query_pipeline import run_query_videos
    from src.query_postprocess import HipPCA
    from tools import ensemble_bench
    m = ensemble_bench.build(dev, "fp16")
    encoders = [(s, 256) for s in m["swins"]] + [(m["vit"], 384)]
    pca = HipPCA(ensemble_bench._Fitted)
    files, _ = jpg_files(720, 1280, 75)
    files = [files[i % DISTINCT] for i in range(40)]
    total = n_videos * 40
    print(f"(c) end to end, {n_videos} videos of 40 720p jpg files in memory ({sum(map(len, files)) / 1e6:.1f} MB compressed, {40 * 720 * 1280 * 3 / 1e6:.0f} MB decoded each), "
          "6 loader workers")
    warm = torch.utils.data.DataLoader(_Zipped(2, files, [256, 384], "host"), batch_size=1, collate_fn=lambda b: b[0])
    run_query_videos(warm, encoders, pca.transform, {}, dev, scorer=m["scorer"])      # first-use costs stay out of the timed runs
    for mode, kw in (("host", {}), ("resize", {"resize": "hip"}), ("decode", {"resize": "hip", "decode": "hip"})):
        loader = torch.utils.data.DataLoader(_Zipped(n_videos, files, [256, 384], mode), batch_size=1, shuffle=False, num_workers=6,
                                             collate_fn=lambda b: b[0], prefetch_factor=4)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_query_videos(loader, encoders, pca.transform, {}, dev, scorer=m["scorer"], **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        label = {"host": "decode host, resize host", "resize": "decode host, resize hip ", "decode": "decode hip,  resize hip "}[mode]
        print(f"  query ensemble  {label} {total / dt:8.1f} frames/s ({dt:.2f} s, {dt / n_videos:.2f} s per video)")


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--pillow", action="store_true")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--videos", type=int, default=12)
    args = ap.parse_args()
    if args.split:
        pillow_bench(SPLIT_KINDS)       # before the GPU is opened: the workers are forked
        sys.stdout.flush()
        from vsc_hip import _lib
        _lib.require_device()
        split_bench(torch.device("cuda:0"))
        sys.exit(0)
    everything = not (args.kernel or args.pillow or args.e2e)
    if args.pillow or everything:
        pillow_bench()              # before the GPU is opened: the workers are forked
        sys.stdout.flush()
    if args.kernel or args.e2e or everything:
        from vsc_hip import _lib
        _lib.require_device()
        dev = torch.device("cuda:0")
        if args.kernel or everything:
            kernel_bench(dev)
            sys.stdout.flush()
        if args.e2e or everything:
            e2e_bench(dev, args.videos)
