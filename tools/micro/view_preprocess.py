"""Query view preprocessing (--preprocess hip) on the GPU box: per-video cost of detection and resize, the CPU cost of the parts that
have a faithful CPU form, and run_query_videos with --preprocess none vs hip on plain videos through the reference's ensemble.

    python tools/micro/view_preprocess.py [--frames 40] [--videos 52] [--skip-ensemble] [--skip-kernels]

Detection = vsc_frame_var_u8 + vsc_canny_count_u8 (20 sampled frames) + one device -> host copy of both maps + the host decisions
(src/image_preprocess.detect_views); resize = vsc_resize_bicubic_u8 of one whole-frame view to 256 and to 384.  Kernel times come
from device events (median of 5 after a warm-up), detection's wall time from the host.  Canny's CPU cost under cv2 is not measured:
cv2 is not installed in this project's environments.

The decisions table (profiles/view_decide_bench.txt) compares ``detect_views`` with the decisions on the host and on the device
(vsc_view_decide_f64), alternating on plain and letterboxed videos, next to the device time of the decide launch alone; the
ensemble then runs with --preprocess none, hip with host decisions and hip with device decisions."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (os.path.join(ROOT, "vsc22-submission_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np
import torch

COPY_TBPS = 6.3   # measured device copy rate
RES = {"360p": (360, 640), "720p": (720, 1280), "1080p": (1080, 1920)}


def plain_frames(n, h, w, seed=0):
    """moving content without static borders or bands: a per-frame colour over a drifting gradient, a few dark rectangles"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    out = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        base = rng.integers(90, 200, 3).astype(np.float32)
        img = base + 40.0 * np.sin(xx / 97.0 + yy / 131.0 + i / 3.0)[:, :, None]
        for _ in range(4):
            y0, x0 = rng.integers(0, h - h // 6), rng.integers(0, w - w // 6)
            img[y0:y0 + h // 6, x0:x0 + w // 6] = rng.integers(0, 60)
        out[i] = np.clip(img, 0, 255).astype(np.uint8)
    return out


def letterbox_frames(n, h, w, seed=0):
    """plain_frames with a static black band of h / 8 lines above and below"""
    out = plain_frames(n, h, w, seed)
    out[:, :h // 8] = 16
    out[:, h - h // 8:] = 16
    return out


def decisions(n_frames):
    """detect_views per video with host and with device decisions, alternating, median of 5 wall times each; beside it the device
    time of the decide launch alone (maps already on the device)"""
    from src.image_preprocess import canny_frames, detect_views
    from vsc_hip import ops
    idx = canny_frames(n_frames)
    print(f"decisions: {n_frames}-frame videos, detect_views wall ms per video (median of 5, host and device decisions alternating), "
          f"the decide launch alone from device events (median of 5)", flush=True)
    rows = []
    for kind, make in (("plain", plain_frames), ("letterbox", letterbox_frames)):
        for name, (h, w) in RES.items():
            d = torch.from_numpy(make(n_frames, h, w)).cuda()
            want = detect_views(d)
            assert detect_views(d, decisions="hip") == want, (kind, name)
            torch.cuda.synchronize()
            walls = {"host": [], "hip": []}
            for _ in range(5):
                for mode in ("host", "hip"):
                    t0 = time.perf_counter()
                    detect_views(d, decisions=mode)
                    walls[mode].append((time.perf_counter() - t0) * 1e3)
            var, count = ops.view_maps_dev(d, idx)
            item = [(0, 0, h, w, len(idx), n_frames)]
            launch_ms = event_ms(lambda: ops.view_decide(var, count, item))
            maps_ms = event_ms(lambda: ops.view_maps_dev(d, idx))
            row = dict(kind=kind, res=name, views=len(want[1]), changed=want[0], host_wall_ms=float(np.median(walls["host"])),
                       hip_wall_ms=float(np.median(walls["hip"])), decide_launch_ms=launch_ms, maps_ms=maps_ms)
            row["hip_over_host"] = row["hip_wall_ms"] / row["host_wall_ms"]
            rows.append(row)
            print(" ".join(f"{k}={v:.3f}" if isinstance(v, float) else f"{k}={v}" for k, v in row.items()), flush=True)
    return rows


def event_ms(fn, reps=5):
    ts = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts[1:]))


def per_video(n_frames):
    from PIL import Image
    from src.image_preprocess import canny_frames, detect_views
    from vsc_hip import ops
    rows = []
    for name, (h, w) in RES.items():
        frames = plain_frames(n_frames, h, w)
        d = torch.from_numpy(frames).cuda()
        idx = canny_frames(n_frames)
        var_ms = event_ms(lambda: ops.frame_var(d))
        canny_ms = event_ms(lambda: ops.canny_count(d, idx))
        detect_views(d)
        torch.cuda.synchronize()
        walls = []
        for _ in range(5):
            t0 = time.perf_counter()
            changed, boxes = detect_views(d)
            walls.append((time.perf_counter() - t0) * 1e3)
        resize_ms = {s: event_ms(lambda s=s: ops.resize_bicubic(d, boxes, s)) for s in (256, 384)}
        in_bytes = frames.nbytes
        t0 = time.perf_counter()
        np.stack(list(frames)).var(axis=0).sum(-1)
        cpu_var = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        for f in frames:
            im = Image.fromarray(f)
            im.resize((256, 256), Image.BICUBIC)
            im.resize((384, 384), Image.BICUBIC)
        cpu_resize = (time.perf_counter() - t0) * 1e3
        row = dict(res=name, frames=n_frames, changed=changed, var_ms=var_ms, var_gbps=2 * in_bytes / var_ms / 1e6,
                   canny_ms=canny_ms, canny_gbps=len(idx) * h * w * 3 / canny_ms / 1e6, detect_wall_ms=float(np.median(walls)),
                   resize256_ms=resize_ms[256], resize384_ms=resize_ms[384],
                   resize_gbps=(in_bytes * 2 + n_frames * 3 * (256 ** 2 + 384 ** 2)) / (resize_ms[256] + resize_ms[384]) / 1e6,
                   cpu_var_ms=cpu_var, cpu_pil_resize_ms=cpu_resize)
        rows.append(row)
        print(" ".join(f"{k}={v:.3f}" if isinstance(v, float) else f"{k}={v}" for k, v in row.items()), flush=True)
    print(f"(GB/s against the {COPY_TBPS} TB/s copy rate; var counts both passes over the frames, canny the sampled frames once, "
          f"resize the crop's bytes read by each size's horizontal pass plus the views written)")
    return rows


def ensemble(n_videos, n_frames, res):
    """run_query_videos on plain videos, alternating --preprocess none (frames resized on the host beforehand, as the workers do),
    hip (full-resolution frames; upload, detection and resize inside run_query_videos) and hip with the decisions on the device"""
    from PIL import Image
    from src.dataset import clip_transform_u8, vit_transform_u8
    from src.image_preprocess import HipViews
    from src.query_pipeline import RAW_KEY, run_query_videos
    from src.query_postprocess import HipPCA
    from tools.ensemble_bench import _Fitted, build
    dev = torch.device("cuda", 0)
    m = build(dev, precision="fp16")
    encoders = [(s, 256) for s in m["swins"]] + [(m["vit"], 384)]
    pca = HipPCA(_Fitted)
    h, w = RES[res]
    base = plain_frames(8, h, w, seed=1)
    reps = (n_frames + 7) // 8
    raw = torch.from_numpy(np.concatenate([base] * reps)[:n_frames])
    pil = [Image.fromarray(f) for f in base]
    made = {s: torch.stack([vit_transform_u8(s, s)(im) for im in pil]) for s in (256, 384)}
    made["clip"] = torch.stack([clip_transform_u8(224)(im) for im in pil])
    made = {k: v.repeat(reps, 1, 1, 1)[:n_frames].clone() for k, v in made.items()}
    none_items = [(f"Q{v:06d}", dict(made), np.arange(n_frames)) for v in range(n_videos)]
    hip_items = [(f"Q{v:06d}", {RAW_KEY: raw, "clip": made["clip"]}, np.arange(n_frames)) for v in range(n_videos)]
    views = {"hip": HipViews(dev), "hip_device": HipViews(dev, decisions="hip")}
    rates = {"none": [], "hip": [], "hip_device": []}
    for rep in range(4):
        for mode in rates:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_query_videos(none_items if mode == "none" else hip_items, encoders, pca.transform, {}, dev, scorer=m["scorer"],
                             views=views.get(mode))
            torch.cuda.synchronize()
            if rep:
                rates[mode].append(n_videos * n_frames / (time.perf_counter() - t0))
    r = {k: float(np.median(v)) for k, v in rates.items()}
    print(f"ensemble {res}: {n_videos} x {n_frames} frames, none {r['none']:.0f} frames/s, hip {r['hip']:.0f} frames/s "
          f"(hip / none = {r['hip'] / r['none']:.3f}), hip with device decisions {r['hip_device']:.0f} frames/s "
          f"(/ none = {r['hip_device'] / r['none']:.3f}, / hip = {r['hip_device'] / r['hip']:.3f})", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--videos", type=int, default=52)
    ap.add_argument("--skip-ensemble", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true", help="only the decisions table and the ensemble")
    ap.add_argument("--ensemble-res", nargs="+", default=["360p", "720p"])
    args = ap.parse_args()
    from vsc_hip import _lib
    _lib.require_device()
    print(f"tools/micro/view_preprocess.py on {torch.cuda.get_device_name(0)}", flush=True)
    if not args.skip_kernels:
        per_video(args.frames)
    decisions(args.frames)
    if not args.skip_ensemble:
        for res in args.ensemble_res:
            ensemble(args.videos, args.frames, res)


if __name__ == "__main__":
    main()
