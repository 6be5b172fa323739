"""Progressive JPEG frames decoded on the device, measured (run on the GPU box; DESIGN.md 4.19 quotes the output):
      python tools/micro/jpeg_scans.py > profiles/jpeg_scans_bench.txt
Input: the synthetic 720p frames of tools/micro/jpeg_decode_bench.py (eight distinct frames, repeated to fill a call), written by
Pillow at quality 75 in 4:2:0 twice: progressive (Pillow's default script: ten scans) and baseline.
(a) Pillow's decode of the progressive files in six worker processes (before the GPU is opened: the workers are forked).
(b) one vsc_jpeg_decode_scans_u8 call of 40 and of 1 024 progressive frames against one vsc_jpeg_decode_u8 call on the same images
    saved as baseline -- one wave per frame in both: the yardstick, because the scan count multiplies the same chain.  Device
    events around every call, two warm-up calls, the calls interleaved round by round, the median of ROUNDS rounds.  The output of
    both is asserted equal to Pillow's.
(c) the per-scan split of the 40-frame call: the scan launch alone (VSC_JPEG_STAGES) over the first k scans of every frame,
    k = 1 .. 10, the median of ROUNDS rounds each; scan k costs the difference of k and k - 1.  The IDCT and the colour launch alone."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (os.path.join(ROOT, "vsc22-submission_amd"), ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np
import torch

import jpeg_decode_bench as single

ROUNDS = 5
H, W, Q = 720, 1280, 75


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def bench(dev):
    from vsc_hip import _lib, jpeg, ops
    prog, pil = single.jpg_files(H, W, Q, progressive=True)
    base, pil_base = single.jpg_files(H, W, Q)
    assert all(np.array_equal(a, b) for a, b in zip(pil, pil_base)), "the progressive files do not hold the baseline files' pixels"
    want = torch.from_numpy(np.stack(pil)).to(dev)
    n_distinct = len(prog)
    script = [(s.comps, s.ss, s.se, s.ah, s.al) for s in jpeg.parse_scans(prog[0]).scans]
    print(f"(b) 720p q{Q} 4:2:0, {n_distinct} distinct frames repeated; progressive {sum(map(len, prog)) / n_distinct / 1e3:.1f} kB, baseline {sum(map(len, base)) / n_distinct / 1e3:.1f} kB a frame; "
          f"median of {ROUNDS} interleaved rounds, device events")
    for n in (40, 1024):
        out_len = n * H * W * 3
        outs = [i * H * W * 3 for i in range(n)]
        data, offsets, records = jpeg.pack_scans([prog[i % n_distinct] for i in range(n)])
        assert all(isinstance(r, jpeg.ScanFrame) for r in records)
        wide = jpeg.ScanTableSets()
        rows, srows, sptr = jpeg.scan_rows(records, offsets[:-1].tolist(), outs, wide)
        bdata, boffsets, brecords = jpeg.pack([base[i % n_distinct] for i in range(n)])
        sets = jpeg.TableSets()
        brows = jpeg.frame_rows(brecords, boffsets[:-1].tolist(), outs, sets)
        dd, bd = torch.from_numpy(data).to(dev), torch.from_numpy(bdata).to(dev)
        out = torch.empty(out_len, dtype=torch.uint8, device=dev)
        frames = out.view(n, H, W, 3)
        calls = {"progressive, vsc_jpeg_decode_scans_u8": lambda: ops.jpeg_decode(dd, rows, wide.array(), out_len, out=out, scans=(srows, sptr)),
                 "baseline,    vsc_jpeg_decode_u8      ": lambda: ops.jpeg_decode(bd, brows, sets.array(), out_len, out=out)}
        for k, fn in calls.items():                              # first use, warm-up and the check of both
            fn()
            out.fill_(0)
            _, status = fn()
            assert int(status.abs().sum()) == 0 and all(torch.equal(frames[i], want[i % n_distinct]) for i in range(n)), f"{k}: the output is not Pillow's"
        times = {k: [] for k in calls}
        for _ in range(ROUNDS):
            for k, fn in calls.items():
                times[k].append(timed(fn))
        ref = statistics.median(times["baseline,    vsc_jpeg_decode_u8      "])
        for k in calls:
            ms = statistics.median(times[k])
            print(f"  {n:5d} frames  {k}  {ms:10.3f} ms (min {min(times[k]):.3f}, max {max(times[k]):.3f})  {n / ms * 1e3:9.1f} frames/s  x{ms / ref:5.2f} of the baseline call")
        sys.stdout.flush()
        if n == 40:
            print(f"(c) the 40-frame call by launch and by scan (scan launch over the first k scans, median of {ROUNDS}); script {script}")
            fn = calls["progressive, vsc_jpeg_decode_scans_u8"]
            last = 0.0
            for k in range(1, len(script) + 1):
                _lib.set_option("VSC_JPEG_STAGES", 1 | k << 8)
                fn()
                ms = statistics.median(timed(fn) for _ in range(ROUNDS))
                print(f"  scans 1 .. {k:2d}: {ms:9.3f} ms   scan {k:2d} {script[k - 1]}: {ms - last:9.3f} ms")
                last = ms
            for name, stages in (("IDCT launch", 4), ("colour launch", 2)):
                _lib.set_option("VSC_JPEG_STAGES", stages)
                fn()
                print(f"  {name}: {statistics.median(timed(fn) for _ in range(ROUNDS)):9.3f} ms")
            _lib.set_option("VSC_JPEG_STAGES", None)
            fn()
            sys.stdout.flush()
        del dd, bd, out, frames


def pillow_six():
    import multiprocessing as mp
    import time
    files, _ = single.jpg_files(H, W, Q, progressive=True)
    work = files * 10
    with mp.get_context("fork").Pool(6) as pool:
        pool.map(single._decode_all, [files] * 6)
        t0 = time.perf_counter()
        pool.map(single._decode_all, [work] * 6)
        six = 6 * len(work) / (time.perf_counter() - t0)
    print(f"(a) Pillow, progressive 720p q{Q} 4:2:0, six worker processes: {six:8.1f} frames/s = {40 / six * 1e3:8.1f} ms per 40 frames, {1024 / six * 1e3:9.1f} ms per 1 024")
    sys.stdout.flush()


if __name__ == "__main__":
    pillow_six()
    from vsc_hip import _lib
    _lib.require_device()
    bench(torch.device("cuda:0"))
