"""Throughput of the CNN encoder (sscd_resnet50) on the GPU, measured and recorded, not a gate:

    python tools/cnn_encoder_bench.py [--out profiles/cnn_encoder_bench.json] [--steps 10] [--skip_torch]

Per operand type (both libraries), size (320 x 320, 288 x 512) and frames per call (64, 256): frames/s from device events around
`steps` calls on the same resident uint8 input, after a warm-up of two calls; the model FLOP/s from the layer table's own count
(vsc_hip.cnn_config.CnnConfig.flops_per_frame) and its fraction of the 2.5 PF/s dense 16-bit peak -- a whole-model rate over
peak, not a kernel's share of it.  Yardstick: PyTorch-ROCm running transformers.ResNetModel with the same weights in fp16
channels_last on the same box (backbone only: it lacks GeM and the head, under 0.1 % of the FLOPs); if that does not run, the
reason is recorded instead."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vsc22-submission_amd"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tools import synth  # noqa: E402
from vsc_hip import weights as W  # noqa: E402
from vsc_hip.cnn_config import IMAGENET_MEAN, IMAGENET_STD, get_cnn_config  # noqa: E402
from vsc_hip.cnn_encoder import CnnHipEncoder  # noqa: E402

PEAK_16BIT = 2.5e15
SIZES = ((320, 320), (288, 512))
CALLS = (64, 256)


def timed(fn, steps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cnn_encoder_bench.json"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip_torch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = get_cnn_config("sscd_resnet50")
    state = synth.resnet_weights(53, cfg)
    folded = W.from_sscd_torchvision(state, cfg)
    rows = []
    frames = {(h, w): torch.from_numpy(synth.frames_u8(7, 8, h, w)).to(dev).repeat(max(CALLS) // 8, 1, 1, 1).contiguous() for h, w in SIZES}
    for precision in ("bf16", "fp16"):
        enc = CnnHipEncoder(cfg, folded, precision=precision, max_pixels=max(CALLS) * max(h * w for h, w in SIZES))
        for h, w in SIZES:
            for n in CALLS:
                x = frames[(h, w)][:n]
                dt = timed(lambda: enc(x), args.steps)
                flops = cfg.flops_per_frame(h, w) * n / dt
                rows.append({"engine": "hip", "operands": precision, "h": h, "w": w, "frames_per_call": n, "ms_per_call": dt * 1e3,
                             "frames_per_s": n / dt, "model_tflops": flops / 1e12, "fraction_of_2.5PF": flops / PEAK_16BIT})
                print(rows[-1], flush=True)
        enc.close()
    if not args.skip_torch:
        try:
            from transformers import ResNetConfig, ResNetModel
            from gen_sscd_resnet_golden import to_hf_state
            hf = ResNetModel(ResNetConfig(layer_type="bottleneck", downsample_in_bottleneck=False, hidden_sizes=list(cfg.widths),
                                          depths=list(cfg.depths), embedding_size=cfg.stem_width)).eval()
            hf.load_state_dict(to_hf_state(state, cfg), strict=True)
            hf = hf.to(dev).half().to(memory_format=torch.channels_last)
            mean = torch.tensor(IMAGENET_MEAN, device=dev).view(1, 3, 1, 1)
            std = torch.tensor(IMAGENET_STD, device=dev).view(1, 3, 1, 1)
            for h, w in SIZES:
                for n in CALLS:
                    x = ((frames[(h, w)][:n].permute(0, 3, 1, 2).float() / 255.0 - mean) / std).half().contiguous(memory_format=torch.channels_last)
                    with torch.no_grad():
                        dt = timed(lambda: hf(x).last_hidden_state, args.steps)
                    flops = cfg.flops_per_frame(h, w) * n / dt
                    rows.append({"engine": "torch fp16 channels_last (backbone only, normalised input resident)", "h": h, "w": w,
                                 "frames_per_call": n, "ms_per_call": dt * 1e3, "frames_per_s": n / dt, "model_tflops": flops / 1e12,
                                 "fraction_of_2.5PF": flops / PEAK_16BIT})
                    print(rows[-1], flush=True)
        except Exception as exc:  # noqa: BLE001 -- recorded: the yardstick did not run here
            rows.append({"engine": "torch fp16 channels_last", "did_not_run": f"{type(exc).__name__}: {exc}"})
            print(rows[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"gflop_per_frame": {f"{h}x{w}": cfg.flops_per_frame(h, w) / 1e9 for h, w in SIZES}, "steps": args.steps, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
