"""Error figures of the CNN encoder against its fixtures, for tests/cnn_encoder_bounds.py (GPU):

    python tools/cnn_encoder_stats.py [--out stats.json]

Per operand type and fixture case: (max |d|, mean |d|, |mean d|) of the L2 descriptors, d = HIP - fixture; and, for
sscd_resnet50 case 0, the same with backbone.layer3.2.conv2.weight scaled by 1.01 (what the mean bound has to see)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vsc22-submission_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cnn_encoder_bounds as B  # noqa: E402
from tools import synth  # noqa: E402
from vsc_hip import weights as W  # noqa: E402
from vsc_hip.cnn_config import get_cnn_config  # noqa: E402
from vsc_hip.cnn_encoder import CnnHipEncoder  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    for preset in ("cnn_tiny", "sscd_resnet50"):
        fx = np.load(os.path.join(ROOT, "tests", "golden", f"cnn_{preset}.npz"))
        cfg = get_cnn_config(preset)
        states = {}
        for precision in ("bf16", "fp16"):
            for case in range(int(fx["n_cases"])):
                n, h, w, wseed, fseed = (int(v) for v in fx[f"c{case}_meta"])
                if wseed not in states:
                    states[wseed] = synth.resnet_weights(wseed, cfg)
                variants = [("", 1.0)] + ([("/layer3.2.conv2 x 1.01", 1.01)] if (preset, case) == ("sscd_resnet50", 0) else [])
                for tag, scale in variants:
                    state = dict(states[wseed])
                    if scale != 1.0:
                        state["backbone.layer3.2.conv2.weight"] = state["backbone.layer3.2.conv2.weight"] * np.float32(scale)
                    enc = CnnHipEncoder(cfg, W.from_sscd_torchvision(state, cfg), precision=precision, max_pixels=n * h * w)
                    got = enc(torch.from_numpy(synth.frames_u8(fseed, n, h, w)).to(dev)).cpu().numpy()
                    enc.close()
                    key = f"{precision}/{preset}/{case}{tag}"
                    out[key] = B.stats(got, fx[f"c{case}_desc_l2"])
                    print(f'    "{key}": ({out[key][0]:.3e}, {out[key][1]:.3e}, {out[key][2]:.3e}),', flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
