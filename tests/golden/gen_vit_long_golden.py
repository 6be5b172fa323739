"""Generate the golden vectors of the encoder presets with more than 320 tokens (run in the build container, NOT on the GPU box).

    python tests/golden/gen_vit_long_golden.py

The same generators as gen_vit_golden.py -- transformers' ViTModel / CLIPVisionModel on the deterministic weights and frames of
tools/synth.py -- called with the long presets: tiny_long (image 384, 577 tokens) and tiny_clip_long (image 320, 401 tokens).  The
files hold what vit_<preset>.npz of the short presets hold (descriptors, pooled features, the first four and the last two tokens),
a few KiB each: tests/golden/vit_tiny_long.npz, tests/golden/vit_tiny_clip_long.npz.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, ROOT, os.path.join(ROOT, "vsc22-submission_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gen_vit_golden import gen_clip, gen_vit  # noqa: E402

if __name__ == "__main__":
    torch.set_num_threads(8)
    gen_vit("tiny_long", 3)
    gen_clip("tiny_clip_long", 3)
