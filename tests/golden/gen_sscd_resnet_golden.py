"""Golden vectors for the CNN descriptor backbone (build container only; executes reference definitions, hence opt-in):

    VSC_RUN_REFERENCE_CODE=1 python tests/golden/gen_sscd_resnet_golden.py            # writes tests/golden/cnn_<preset>.npz
    VSC_RUN_REFERENCE_CODE=1 python tests/golden/gen_sscd_resnet_golden.py --check    # regenerates and compares with the committed files

The VSC22 baseline's descriptor model is the SSCD ResNet-50 (infer/vsc/baseline/adapt_sscd_model.py adapts
sscd_disc_mixup.torchvision.pt): torchvision's ResNet-50 v1.5 without ``fc``, then the reference's GlobalGeMPool2d(3.), Linear and
L2Norm.  Neither torchvision nor the checkpoint is on this image, so the BACKBONE is transformers.ResNetModel configured as that very
network (bottleneck layers, the stride on the 3 x 3: downsample_in_bottleneck=False) and the HEAD is the reference's own classes,
instantiated from their source through _reference_classes.py (train/train_v106/.../backbones/sscd.py:10-47, pinned by SHA-256
below).  Weights are tools/synth.resnet_weights, inputs tools/synth.frames_u8 normalised with ImageNet's mean / std.  The generator
asserts that tests/sscd_resnet_contract.py (which the GPU tests compare against) equals this chain to fp32 round-off, and that the
activation RMS of every stage lies within [0.1, 10].  No weights are stored: seeds, sizes, descriptors (raw and L2) and small
slices of the stage outputs.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "vsc22-submission_amd"), os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from tools import synth  # noqa: E402
from vsc_hip import weights as W  # noqa: E402
from vsc_hip.cnn_config import IMAGENET_MEAN, IMAGENET_STD, get_cnn_config  # noqa: E402

HEAD_SRC = "VSC22-Descriptor-Track-1st/train/train_v106/vsc/baseline/model_factory/backbones/sscd.py"
HEAD_SHA256 = "0bf451cc923161393269c5bae7606383b3ad8eed43450eb694dcd40d0d60639e"
# (preset, frames, H, W, weight seed, frame seed)
CASES = {
    "cnn_tiny": [(3, 64, 64, 41, 43), (2, 72, 88, 41, 47)],
    "sscd_resnet50": [(2, 96, 128, 53, 59), (2, 288, 512, 53, 61), (2, 96, 128, 67, 59)],
}
ROUND_OFF = 2e-6      # contract vs HF + reference head, on L2 descriptors (|d| <= 1) and relative on the raw ones
SLICE = (slice(None), slice(0, 8), slice(0, 2), slice(0, 3))


def to_hf_state(state: dict, cfg) -> dict:
    """torchvision names -> transformers.ResNetModel names (backbone only)"""
    out = {}

    def put(conv, bn, dst):
        out[dst + ".convolution.weight"] = torch.from_numpy(state[conv + ".weight"])
        for k in ("weight", "bias", "running_mean", "running_var"):
            out[f"{dst}.normalization.{k}"] = torch.from_numpy(state[f"{bn}.{k}"])
        out[dst + ".normalization.num_batches_tracked"] = torch.tensor(0)

    put("backbone.conv1", "backbone.bn1", "embedder.embedder")
    for s in range(4):
        for b in range(cfg.depths[s]):
            src, dst = f"backbone.layer{s + 1}.{b}.", f"encoder.stages.{s}.layers.{b}."
            for k in (1, 2, 3):
                put(f"{src}conv{k}", f"{src}bn{k}", f"{dst}layer.{k - 1}")
            if b == 0:
                put(src + "downsample.0", src + "downsample.1", dst + "shortcut")
    return out


def reference_chain(state: dict, cfg, x: torch.Tensor):
    """HF ResNetModel backbone + the reference's GlobalGeMPool2d / Linear / L2Norm -> (raw, l2, last map)"""
    from transformers import ResNetConfig, ResNetModel
    import _reference_classes as R
    R._PINNED.setdefault(HEAD_SRC, HEAD_SHA256)     # this generator's own pin (the loader refuses any other content)
    ns = R.load_definitions(HEAD_SRC)
    hf = ResNetModel(ResNetConfig(layer_type="bottleneck", downsample_in_bottleneck=False, hidden_sizes=list(cfg.widths),
                                  depths=list(cfg.depths), embedding_size=cfg.stem_width)).eval()
    missing, unexpected = hf.load_state_dict(to_hf_state(state, cfg), strict=True)
    assert not missing and not unexpected
    linear = torch.nn.Linear(cfg.widths[3], cfg.out_dim)
    linear.load_state_dict({"weight": torch.from_numpy(state["embeddings.1.weight"]), "bias": torch.from_numpy(state["embeddings.1.bias"])})
    with torch.no_grad():
        fmap = hf(x).last_hidden_state
        raw = linear(ns["GlobalGeMPool2d"](cfg.gem_p)(fmap))
        return raw, ns["L2Norm"]()(raw), fmap


def build(preset: str) -> dict:
    import sscd_resnet_contract as C
    cfg = get_cnn_config(preset)
    out = {"n_cases": np.int64(len(CASES[preset]))}
    for i, (n, h, w, wseed, fseed) in enumerate(CASES[preset]):
        state = synth.resnet_weights(wseed, cfg)
        x = C.normalize_u8(synth.frames_u8(fseed, n, h, w), IMAGENET_MEAN, IMAGENET_STD)
        raw_ref, l2_ref, fmap = reference_chain(state, cfg, x)
        raw, l2, stages = C.forward(W.from_sscd_torchvision(state, cfg), cfg, x, return_stages=True)
        e_l2 = float((l2 - l2_ref).abs().max())
        e_raw = float((raw - raw_ref).abs().max() / raw_ref.abs().max())
        e_map = float((stages["layer4"] - fmap).abs().max() / fmap.abs().max())
        assert e_l2 <= ROUND_OFF and e_raw <= ROUND_OFF and e_map <= 1e-5, (preset, i, e_l2, e_raw, e_map)
        rms = {k: float(v.pow(2).mean().sqrt()) for k, v in stages.items()}
        assert all(0.1 <= r <= 10.0 for r in rms.values()), (preset, i, rms)
        out[f"c{i}_meta"] = np.array([n, h, w, wseed, fseed], dtype=np.int64)
        out[f"c{i}_desc"] = raw_ref.numpy()
        out[f"c{i}_desc_l2"] = l2_ref.numpy()
        for k, v in stages.items():
            out[f"c{i}_{k}"] = v[SLICE].numpy().copy()
        print(f"{preset} case {i} {n} x {h} x {w}: contract vs HF + reference head: l2 {e_l2:.2e}, raw {e_raw:.2e} (rel), map {e_map:.2e} (rel); "
              f"stage RMS {' '.join(f'{k} {r:.2f}' for k, r in rms.items())}")
    return out


def main(check: bool) -> None:
    for preset in CASES:
        path = os.path.join(HERE, f"cnn_{preset}.npz")
        data = build(preset)
        if check:
            have = np.load(path)
            assert sorted(have.files) == sorted(data), (sorted(have.files), sorted(data))
            worst = max(float(np.abs(have[k].astype(np.float64) - np.asarray(data[k], dtype=np.float64)).max()) for k in data)
            assert worst <= ROUND_OFF, f"{path} differs from a fresh run by {worst}"
            print(f"{path}: matches a fresh run (max |d| {worst:.1e})")
        else:
            np.savez_compressed(path, **data)
            print(f"{path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main("--check" in sys.argv[1:])
