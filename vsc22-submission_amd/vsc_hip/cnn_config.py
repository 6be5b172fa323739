"""CNN descriptor-backbone configurations: the VSC22 baseline's SSCD ResNet-50 (infer/vsc/baseline: torchvision's ResNet-50 v1.5
without ``fc``, GeM(p = 3) over the last map, Linear 2048 -> 512, L2) and a parity-test size of the same block structure."""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Tuple

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


@dataclass(frozen=True)
class CnnConfig:
    name: str = "sscd_resnet50"
    channels: int = 3
    stem_width: int = 64
    widths: Tuple[int, ...] = (256, 512, 1024, 2048)      # stage outputs; a block's bottleneck width is a quarter
    depths: Tuple[int, ...] = (3, 4, 6, 3)
    out_dim: int = 512
    gem_p: float = 3.0
    bn_eps: float = 1e-5

    @property
    def desc_dim(self) -> int:
        return self.out_dim

    def block_io(self, stage: int, block: int):
        """(cin, mid, cout, stride) of a bottleneck block; v1.5: the stride sits on the 3 x 3 convolution"""
        cin = self.widths[stage] if block else (self.widths[stage - 1] if stage else self.stem_width)
        return cin, self.widths[stage] // 4, self.widths[stage], 2 if (block == 0 and stage > 0) else 1

    def layer_table(self, h: int, w: int) -> list:
        """[(name, positions, K, cout)] of every convolution and the head for one h x w frame: the FLOP count's source"""
        half = lambda v: (v - 1) // 2 + 1
        h, w = half(h), half(w)
        rows = [("conv1", h * w, 147, self.stem_width)]
        h, w = half(h), half(w)
        for s in range(4):
            for b in range(self.depths[s]):
                cin, mid, cout, stride = self.block_io(s, b)
                ho, wo = (half(h), half(w)) if stride == 2 else (h, w)
                p = f"layer{s + 1}.{b}."
                rows += [(p + "conv1", h * w, cin, mid), (p + "conv2", ho * wo, 9 * mid, mid), (p + "conv3", ho * wo, mid, cout)]
                if b == 0:
                    rows.append((p + "downsample", ho * wo, cin, cout))
                h, w = ho, wo
        return rows + [("head", 1, self.widths[3], self.out_dim)]

    def flops_per_frame(self, h: int, w: int) -> int:
        return sum(2 * p * k * n for _, p, k, n in self.layer_table(h, w))


CNN_PRESETS = {
    "sscd_resnet50": CnnConfig(),
    # parity-test size: the same block structure, every channel count a multiple of 64
    "cnn_tiny": CnnConfig(name="cnn_tiny", widths=(256, 256, 512, 512), depths=(2, 1, 1, 1), out_dim=128),
}


def get_cnn_config(name: str, **overrides) -> CnnConfig:
    cfg = CNN_PRESETS[name]
    return replace(cfg, **overrides) if overrides else cfg


def cnn_weight_names(cfg: CnnConfig) -> list:
    """the folded tensors the C handle expects (csrc/cnn_encoder.hip)"""
    names = ["conv1.weight", "conv1.bias"]
    for s in range(4):
        for b in range(cfg.depths[s]):
            p = f"layer{s + 1}.{b}."
            for conv in ("conv1", "conv2", "conv3") + (("downsample",) if b == 0 else ()):
                names += [p + conv + ".weight", p + conv + ".bias"]
    return names + ["head.weight", "head.bias"]
