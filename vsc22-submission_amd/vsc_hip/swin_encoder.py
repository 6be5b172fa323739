"""``SwinHipEncoder``: stands where the reference puts the swinv2_v1xx TorchScript backbones
(``torch.jit.load(...)`` / ``model(flat_frames)``: infer/extract_ref_feats.py:24-27,
infer/src/extractor.py:23).  Weights are given under the reference's own state-dict names
(train/train_v115/torch2scripts.py:677-684: ``module.backbone.`` prefix stripped)."""
from __future__ import annotations

import ctypes
import re

import numpy as np
import torch

from . import _lib
from ._lib import SwinConfigC
from ._model import HipModel
from .config import aligned_batch
from .swin_config import SwinConfig, get_swin_config


def swin_weight_names(cfg: SwinConfig) -> list:
    names = ["patch_embed.proj.weight", "patch_embed.proj.bias", "patch_embed.norm.weight", "patch_embed.norm.bias"]
    for s in range(cfg.stages):
        for b in range(cfg.depths[s]):
            p = f"layers.{s}.blocks.{b}."
            names += [p + n for n in (
                "attn.qkv.weight", "attn.q_bias", "attn.v_bias", "attn.logit_scale", "attn.cpb_mlp.0.weight",
                "attn.cpb_mlp.0.bias", "attn.cpb_mlp.2.weight", "attn.proj.weight", "attn.proj.bias",
                "norm1.weight", "norm1.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias",
                "norm2.weight", "norm2.bias")]
        if s + 1 < cfg.stages:
            p = f"layers.{s}.downsample."
            names += [p + "reduction.weight", p + "norm.weight", p + "norm.bias"]
    return names + ["norm.weight", "norm.bias", "output_proj.weight", "output_proj.bias"]


def from_reference_state(state: dict) -> dict:
    """Strip ``module.`` / ``backbone.`` prefixes (torch2scripts.py:679-683); buffers are ignored."""
    out = {}
    for k, v in state.items():
        k = re.sub(r"^(module\.)?(backbone\.)?", "", k)
        out[k] = v.detach().cpu().float().numpy() if isinstance(v, torch.Tensor) else np.asarray(v, np.float32)
    return out


class SwinHipEncoder(HipModel):
    PREFIX = "vsc_swin"

    def __init__(self, cfg: SwinConfig | str, weights: dict, *, max_batch: int = 32, l2_normalize: bool = False,
                 u8_mean=(0.5, 0.5, 0.5), u8_std=(0.5, 0.5, 0.5), precision: str = "bf16"):
        if isinstance(cfg, str):
            cfg = get_swin_config(cfg)
        super().__init__(cfg, max_batch, precision, u8_mean, u8_std)
        names = swin_weight_names(cfg)
        missing = [n for n in names if n not in weights]
        if missing:
            raise KeyError(f"swin weights missing {len(missing)} tensors, e.g. {missing[:4]}")
        pad4 = lambda t: (ctypes.c_int32 * 4)(*(list(t) + [0] * (4 - len(t))))
        c = SwinConfigC(image_size=cfg.image_size, patch_size=cfg.patch_size, channels=cfg.channels,
                        embed_dim=cfg.embed_dim, stages=cfg.stages, depths=pad4(cfg.depths), heads=pad4(cfg.heads),
                        window_size=cfg.window_size, pretrained_window_sizes=pad4(cfg.pretrained_window_sizes),
                        mlp_ratio=cfg.mlp_ratio, out_dim=cfg.out_dim, ln_eps=cfg.ln_eps, gem_p=cfg.gem_p,
                        max_batch=max_batch, l2_normalize=int(l2_normalize))
        self._load(c, names, weights)

    @property
    def _desc_dim(self) -> int:
        return self.cfg.out_dim

    @property
    def _token_shape(self) -> tuple:
        last = self.cfg.stages - 1
        return self.cfg.resolution(last) ** 2, self.cfg.dim(last)

    @property
    def preferred_batch(self) -> int:
        """Frames per call that fill whole rounds of GEMM tiles in the deepest stage (where most of the time goes:
        swinv2_base_256 has 16 x 16 = 256 tokens per frame there -> 256 frames), within max_batch."""
        deepest = max(range(self.cfg.stages), key=lambda s: self.cfg.depths[s])
        return min(self.max_batch, aligned_batch(self.cfg.resolution(deepest) ** 2))

    @property
    def preferred_call(self) -> int:
        """Frames per CALL that keep both lanes busy (the chunks of a call alternate over the encoder's two lanes)."""
        return 2 * self.preferred_batch

    def profile(self) -> dict:
        """{class name: (ms, launches)} accumulated since profiling was switched on; stage classes are "s<stage>.<kind>"."""
        ms, cnt = self._get_profile(_lib.SWIN_PROF_CLASSES)
        names = ["patchify", "patch_embed", "pool_head"]
        for s in range(4):
            names += [f"s{s}.{k}" for k in _lib.SWIN_PROF_KINDS]
        return {n: (float(ms[i]), int(cnt[i])) for i, n in enumerate(names) if cnt[i]}
