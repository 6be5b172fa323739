"""``HipEncoder``: the callable that stands where the reference puts its TorchScript
backbone -- ``model = torch.jit.load(...)``, ``flat_features = model(flat_frames)``
(infer/extract_ref_feats.py:24-27, infer/src/extractor.py:23,
infer/extract_query_feats.py:145-155).  Same call shape: frames [n,3,H,W] float32
on the GPU in, features [n, dim] float32 on the GPU out.
"""
from __future__ import annotations

from . import _lib, weights as wnames
from ._lib import EncoderConfigC
from ._model import HipModel
from .config import EncoderConfig, aligned_batch, get_config


class HipEncoder(HipModel):
    PREFIX = "vsc_encoder"

    def __init__(self, cfg: EncoderConfig | str, weights: dict, *, max_batch: int = 128,
                 l2_normalize: bool = False, lanes: int = 2, fuse_ln: int = 0,
                 u8_mean=(0.5, 0.5, 0.5), u8_std=(0.5, 0.5, 0.5), precision: str = "bf16"):
        """precision: the 16-bit type of the MFMA operands (weights and activations between the fp32 residual stream / LayerNorm /
        softmax): "bf16" (libvsc_hip.so, the benchmarked configuration) or "fp16" (libvsc_hip_f16.so: same kernels and speed, 8 x
        smaller rounding; what the infer/ entry points use)."""
        if isinstance(cfg, str):
            cfg = get_config(cfg)
        super().__init__(cfg, max_batch, precision, u8_mean, u8_std)
        self.lanes = lanes
        self.l2 = l2_normalize
        wnames.check_complete(weights, cfg)
        c = EncoderConfigC(
            image_size=cfg.image_size, patch_size=cfg.patch_size, channels=cfg.channels,
            width=cfg.width, layers=cfg.layers, heads=cfg.heads, mlp_dim=cfg.mlp_dim,
            out_dim=cfg.out_dim, ln_eps=cfg.ln_eps, act={"gelu": 0, "quick_gelu": 1}[cfg.act],
            pre_ln=int(cfg.pre_ln), patch_bias=int(cfg.patch_bias),
            pool={"gem": 0, "cls": 1}[cfg.pool], gem_p=cfg.gem_p, max_batch=max_batch,
            l2_normalize=int(l2_normalize), head_conv_dim=cfg.head_conv_dim, lanes=lanes, fuse_ln=int(fuse_ln))
        self._load(c, wnames.canonical_names(cfg), weights)

    @property
    def _desc_dim(self) -> int:
        return self.cfg.desc_dim

    @property
    def _token_shape(self) -> tuple:
        return self.cfg.tokens, self.cfg.width

    @property
    def preferred_batch(self) -> int:
        """Frames per call that fill whole rounds of GEMM tiles (config.aligned_batch), within max_batch."""
        return min(self.max_batch, aligned_batch(self.cfg.tokens))

    @property
    def preferred_call(self) -> int:
        """Frames per CALL that keep every lane busy: the chunks of a call alternate over the encoder's lanes (two by default), so a
        call of one chunk runs on one lane alone (ViT-B/16: 332 frames 25.4 k frames/s, 664 frames 25.7 k; Swin-V2-B 16.1 vs 17.0 k)."""
        return self.preferred_batch * max(int(self.lanes), 1)

    def get_profile(self) -> dict:
        """{class: (total_ms, launches)} accumulated since set_profiling(True)."""
        ms, cnt = self._get_profile(len(_lib.PROF_CLASSES))
        return {name: (ms[i], cnt[i]) for i, name in enumerate(_lib.PROF_CLASSES)}
