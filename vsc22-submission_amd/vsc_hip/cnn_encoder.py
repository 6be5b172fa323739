"""``CnnHipEncoder``: stands where the VSC22 baseline puts its TorchScript SSCD ResNet-50 (infer/vsc/baseline/inference_impl.py:
``model(img)``).  Weights are the folded tensors of ``weights.from_sscd_torchvision``.  Unlike the ViT / Swin encoders the input
size is free: frames are [n, 3, H, W] float32 (already normalised) or [n, H, W, 3] uint8 of any H, W >= 1."""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import CnnEncoderConfigC, check, current_stream, ptr
from ._model import HipModel
from .cnn_config import IMAGENET_MEAN, IMAGENET_STD, CnnConfig, cnn_weight_names, get_cnn_config


class CnnHipEncoder(HipModel):
    PREFIX = "vsc_cnn_encoder"

    def __init__(self, cfg: CnnConfig | str, weights: dict, *, max_pixels: int = 64 * 320 * 320, l2_normalize: bool = True,
                 u8_mean=IMAGENET_MEAN, u8_std=IMAGENET_STD, precision: str = "bf16"):
        """max_pixels: the largest n * H * W of one launch sequence; longer calls are split into chunks of whole frames.
        l2_normalize = False gives the adapted model's un-normalised projection (adapt_sscd_model.py)."""
        if isinstance(cfg, str):
            cfg = get_cnn_config(cfg)
        super().__init__(cfg, 0, precision, u8_mean, u8_std)
        self.max_pixels = int(max_pixels)
        names = cnn_weight_names(cfg)
        missing = [n for n in names if n not in weights]
        if missing:
            raise KeyError(f"cnn weights missing {len(missing)} tensors, e.g. {missing[:4]}")
        i4 = lambda t: (ctypes.c_int32 * 4)(*t)
        c = CnnEncoderConfigC(stem_width=cfg.stem_width, widths=i4(cfg.widths), depths=i4(cfg.depths), head_in=cfg.widths[3],
                              head_out=cfg.out_dim, gem_p=cfg.gem_p, l2=int(l2_normalize),
                              max_pixels=self.max_pixels)
        self._load(c, names, weights)

    @property
    def _desc_dim(self) -> int:
        return self.cfg.out_dim

    def __call__(self, frames: torch.Tensor):
        assert self._h is not None, "encoder was closed"
        u8 = frames.dtype == torch.uint8
        ok = frames.dim() == 4 and (frames.shape[3] if u8 else frames.shape[1]) == 3 and min(frames.shape[1:]) >= 1
        if not ok:
            raise ValueError(f"expected frames [n,3,H,W] float32 or [n,H,W,3] uint8, got {tuple(frames.shape)} {frames.dtype}")
        if not frames.is_cuda:
            raise _lib.HipPathUnavailable("frames must be on the GPU; there is no CPU path")
        frames = frames.contiguous() if u8 else frames.to(torch.float32).contiguous()
        n = frames.shape[0]
        h, w = (frames.shape[1], frames.shape[2]) if u8 else (frames.shape[2], frames.shape[3])
        if h * w > self.max_pixels:
            raise ValueError(f"one {h} x {w} frame is above max_pixels {self.max_pixels}")
        desc = torch.empty((n, self._desc_dim), dtype=torch.float32, device=frames.device)
        step = max(1, self.max_pixels // (h * w))
        for i in range(0, n, step):
            m = min(step, n - i)
            if u8:
                check(self._fn("forward_u8")(current_stream(), self._h, ptr(frames[i:i + m]), m, h, w, self.u8_mean, self.u8_std,
                                             ptr(desc[i:i + m])))
            else:
                check(self._fn("forward")(current_stream(), self._h, ptr(frames[i:i + m]), m, h, w, ptr(desc[i:i + m])))
        return desc

    def profile(self) -> dict:
        """{class name: (ms, launches)} accumulated since profiling was switched on"""
        ms, cnt = self._get_profile(len(_lib.CNN_PROF_CLASSES))
        return {n: (float(ms[i]), int(cnt[i])) for i, n in enumerate(_lib.CNN_PROF_CLASSES) if cnt[i]}
