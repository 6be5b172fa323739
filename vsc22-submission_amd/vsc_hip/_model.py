"""``HipModel``: what the two frame encoders' host classes (``HipEncoder``, ``SwinHipEncoder``) share -- the handle's life cycle
over the C ABI (create -> set weights -> finalize, destroy), the call with its input checks, and the nn.Module-ish surface the
reference call sites use.  A subclass names its C functions by prefix, builds its config struct, lists its weight names and
gives the descriptor width and the debug-token shape."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, current_stream, ptr


class HipModel:
    PREFIX = ""         # "vsc_encoder" / "vsc_swin": the handle's functions are <PREFIX>_create, _set_weight, ...
    _h = None

    def __init__(self, cfg, max_batch: int, precision: str, u8_mean, u8_std):
        self.cfg, self.max_batch = cfg, max_batch
        # Normalize(mean, std) applied to uint8 [n,H,W,C] inputs inside the patchify kernel (vit_transform: 0.5 / 0.5)
        self.u8_mean = (ctypes.c_float * cfg.channels)(*u8_mean[: cfg.channels])
        self.u8_std = (ctypes.c_float * cfg.channels)(*u8_std[: cfg.channels])
        self.precision = precision      # 16-bit operand type: "bf16" | "fp16" (HipEncoder's docstring)
        self._lib = _lib.require_device(precision)

    def _fn(self, name: str):
        return getattr(self._lib, f"{self.PREFIX}_{name}")

    def _load(self, config_c, names, weights: dict) -> None:
        """create -> set every named weight -> finalize; the handle is destroyed again if any step fails"""
        handle = ctypes.c_void_p()
        check(self._fn("create")(ctypes.byref(config_c), ctypes.byref(handle)))
        self._h = handle
        try:
            for name in names:
                arr = weights[name]
                arr = arr.detach().cpu().numpy() if isinstance(arr, torch.Tensor) else arr
                arr = np.ascontiguousarray(arr, dtype=np.float32)
                check(self._fn("set_weight")(self._h, name.encode(), arr.ctypes.data_as(ctypes.c_void_p), arr.size))
            check(self._fn("finalize")(self._h))
        except Exception:
            self.close()
            raise

    # nn.Module-ish surface the reference call sites use
    def eval(self):
        return self

    def cuda(self, *_a, **_k):
        return self

    def to(self, *_a, **_k):
        return self

    @property
    def workspace_bytes(self) -> int:
        return int(self._fn("workspace_bytes")(self._h))

    def __call__(self, frames: torch.Tensor, return_tokens: bool = False):
        """frames: float32 [n,C,H,W] already normalised (the reference's tensors), or uint8 [n,H,W,C] decoded frames
        (ToTensor + Normalize(u8_mean, u8_std) then happen on the GPU; bit-identical descriptors, 4x fewer bytes)."""
        assert self._h is not None, "encoder was closed"
        cfg = self.cfg
        u8 = frames.dtype == torch.uint8
        want = (cfg.image_size, cfg.image_size, cfg.channels) if u8 else (cfg.channels, cfg.image_size, cfg.image_size)
        if frames.dim() != 4 or tuple(frames.shape[1:]) != want:
            raise ValueError(f"expected frames [n,{cfg.channels},{cfg.image_size},{cfg.image_size}] float32 or "
                             f"[n,{cfg.image_size},{cfg.image_size},{cfg.channels}] uint8, got {tuple(frames.shape)} {frames.dtype}")
        if not frames.is_cuda:
            raise _lib.HipPathUnavailable("frames must be on the GPU; there is no CPU path")
        frames = frames.contiguous() if u8 else frames.to(torch.float32).contiguous()
        n = frames.shape[0]
        desc = torch.empty((n, self._desc_dim), dtype=torch.float32, device=frames.device)
        tokens = None
        if return_tokens:
            if u8:
                raise ValueError("return_tokens is a debug path of the float32 entry point")
            tokens = torch.empty((n, *self._token_shape), dtype=torch.float32, device=frames.device)
        if n and u8:
            check(self._fn("forward_u8")(self._h, ptr(frames), n, self.u8_mean, self.u8_std, ptr(desc), current_stream()))
        elif n:
            check(self._fn("forward_debug")(self._h, ptr(frames), n, ptr(desc), ptr(tokens), current_stream()))
        return (desc, tokens) if return_tokens else desc

    def set_profiling(self, on: bool) -> None:
        """Per-launch HIP events; while on, the chunks of a call run back to back on the caller's stream."""
        check(self._fn("set_profiling")(self._h, int(on)))

    def _get_profile(self, classes: int):
        """(ms, launches) per class index, accumulated since set_profiling(True)"""
        ms = (ctypes.c_double * classes)()
        cnt = (ctypes.c_int64 * classes)()
        check(self._fn("get_profile")(self._h, ms, cnt))
        return ms, cnt

    def close(self):
        if self._h is not None:
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
