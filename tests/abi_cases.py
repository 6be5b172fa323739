"""Case table of the ABI placement tests (tests/test_gpu_abi_placement.py, tests/test_abi_cases_cpu.py).

One case is ONE call through the C ABI of include/vsc_hip.h, made with ctypes as vsc_hip/ops.py makes it, at the smallest
shapes at which the entry's write-out can still go wrong: one shape ragged in every tiled dimension, one of whole tiles.
The GPU test runs every case four ways -- plain, between guard bands, on a side stream behind a delay, and after other users
of the shared scratch -- and the CPU test holds the table to itself (every stream-taking export has a case or a stated
exclusion, `make` is deterministic, input and decoy give different references, every reference runs).

A case holds
  name        entry point and shape tag
  entry       the export(s) the call goes through
  make(seed)  -> dict of operands: torch CPU tensors are device operands (uploaded as they are), numpy arrays under keys that
              start with "h_" are HOST operands (tables, parameters).  make(SEED) is the input, make(DECOY) the decoy: the same
              shapes, other values, equally valid, another result.  Host operands are taken from the input in both.
  outputs     name -> (shape, torch dtype) of every device tensor the call only writes
  inout       names of operands the call also writes
  call(lib, p, inp, stream) -> dict of host results or None; p[name] is the device pointer of operand / output `name`
  reference(inp) -> name -> expected (torch tensor / numpy array; for the "bound" tolerance a pair (expected, bound))
  tol         name -> None (bit equality) | (rtol, atol) | "bound": the tolerance of the entry's existing parity test (`cite`)
  leave(inp)  -> name -> bool array, True where the header lets the call leave the element alone
  relations(out) asserts what the header promises BETWEEN outputs (the bf16 shadow is the rounded fp32 output, ...)
  enqueue_only  the header says the call only enqueues
  scratch     the call draws from the shared grow-only search scratch
  options     switches (vsc_set_option) the call runs under
  placement_bits  False (with placement_reason) where the result cannot be bit-identical across placements
"""
from __future__ import annotations

import ctypes
import functools
import math
import os
import sys
from dataclasses import dataclass, field
from typing import Callable

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from tools import synth  # noqa: E402

SEED, DECOY = 1, 1001
BF16, F32, F64, I32, I64, U8, U16 = (torch.bfloat16, torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8,
                                     torch.uint16)
FLT_MIN = np.finfo(np.float32).min     # -FLT_MAX: the search's padding score

# Exports that take a stream and have no case, each with its reason.
EXCLUDED = {
    "vsc_debug_spin_ticks": "measurement aid; it IS the delay of the stream leg (one wave, one store of its own tick count)",
}


@dataclass
class Case:
    name: str
    entry: tuple
    make: Callable
    outputs: dict
    call: Callable
    reference: Callable
    tol: dict
    cite: str
    inout: tuple = ()
    leave: Callable = None
    relations: Callable = None
    enqueue_only: bool = False
    scratch: bool = False
    options: dict = field(default_factory=dict)
    placement_bits: bool = True
    placement_reason: str = ""
    open: Callable = None          # (lib) -> context kept for the module (an encoder handle); call finds it under p["ctx"]

    def inputs(self):
        return self.make(SEED)

    def decoy(self):
        real, d = self.make(SEED), self.make(DECOY)
        return {k: (real[k] if k.startswith("h_") else v) for k, v in d.items()}

    def written(self):
        """names of every device tensor the call writes"""
        return tuple(self.inout) + tuple(self.outputs)


CASES: list = []


def _add(**kw):
    kw["entry"] = (kw["entry"],) if isinstance(kw["entry"], str) else tuple(kw["entry"])
    CASES.append(Case(**kw))


def by_name():
    return {c.name: c for c in CASES}


def _n(seed, shape, std=1.0):
    """bell-shaped values of the given std; operands above a million elements are uniform of that std instead (one hash pass, not
    four) and kept for the next case of the same shape -- callers do not write into them"""
    if int(np.prod(shape)) > 1 << 20:
        return _big(seed, tuple(shape), float(std))
    return torch.from_numpy(synth.normalish(seed, shape, std))


@functools.lru_cache(maxsize=6)
def _big(seed, shape, std):
    half = std * math.sqrt(3.0)
    return torch.from_numpy(synth.uniform(seed, shape, -half, half))


def _np(t):
    return t.numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _hp(a):
    """host pointer of a numpy array"""
    return ctypes.c_void_p(a.ctypes.data)


def _lib():
    from vsc_hip import _lib as L
    return L


# ======================================================================================================================
# vsc_gemm_bf16: 128 x 128 kernel (small problems), the 256-row kernels (m >= 1024 and more than 64 big tiles), the
# persistent kernel (more 256 x 256 tiles than CUs at K % 128 == 0).  tests/test_gpu_kernels.py: bf16 outputs rtol 2^-7,
# atol 2e-3 against fp32 torch on the rounded operands; fp32 outputs rtol 1e-5, atol 2e-4.
# ======================================================================================================================
EPI = {"bf16": 0, "gelu": 1, "qgelu": 2, "resadd": 3, "patch": 4, "f32": 5}
GEMM_SHAPES = [(257, 132, 64), (256, 256, 128), (1, 4, 64),
               (16385, 136, 64),       # 65 row tiles of 256: the smallest m that leaves the 128 x 128 kernel at k <= 512 (last tile: one row)
               (65537, 256, 128)]      # 257 tiles of 256 x 256 > 256 CUs: the smallest m on the persistent kernel at n = 256, k = 128


def _gemm_case(epi, m, n, k):
    tokens = 17 if epi == "patch" else 0
    frames = m // 16 if epi == "patch" else 0
    out_rows = frames * tokens if epi == "patch" else m
    out_dtype = BF16 if epi in ("bf16", "gelu", "qgelu") else F32

    def make(seed):
        s = seed * 100
        d = {"a": _n(s + 1, (m, k)).to(BF16), "w": _n(s + 2, (n, k), 0.05).to(BF16), "bias": _n(s + 3, (n,), 0.5)}
        if epi == "resadd":
            d["aux"] = _n(s + 4, (m, n))
        if epi == "patch":
            d["aux"] = _n(s + 4, (tokens, n), 0.3)
        return d

    def call(lib, p, inp, stream):
        return lib.vsc_gemm_bf16(p["a"], p["w"], p["bias"], p.get("aux"), p["out"], m, n, k, EPI[epi], tokens, stream)

    def reference(inp):
        z = inp["a"].float() @ inp["w"].float().t() + inp["bias"]
        if epi == "gelu":
            z = F.gelu(z)
        elif epi == "qgelu":
            z = z * torch.sigmoid(1.702 * z)
        elif epi == "resadd":
            z = z + inp["aux"]
        elif epi == "patch":
            full = torch.zeros(frames, tokens, n)
            full[:, 1:] = z.reshape(frames, tokens - 1, n) + inp["aux"][1:]
            z = full.reshape(out_rows, n)
        return {"out": z}

    def leave(inp):      # the CLS rows of VSC_EPI_PATCH_F32 are not this kernel's to write
        mask = np.zeros((frames, tokens, n), bool)
        mask[:, 0] = True
        return {"out": mask.reshape(out_rows, n)}

    _add(name=f"gemm_bf16/{epi}/{m}x{n}x{k}", entry="vsc_gemm_bf16", make=make, outputs={"out": ((out_rows, n), out_dtype)},
         call=call, reference=reference, tol={"out": (2 ** -7, 2e-3) if out_dtype == BF16 else (1e-5, 2e-4)},
         cite="test_gpu_kernels.py::test_gemm_bf16_store / _activation_epilogues / _residual_epilogue_in_place / _patch_epilogue",
         leave=leave if epi == "patch" else None, enqueue_only=True)


for _epi in ("bf16", "gelu", "qgelu", "resadd", "f32"):
    for _s in GEMM_SHAPES:
        _gemm_case(_epi, *_s)
for _s in ((48, 132, 64), (48, 256, 128), (16400, 136, 64)):     # frames = 3 (and 1025 on the 256-row kernel), tokens = 17
    _gemm_case("patch", *_s)


# vsc_gemm_resadd_ln_bf16: the tail form needs VSC_GEMM_LN_TAIL=1, n = 768, k > 512 with k % 128 == 0, ceil(m / 256) % 8 == 0 and
# more tiles than CUs -- 88 row blocks (264 tiles) is the smallest; one row more (89 blocks) must take the two launches.
def _resadd_ln_case(m, tail, want_path):
    n, k, eps = 768, 768, 1e-6

    def make(seed):
        s = seed * 100 + 10
        x = _n(s + 4, (m, n)).clone()
        x[:, 301] += 100.0
        return {"a": _n(s + 1, (m, k)).to(BF16), "w": _n(s + 2, (n, k), 0.05).to(BF16), "bias": _n(s + 3, (n,)), "x": x,
                "gamma": 1.0 + _n(s + 5, (n,), 0.1), "beta": _n(s + 6, (n,), 0.1)}

    def call(lib, p, inp, stream):
        rc = lib.vsc_gemm_resadd_ln_bf16(p["a"], p["w"], p["bias"], p["x"], p["gamma"], p["beta"], p["y"], m, n, k, eps, stream)
        assert rc or lib.vsc_gemm_resadd_ln_last_path() == want_path, "vsc_gemm_resadd_ln_last_path"
        return rc

    def reference(inp):
        x = inp["x"] + inp["a"].float() @ inp["w"].float().t() + inp["bias"]
        return {"x": x, "y": F.layer_norm(x, (n,), inp["gamma"], inp["beta"], eps).to(BF16).float()}

    def relations(out, inp):    # y is the LayerNorm of the x the call stored (test_gpu_kernels.py::test_layernorm: rtol 2^-7, atol 1e-5)
        want = F.layer_norm(out["x"], (n,), inp["gamma"], inp["beta"], eps).to(BF16).float()
        torch.testing.assert_close(out["y"].float(), want, rtol=2 ** -7, atol=1e-5)

    # y against the reference's own x: the 100-offset channel makes rstd ~ 1 / 36, so x's 2e-4 moves y by ~1e-5: inside rtol 2^-7
    _add(name=f"gemm_resadd_ln/{'tail' if tail else 'plain'}/{m}", entry="vsc_gemm_resadd_ln_bf16", make=make,
         outputs={"y": ((m, n), BF16)}, inout=("x",), call=call, reference=reference, tol={"x": (1e-5, 2e-4), "y": (2 ** -7, 2e-3)},
         cite="test_gpu_kernels.py::test_gemm_residual_epilogue_in_place (x), ::test_gemm_bf16_store's bf16 bound (y); "
              "test_gpu_gemm_ln_tail.py for the path", relations=relations, enqueue_only=True,
         options={"VSC_GEMM_LN_TAIL": "1"} if tail else {})


RESADD_LN_M = 88 * 256
_resadd_ln_case(RESADD_LN_M, True, 1)
_resadd_ln_case(RESADD_LN_M + 1, True, 2)
_resadd_ln_case(RESADD_LN_M, False, 2)
_resadd_ln_case(RESADD_LN_M + 1, False, 2)


# vsc_gemm_ln_bf16: row-owning tiles 512 x 128 / 256 x 256 / 128 x 512; with VSC_GEMM_LN_V4=1 the persistent kernel at n = 512
# needs ceil(m / 256) % 8 == 0 and more tiles than CUs: 136 row blocks, the last one holding one row.
def _gemm_ln_case(m, n, k, v4):
    eps = 1e-5

    def make(seed):
        s = seed * 100 + 20
        return {"a": _n(s + 1, (m, k)).to(BF16), "w": _n(s + 2, (n, k), k ** -0.5).to(BF16), "bias": _n(s + 3, (n,), 0.2),
                "gamma": 0.3 + _n(s + 5, (n,), 0.05), "beta": _n(s + 6, (n,), 0.05), "x_in": _n(s + 4, (m, n))}

    def call(lib, p, inp, stream):
        return lib.vsc_gemm_ln_bf16(p["a"], p["w"], p["bias"], p["gamma"], p["beta"], p["x_in"], p["x"], p["xb"], m, n, k, eps, stream)

    def reference(inp):
        t = inp["a"].float() @ inp["w"].float().t() + inp["bias"]
        return {"x": inp["x_in"] + F.layer_norm(t, (n,), inp["gamma"], inp["beta"], eps)}

    _add(name=f"gemm_ln/{'v4/' if v4 else ''}{m}x{n}x{k}", entry="vsc_gemm_ln_bf16", make=make,
         outputs={"x": ((m, n), F32), "xb": ((m, n), BF16)}, call=call, reference=reference, tol={"x": (1e-4, 1e-4)},
         cite="test_gpu_swin.py::test_gemm_ln_matches_torch", relations=_shadow("x", "xb"), enqueue_only=True,
         options={"VSC_GEMM_LN_V4": "1"} if v4 else {})


def _shadow(x, xb):
    def rel(out, inp):
        assert torch.equal(out[xb].view(torch.int16), out[x].to(BF16).view(torch.int16)), f"{xb} is not bf16({x})"
    return rel


_gemm_ln_case(129, 128, 32, False)
_gemm_ln_case(257, 512, 64, False)
_gemm_ln_case(256, 256, 64, False)
_gemm_ln_case(135 * 256 + 1, 512, 128, True)


# ---- the fused Swin-V2 block halves (csrc/swin_mlp.hip: 128-row tiles; csrc/swin_mlp512.hip: 128 rows per workgroup) ----------------
def _permuted_w2(w2):
    h = np.ascontiguousarray(w2.numpy())
    out = np.empty_like(h)
    rc = _lib().load().vsc_swin_mlp_permute_hidden_f32(h.ctypes.data, out.ctypes.data, h.shape[0])
    assert rc == 0
    return torch.from_numpy(out).to(BF16)


def _swin_block_case(kind, m, c):
    eps = 1e-5

    def make(seed):
        s = seed * 100 + 30
        w2 = _n(s + 4, (c, 4 * c), (4 * c) ** -0.5)
        d = {"w1": _n(s + 2, (4 * c, c), c ** -0.5).to(BF16), "b1": _n(s + 3, (4 * c,), 0.2), "w2": w2.to(BF16), "w2p": _permuted_w2(w2),
             "b2": _n(s + 5, (c,), 0.2), "g2": 0.3 + _n(s + 6, (c,), 0.05), "be2": _n(s + 7, (c,), 0.05), "x": _n(s + 1, (m, c))}
        if kind == "mlp":
            d["xb"] = d["x"].to(BF16)          # the MLP alone reads the shadow of x and writes the new one in its place
        if kind != "mlp":
            d.update(att=_n(s + 8, (m, c)).to(BF16), wp=_n(s + 9, (c, c), c ** -0.5).to(BF16), bp=_n(s + 10, (c,), 0.2),
                     g1=0.3 + _n(s + 11, (c,), 0.05), be1=_n(s + 12, (c,), 0.05))
        if kind == "qkv":
            d.update(wq=_n(s + 13, (3 * c, c), c ** -0.5).to(BF16), bq=_n(s + 14, (3 * c,), 0.2))
        return d

    def call(lib, p, inp, stream):
        if kind == "mlp":
            return lib.vsc_swin_mlp_bf16(p["w1"], p["b1"], p["w2p"], p["b2"], p["g2"], p["be2"], p["x"], p["xb"], m, c, eps, stream)
        head = (p["att"], p["wp"], p["bp"], p["g1"], p["be1"], p["w1"], p["b1"], p["w2p"], p["b2"], p["g2"], p["be2"])
        if kind == "proj":
            return lib.vsc_swin_proj_mlp_bf16(*head, p["x"], p["xb"], m, c, eps, stream)
        return lib.vsc_swin_proj_mlp_qkv_bf16(*head, p["wq"], p["bq"], p["x"], p["qkv"], m, c, eps, stream)

    def reference(inp):
        x1 = inp["x"]
        if kind != "mlp":
            x1 = x1 + F.layer_norm(inp["att"].float() @ inp["wp"].float().t() + inp["bp"], (c,), inp["g1"], inp["be1"], eps)
        h = F.gelu(x1.to(BF16).float() @ inp["w1"].float().t() + inp["b1"]).to(BF16).float()
        return {"x": x1 + F.layer_norm(h @ inp["w2"].float().t() + inp["b2"], (c,), inp["g2"], inp["be2"], eps)}

    def qkv_relation(out, inp):   # test_swin_proj_mlp_qkv_equals_proj_mlp_then_gemm: rtol 2^-7, atol 2e-3 against the stored x's shadow
        t = out["x"].to(BF16).float() @ inp["wq"].float().t() + inp["bq"]
        torch.testing.assert_close(out["qkv"].float(), t, rtol=2 ** -7, atol=2e-3)

    entry = {"mlp": "vsc_swin_mlp_bf16", "proj": "vsc_swin_proj_mlp_bf16", "qkv": "vsc_swin_proj_mlp_qkv_bf16"}[kind]
    outs = {"qkv": ((m, 3 * c), BF16)} if kind == "qkv" else {} if kind == "mlp" else {"xb": ((m, c), BF16)}
    # w2 (module order) is the reference's operand only; the call takes w2p
    _add(name=f"swin_{kind}/{m}x{c}", entry=entry, make=make, outputs=outs, inout=("x", "xb") if kind == "mlp" else ("x",), call=call,
         reference=reference,
         tol={"x": (0, 2e-3 if kind == "mlp" else 3e-3)},
         cite="test_gpu_swin.py::test_swin_mlp_matches_torch / _proj_mlp_matches_torch / _proj_mlp_qkv_equals_proj_mlp_then_gemm",
         relations=qkv_relation if kind == "qkv" else _shadow("x", "xb"), enqueue_only=True)


for _c in (128, 256, 512):
    for _m in (129, 128) + ((5,) if _c == 512 else ()):
        _swin_block_case("mlp", _m, _c)
        _swin_block_case("proj", _m, _c)
        if _c == 512:
            _swin_block_case("qkv", _m, _c)


# ---- attention ------------------------------------------------------------------------------------------------------------------
def _attention_case(frames, tokens, heads, dma):
    d = heads * 64

    def make(seed):
        qkv = _n(seed * 100 + 40 + tokens, (frames * tokens, 3 * d))
        qkv[:, : 2 * d] *= 2.0
        return {"qkv": qkv.to(BF16)}

    def call(lib, p, inp, stream):
        return lib.vsc_attention_bf16(p["qkv"], p["out"], frames, tokens, heads, stream)

    def reference(inp):
        q, k, v = inp["qkv"].float().reshape(frames, tokens, 3, heads, 64).permute(2, 0, 3, 1, 4)
        s = q @ k.transpose(-1, -2) / math.sqrt(64)
        return {"out": (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(frames * tokens, d)}

    _add(name=f"attention_bf16/{'dma/' if dma else ''}{frames}x{tokens}x{heads}", entry="vsc_attention_bf16", make=make,
         outputs={"out": ((frames * tokens, d), BF16)}, call=call, reference=reference, tol={"out": (2 ** -6, 1e-2)},
         cite="test_gpu_kernels.py::test_attention", enqueue_only=True, options={"VSC_ATTN_DMA": "1"} if dma else {})


for _dma in (False, True):
    for _s in ((2, 17, 2), (1, 1, 1), (2, 197, 3)):
        _attention_case(*_s, _dma)


def _attention_f32_case(kind):
    import attention_cases as ac
    heads, head_dim = 3, 48
    width = heads * head_dim
    if kind == "single":
        offs, rows = [0, 33], 33
    elif kind == "batch":
        offs, rows = [0, 7, 14, 21], 21
    else:                       # lengths 1, 7, 33 from row 3 on, four rows behind the last sequence
        offs, rows = [3, 4, 11, 44], 48

    def make(seed):
        d = {"qkv": ac.f32_random(seed * 100 + 50, rows, heads, head_dim)}
        if kind == "varlen":
            d["offs"] = torch.tensor(offs, dtype=I32)
        return d

    def call(lib, p, inp, stream):
        if kind == "single":
            return lib.vsc_attention_f32(p["qkv"], p["out"], 33, heads, head_dim, stream)
        if kind == "batch":
            return lib.vsc_attention_f32_batch(p["qkv"], p["out"], 7, heads, head_dim, 3, stream)
        return lib.vsc_attention_f32_varlen(p["qkv"], p["out"], p["offs"], 3, 33, heads, head_dim, stream)

    def reference(inp):
        return {"out": ac.f32_reference(inp["qkv"], heads, head_dim, offs)}

    def leave(inp):
        mask = np.ones((rows, width), bool)
        mask[offs[0]:offs[-1]] = False
        return {"out": mask}

    entry = {"single": "vsc_attention_f32", "batch": "vsc_attention_f32_batch", "varlen": "vsc_attention_f32_varlen"}[kind]
    _add(name=f"attention_f32/{kind}", entry=entry, make=make, outputs={"out": ((rows, width), F32)}, call=call,
         reference=reference, tol={"out": "bound"}, cite="test_gpu_attention.py::test_attention_f32_within_fp32_bound "
         "(attention_cases.f32_reference)", leave=leave if kind == "varlen" else None, enqueue_only=True)


for _k in ("single", "batch", "varlen"):
    _attention_f32_case(_k)


def _window_attention_case(window, res, shift, bounded):
    from oracle import swin_oracle
    heads = 2
    frames = 2 if res == window else 1
    c, n = heads * 32, window * window

    def raw(seed):
        s = seed * 100 + 60
        qkv = _n(s + res + shift, (frames * res * res, 3 * c)).to(BF16)
        table = 16 * torch.sigmoid(_n(s + 7, (heads, (2 * window - 1) ** 2)))
        scale = torch.exp(torch.clamp(math.log(10.0) + _n(s + 8, (heads,), 0.4), max=math.log(100.0)))
        return qkv, table, scale

    def make(seed):
        qkv, table, scale = raw(seed)
        if bounded:       # ops.window_attention_bf16(bounded=True): the head's upper bound folded into its table, -scale passed
            bmax, bmin = table.max(dim=1).values, table.min(dim=1).values
            ok = (2 * scale + (bmax - bmin)) <= 69.0
            table = torch.where(ok[:, None], table - (bmax + scale)[:, None], table).contiguous()
            scale = torch.where(ok, -scale, scale).contiguous()
        return {"qkv": qkv, "table": table, "scale": scale}

    def call(lib, p, inp, stream):
        return lib.vsc_window_attention_bf16(p["qkv"], p["out"], p["table"], p["scale"], frames, res, window, shift, heads, stream)

    def reference(inp):
        # (bounded form: a head's table shifted by a constant leaves its softmax alone, and |scale| is its scale)
        qkv, table, scale = inp["qkv"], inp["table"], inp["scale"].abs()
        bias = table[:, swin_oracle.relative_position_index(window).reshape(-1)].reshape(heads, n, n)
        x = qkv.float().reshape(frames, res, res, 3 * c)
        if shift:
            x = torch.roll(x, (-shift, -shift), (1, 2))
        xw = swin_oracle._windows(x, res, window)
        q, k, v = xw.reshape(-1, n, 3, heads, 32).permute(2, 0, 3, 1, 4)
        attn = F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1) * scale.reshape(1, heads, 1, 1) + bias[None]
        if shift:
            mk = swin_oracle.shift_mask(res, window, shift)
            attn = (attn.reshape(frames, -1, heads, n, n) + mk[None, :, None]).reshape(-1, heads, n, n)
        o = (torch.softmax(attn, -1) @ v).transpose(1, 2).reshape(-1, n, c)
        o = swin_oracle._unwindows(o, res, window, frames)
        if shift:
            o = torch.roll(o, (shift, shift), (1, 2))
        return {"out": o.reshape(frames * res * res, c)}

    _add(name=f"window_attention/{'bounded/' if bounded else ''}w{window}_r{res}_s{shift}", entry="vsc_window_attention_bf16", make=make,
         outputs={"out": ((frames * res * res, c), BF16)}, call=call, reference=reference, tol={"out": (2 ** -6, 2e-2)},
         cite="test_gpu_swin.py::test_window_attention", enqueue_only=True)


for _w in (8, 12, 16, 24):
    for _res in (_w, 2 * _w):
        for _shift in (0, _w // 2):
            for _b in (False, True):
                _window_attention_case(_w, _res, _shift, _b)


# ---- row kernels ----------------------------------------------------------------------------------------------------------------
def _layernorm_case(rows, width, out_f32):
    eps = 1e-6

    def make(seed):
        s = seed * 100 + 70
        return {"x": _n(s, (rows, width), 2.0) + 0.5, "g": 1.0 + _n(s + 1, (width,), 0.1), "b": _n(s + 2, (width,), 0.1)}

    def call(lib, p, inp, stream):
        return lib.vsc_layernorm_f32(p["x"], p["g"], p["b"], p["out"], rows, width, eps, int(out_f32), stream)

    def reference(inp):
        ref = F.layer_norm(inp["x"], (width,), inp["g"], inp["b"], eps)
        return {"out": ref if out_f32 else ref.to(BF16).float()}

    _add(name=f"layernorm/{'f32' if out_f32 else 'bf16'}/{rows}x{width}", entry="vsc_layernorm_f32", make=make,
         outputs={"out": ((rows, width), F32 if out_f32 else BF16)}, call=call, reference=reference,
         tol={"out": (1e-5, 1e-5) if out_f32 else (2 ** -7, 1e-5)}, cite="test_gpu_kernels.py::test_layernorm", enqueue_only=True)


for _f in (False, True):
    _layernorm_case(5, 128, _f)
    _layernorm_case(3, 1024, _f)


def _ln_residual_case(rows, width):
    eps = 1e-5

    def make(seed):
        s = seed * 100 + 80
        return {"t": _n(s, (rows, width), 2.0) + 0.3, "g": 0.3 + _n(s + 2, (width,), 0.05), "b": _n(s + 3, (width,), 0.05),
                "x_in": _n(s + 1, (rows, width))}

    def call(lib, p, inp, stream):
        return lib.vsc_ln_residual_f32(p["t"], p["g"], p["b"], p["x_in"], p["x"], p["xb"], rows, width, eps, stream)

    _add(name=f"ln_residual/{rows}x{width}", entry="vsc_ln_residual_f32", make=make,
         outputs={"x": ((rows, width), F32), "xb": ((rows, width), BF16)}, call=call,
         reference=lambda inp: {"x": inp["x_in"] + F.layer_norm(inp["t"], (width,), inp["g"], inp["b"], eps)},
         tol={"x": (1e-5, 1e-5)}, cite="test_gpu_swin.py::test_ln_residual", relations=_shadow("x", "xb"), enqueue_only=True)


_ln_residual_case(7, 64)


def _patchify_case():
    from oracle import vit_oracle
    from vsc_hip.config import get_config
    cfg = get_config("tiny")
    n = 2
    kpad = (cfg.patch_dim + 63) // 64 * 64
    rows = n * (cfg.image_size // cfg.patch_size) ** 2

    def reference(inp):
        out = torch.zeros(rows, kpad, dtype=BF16)
        out[:, : cfg.patch_dim] = vit_oracle.patchify(inp["frames"], cfg.patch_size).reshape(-1, cfg.patch_dim).to(BF16)
        return {"out": out}

    _add(name="patchify/tiny", entry="vsc_patchify_bf16", make=lambda seed: {"frames": torch.from_numpy(synth.frames(seed + 50, n, cfg))},
         outputs={"out": ((rows, kpad), BF16)},
         call=lambda lib, p, inp, stream: lib.vsc_patchify_bf16(p["frames"], p["out"], n, cfg.channels, cfg.image_size, cfg.patch_size, kpad, stream),
         reference=reference, tol={"out": None}, cite="test_gpu_kernels.py::test_patchify_bit_exact", enqueue_only=True)


_patchify_case()


def _merge_gather_case(frames, res, c):
    def reference(inp):
        g = inp["xb"].reshape(frames, res, res, c)
        return {"out": torch.cat([g[:, 0::2, 0::2], g[:, 1::2, 0::2], g[:, 0::2, 1::2], g[:, 1::2, 1::2]], -1).reshape(-1, 4 * c).contiguous()}

    _add(name=f"merge_gather/{frames}x{res}x{c}", entry="vsc_merge_gather_bf16",
         make=lambda seed: {"xb": _n(seed * 100 + 90, (frames * res * res, c)).to(BF16)},
         outputs={"out": ((frames * (res // 2) ** 2, 4 * c), BF16)},
         call=lambda lib, p, inp, stream: lib.vsc_merge_gather_bf16(p["xb"], p["out"], frames, res, c, stream),
         reference=reference, tol={"out": None}, cite="test_gpu_swin.py::test_merge_gather_bit_exact", enqueue_only=True)


_merge_gather_case(3, 8, 64)


def _l2_case(n, d):
    from oracle import knn_oracle

    def make(seed):
        x = synth.normalish(seed * 100 + 95, (n, d))
        x[2] = 0.0
        return {"x": torch.from_numpy(x)}

    _add(name=f"l2_normalize/{n}x{d}", entry="vsc_l2_normalize_f32", make=make, outputs={}, inout=("x",),
         call=lambda lib, p, inp, stream: lib.vsc_l2_normalize_f32(p["x"], n, d, stream),
         reference=lambda inp: {"x": knn_oracle.l2_normalize(inp["x"].numpy())}, tol={"x": (0, 1e-6)},
         cite="test_gpu_kernels.py::test_l2_normalize", enqueue_only=True)


_l2_case(5, 511)


# ======================================================================================================================
# Search: bit-exact against oracle/knn_oracle (tests/test_gpu_knn.py).  Exact path: nq * nr < 2^24.
# ======================================================================================================================
def _bank(seed, n, d):
    return synth.descriptor_bank(seed, n, d)


def _knn_case(nq, nr, d, k, path):
    from oracle import knn_oracle
    want_path = {"exact": 1, "bf16": 2}[path]

    def make(seed):
        return {"q": torch.from_numpy(_bank(seed * 100 + 1, nq, d)), "r": torch.from_numpy(_bank(seed * 100 + 2, nr, d))}

    def call(lib, p, inp, stream):
        rc = lib.vsc_knn_ip_f32(p["q"], nq, p["r"], nr, d, k, 7, p["scores"], p["ids"], stream)
        assert rc or lib.vsc_knn_last_path() in ((1,) if want_path == 1 else (2, 3)), "vsc_knn_last_path"
        return rc

    def reference(inp):
        D, I = knn_oracle.knn_ip(inp["q"].numpy(), inp["r"].numpy(), k)
        return {"scores": D, "ids": I + 7}

    _add(name=f"knn_ip/{path}/{nq}x{nr}x{d}_k{k}", entry="vsc_knn_ip_f32", make=make,
         outputs={"scores": ((nq, k), F32), "ids": ((nq, k), I64)}, call=call, reference=reference, tol={"scores": None, "ids": None},
         cite="test_gpu_knn.py (bit-exact against oracle/knn_oracle.c)", enqueue_only=path == "exact", scratch=True,
         options={"VSC_KNN_PATH": path} if path != "exact" else {})


for _d in (5, 512):
    for _k in (1, 100):
        _knn_case(257, 1025, _d, _k, "exact")
_knn_case(257, 4097, 512, 100, "bf16")


def _knn_floor_case(nq, nr, d, k):
    from oracle import knn_oracle

    def make(seed):
        q, r = _bank(seed * 100 + 3, nq, d), _bank(seed * 100 + 4, nr, d)
        Dr, _ = knn_oracle.knn_ip(q, r, k)
        floor = Dr[:, k // 2].copy()                   # exactly a score of the list: ties at the floor stay in
        floor[0:8] = Dr[0:8, 0] + 1.0                  # nothing reaches it
        floor[8:16] = FLT_MIN
        floor[16:24] = -np.inf
        return {"q": torch.from_numpy(q), "r": torch.from_numpy(r), "floor": torch.from_numpy(floor)}

    def reference(inp):
        D, I = knn_oracle.knn_ip(inp["q"].numpy(), inp["r"].numpy(), k)
        cut = D < inp["floor"].numpy()[:, None]
        return {"scores": np.where(cut, FLT_MIN, D).astype(np.float32), "ids": np.where(cut, -1, I)}

    _add(name=f"knn_ip_floor/{nq}x{nr}x{d}_k{k}", entry="vsc_knn_ip_floor_f32", make=make,
         outputs={"scores": ((nq, k), F32), "ids": ((nq, k), I64)},
         call=lambda lib, p, inp, stream: lib.vsc_knn_ip_floor_f32(p["q"], nq, p["r"], nr, d, k, 0, p["floor"], p["scores"], p["ids"], stream),
         reference=reference, tol={"scores": None, "ids": None}, cite="test_gpu_knn.py::test_knn_with_a_floor_bit_exact",
         enqueue_only=True, scratch=True)


_knn_floor_case(257, 1025, 64, 10)


def _knn_merge_case(nq, d, k):
    from oracle import knn_oracle
    cuts = [0, 400, 405, 1025]         # three shards, one of them with fewer rows than k

    def make(seed):
        q, r = _bank(seed * 100 + 5, nq, d), _bank(seed * 100 + 6, cuts[-1], d)
        S, I = np.full((3, nq, k), FLT_MIN, np.float32), np.full((3, nq, k), -1, np.int64)
        for s in range(3):
            rows = cuts[s + 1] - cuts[s]
            D, J = knn_oracle.knn_ip(q, r[cuts[s]:cuts[s + 1]], min(k, rows))
            S[s, :, :min(k, rows)], I[s, :, :min(k, rows)] = D, J + cuts[s]
        return {"scores_in": torch.from_numpy(S), "ids_in": torch.from_numpy(I)}

    def reference(inp):
        # the k best of the union of the parts' lists, score descending, equal scores by ascending id
        S, I = inp["scores_in"].numpy().transpose(1, 0, 2).reshape(nq, -1), inp["ids_in"].numpy().transpose(1, 0, 2).reshape(nq, -1)
        out_s, out_i = np.empty((nq, k), np.float32), np.empty((nq, k), np.int64)
        for i in range(nq):
            valid = np.flatnonzero(I[i] >= 0)
            order = valid[np.lexsort((I[i][valid], -S[i][valid].astype(np.float64)))][:k]
            out_s[i], out_i[i] = S[i][order], I[i][order]
        return {"scores": out_s, "ids": out_i}

    _add(name=f"knn_merge_parts/3x{nq}_k{k}", entry="vsc_knn_merge_parts_f32", make=make,
         outputs={"scores": ((nq, k), F32), "ids": ((nq, k), I64)},
         call=lambda lib, p, inp, stream: lib.vsc_knn_merge_parts_f32(p["scores_in"], p["ids_in"], 3, nq, k, p["scores"], p["ids"], stream),
         reference=reference, tol={"scores": None, "ids": None},
         cite="test_gpu_knn.py::test_knn_shard_by_shard_with_carried_floor_equals_one_sweep (the merge equals one sweep bit for bit)",
         enqueue_only=True, scratch=True)


_knn_merge_case(257, 64, 10)


def _range_case(nq, nr, d, path, fill):
    from oracle import knn_oracle
    radius = 0.3
    want_path = {"exact": (1,), "bf16": (2, 3)}[path]

    def make(seed):
        q, r = _bank(seed * 100 + 7, nq, d), _bank(seed * 100 + 8, nr, d)
        return {"q": torch.from_numpy(q), "r": torch.from_numpy(r)}

    def capacity():
        inp = make(SEED)
        return int(knn_oracle.range_search_ip(inp["q"].numpy(), inp["r"].numpy(), radius)[0][-1]) + 5 if fill else 0

    cap = capacity()

    def call(lib, p, inp, stream):
        total = ctypes.c_int64(-1)
        rc = lib.vsc_range_search_ip_f32(p["q"], nq, p["r"], nr, d, radius, 3, p["lims"], p.get("scores"), p.get("ids"), cap,
                                         ctypes.byref(total), stream)
        assert rc or lib.vsc_range_search_last_path() in want_path, "vsc_range_search_last_path"
        return rc, {"h_total": np.array([total.value], np.int64)}

    def reference(inp):
        lims, D, I = knn_oracle.range_search_ip(inp["q"].numpy(), inp["r"].numpy(), radius)
        out = {"lims": lims, "h_total": np.array([lims[-1]], np.int64)}
        if fill and lims[-1] <= cap:
            out["scores"], out["ids"] = np.resize(D, cap).astype(np.float32), np.resize(I + 3, cap)
        return out

    def leave(inp):     # CSR slots past *total_out; everything when the total exceeds the capacity (the decoy's may)
        total = int(knn_oracle.range_search_ip(inp["q"].numpy(), inp["r"].numpy(), radius)[0][-1])
        mask = np.arange(cap) >= (total if total <= cap else 0)
        return {"scores": mask, "ids": mask}

    _add(name=f"range_search/{path}/{'fill' if fill else 'count'}/{nq}x{nr}x{d}", entry="vsc_range_search_ip_f32", make=make,
         outputs={"lims": ((nq + 1,), I64), **({"scores": ((cap,), F32), "ids": ((cap,), I64)} if fill else {})}, call=call,
         reference=reference, tol={"lims": None, "scores": None, "ids": None, "h_total": None},
         cite="test_gpu_knn.py (range search against oracle/knn_oracle.c, bit-exact)", leave=leave if fill else None, scratch=True,
         options={"VSC_RANGE_PATH": path})


for _path, _nr in (("exact", 1025), ("bf16", 4097)):
    for _fill in (False, True):
        _range_case(257, _nr, 64, _path, _fill)


def _pair_similarity_case():
    from oracle import knn_oracle
    nq, nr, d = 40, 50, 33
    pairs = np.array([[0, 7, 3, 9], [8, 1, 49, 1], [20, 20, 0, 50]], np.int64)     # one of them 1 x 1
    total = int((pairs[:, 1] * pairs[:, 3]).sum())

    def make(seed):
        return {"q": torch.from_numpy(_bank(seed * 100 + 9, nq, d)), "r": torch.from_numpy(_bank(seed * 100 + 10, nr, d)), "h_pairs": pairs}

    def call(lib, p, inp, stream):
        offs = np.full(len(pairs) + 1, -1, np.int64)
        rc = lib.vsc_pair_similarity_f32(p["q"], nq, p["r"], nr, d, _hp(pairs), len(pairs), _hp(offs), p["out"], total, stream)
        return rc, {"h_offsets": offs}

    def reference(inp):
        full = knn_oracle.ip_matrix(inp["q"].numpy(), inp["r"].numpy())
        parts = [full[a:a + b, c:c + e].reshape(-1) for a, b, c, e in pairs]
        return {"out": np.concatenate(parts), "h_offsets": np.concatenate([[0], np.cumsum([x.size for x in parts])]).astype(np.int64)}

    _add(name="pair_similarity/3_pairs", entry="vsc_pair_similarity_f32", make=make, outputs={"out": ((total,), F32)}, call=call,
         reference=reference, tol={"out": None, "h_offsets": None}, cite="test_gpu_knn.py (pair_similarity equals slices of the exact product)",
         scratch=True)


_pair_similarity_case()


def _pair_max_case(nq, nr, d, path):
    from oracle import matching_oracle
    nqv, nrv, thr = 7, 30, 0.3
    want_path = {"exact": (1,), "bf16": (2, 3)}[path]

    def make(seed):
        s = seed * 100 + 11
        qv = np.sort((synth.uniform(s + 2, (nq,), 0, nqv)).astype(np.int32))
        rv = np.sort((synth.uniform(s + 3, (nr,), 0, nrv)).astype(np.int32))
        return {"q": torch.from_numpy(_bank(s, nq, d)), "qv": torch.from_numpy(qv), "r": torch.from_numpy(_bank(s + 1, nr, d)),
                "rv": torch.from_numpy(rv)}

    def ref(inp):
        return matching_oracle.video_pair_max(inp["q"].numpy(), inp["qv"].numpy(), nqv, inp["r"].numpy(), inp["rv"].numpy(), nrv, thr)

    cap = int(ref(make(SEED))[0][-1]) + 3

    def call(lib, p, inp, stream):
        total = ctypes.c_int64(-1)
        rc = lib.vsc_video_pair_max_f32(p["q"], nq, p["qv"], nqv, p["r"], nr, p["rv"], nrv, d, thr, p["lims"], p["rvideo"], p["score"],
                                        cap, ctypes.byref(total), stream)
        assert rc or lib.vsc_video_pair_max_last_path() in want_path, "vsc_video_pair_max_last_path"
        return rc, {"h_total": np.array([total.value], np.int64)}

    def reference(inp):
        lims, cols, sc = ref(inp)
        out = {"lims": lims, "h_total": np.array([lims[-1]], np.int64)}
        if lims[-1] <= cap:
            out["rvideo"], out["score"] = np.resize(cols, cap).astype(np.int32), np.resize(sc, cap).astype(np.float32)
        return out

    def leave(inp):
        total = int(ref(inp)[0][-1])
        mask = np.arange(cap) >= (total if total <= cap else 0)
        return {"rvideo": mask, "score": mask}

    _add(name=f"video_pair_max/{path}/{nq}x{nr}", entry="vsc_video_pair_max_f32", make=make,
         outputs={"lims": ((nqv + 1,), I64), "rvideo": ((cap,), I32), "score": ((cap,), F32)}, call=call, reference=reference,
         tol={"lims": None, "rvideo": None, "score": None, "h_total": None},
         cite="test_gpu_knn.py (video_pair_max against oracle/matching_oracle.video_pair_max, bit-exact)", leave=leave, scratch=True,
         options={"VSC_PAIRMAX_PATH": path})


_pair_max_case(257, 1025, 64, "exact")
_pair_max_case(257, 4097, 64, "bf16")


def _global_topk_case(n, want, with_rows):
    import global_topk_contract as G
    cap = min(want, n)

    def make(seed):
        s = seed * 100 + 15
        scores = np.round(synth.uniform(s, (n,)) * 64) / 64             # a coarse grid: many equal scores
        scores[5], scores[n - 1] = -0.0, 0.0
        ids = (synth.uniform(s + 1, (n,), 0, 5000)).astype(np.int64)
        ids[::97] = -1                                                   # padding entries
        d = {"scores": torch.from_numpy(scores.astype(np.float32)), "ids": torch.from_numpy(ids)}
        if with_rows:
            d["rows"] = torch.from_numpy((synth.uniform(s + 2, (n,), 0, 300)).astype(np.int64))
        return d

    def ref(inp):
        return G.global_topk(inp["scores"].numpy(), inp["ids"].numpy(), want, rows=inp["rows"].numpy() if with_rows else None,
                             row_stride=None if with_rows else 3)

    def call(lib, p, inp, stream):
        return lib.vsc_global_topk_f32(p["scores"], p.get("rows"), p["ids"], n, 3, want, p["out_rows"], p["out_ids"], p["out_scores"],
                                       p["count"], stream)

    def reference(inp):
        rows, ids, sc = ref(inp)
        m = len(ids)
        return {"out_rows": np.resize(rows, cap), "out_ids": np.resize(ids, cap), "out_scores": np.resize(sc, cap).astype(np.float32),
                "count": np.array([m], np.int64)}

    def leave(inp):
        mask = np.arange(cap) >= len(ref(inp)[1])
        return {"out_rows": mask, "out_ids": mask, "out_scores": mask}

    _add(name=f"global_topk/{'rows' if with_rows else 'stride'}/n{n}_want{want}", entry="vsc_global_topk_f32", make=make,
         outputs={"out_rows": ((cap,), I64), "out_ids": ((cap,), I64), "out_scores": ((cap,), F32), "count": ((1,), I64)}, call=call,
         reference=reference, tol={"out_rows": None, "out_ids": None, "out_scores": None, "count": None},
         cite="test_gpu_global_topk.py (bit for bit against tests/global_topk_contract.py)", leave=leave, enqueue_only=True, scratch=True)


GLOBAL_TOPK_TILE = 2048        # VSC_GLOBAL_TOPK_TILE
for _rows in (False, True):
    for _want in (1, GLOBAL_TOPK_TILE + 1):
        _global_topk_case(GLOBAL_TOPK_TILE + 1, _want, _rows)


def _first_hits_case(n, limit):
    import global_topk_contract as G
    nq_rows, nr_rows, nrv = 600, 900, 23
    cap = n if limit < 0 else min(n, limit)

    def make(seed):
        s = seed * 100 + 18
        rows, ids = (synth.uniform(s, (n,), 0, nq_rows)).astype(np.int64), (synth.uniform(s + 1, (n,), 0, nr_rows)).astype(np.int64)
        dup = 1 + seed // 1000 % 2            # a repeated pair among the first three hits, elsewhere in the decoy
        rows[dup], ids[dup] = rows[0], ids[0]
        return {"rows": torch.from_numpy(rows), "ids": torch.from_numpy(ids),
                "qv": torch.from_numpy((synth.uniform(s + 2, (nq_rows,), 0, 11)).astype(np.int32)),
                "rv": torch.from_numpy((synth.uniform(s + 3, (nr_rows,), 0, nrv)).astype(np.int32))}

    def ref(inp):
        return G.pair_first_hits(inp["rows"].numpy(), inp["ids"].numpy(), inp["qv"].numpy(), inp["rv"].numpy(), nrv, limit)

    def reference(inp):
        pos = ref(inp)
        return {"pos": np.resize(pos, cap), "count": np.array([len(pos)], np.int64)}

    _add(name=f"pair_first_hits/n{n}_limit{limit}", entry="vsc_pair_first_hits", make=make,
         outputs={"pos": ((cap,), I64), "count": ((1,), I64)},
         call=lambda lib, p, inp, stream: lib.vsc_pair_first_hits(p["rows"], p["ids"], n, p["qv"], p["rv"], nrv, limit, p["pos"], p["count"], stream),
         reference=reference, tol={"pos": None, "count": None}, cite="test_gpu_global_topk.py (against global_topk_contract.pair_first_hits)",
         leave=lambda inp: {"pos": np.arange(cap) >= len(ref(inp))}, enqueue_only=True, scratch=True)


_first_hits_case(2049, -1)
_first_hits_case(2049, 3)


# ======================================================================================================================
# Structured entries: the smallest cases of the existing case files, packed at odd element offsets.  The decoy is the same
# set of matrices with their rows reversed.
# ======================================================================================================================
def _pack(mats, lead=7):
    """matrices back to back behind `lead` unused floats, one unused float wherever that makes the next offset odd"""
    parts, offs, off = [np.full(lead, 9.0e9, np.float32)], [], lead
    for m in mats:
        if off % 2 == 0:
            parts.append(np.full(1, 9.0e9, np.float32))
            off += 1
        offs.append(off)
        parts.append(np.ascontiguousarray(m, np.float32).reshape(-1))
        off += m.size
    return np.concatenate(parts), offs


def _tn_case():
    import tn_cases
    import tn_contract
    by = tn_cases.by_name()
    picks = [by[k] for k in ("q1r1_b05", "q2_b05", "qlestep_b05", "const_b05_1", "lastnode_b05", "diag1_b05_30x60_0")]
    prm = tn_cases.TN_SSCD
    assert all(c["params"] == prm and c["bias"] == 0.5 for c in picks)
    slots = prm["max_path"] + 1
    n = len(picks)

    def make(seed):
        mats = [tn_cases.matrix(c) for c in picks]
        if seed != SEED:
            mats = [np.ascontiguousarray(m[::-1]) for m in mats]
        flat, offs = _pack(mats)
        table = np.array([[o, m.shape[0], m.shape[1]] for o, m in zip(offs, mats)], np.int64)
        return {"sims": torch.from_numpy(flat), "h_pairs": table}

    def call(lib, p, inp, stream):
        return lib.vsc_tn_align_f32(p["sims"], inp["sims"].numel(), _hp(inp["h_pairs"]), n, 0.5, prm["tn_max_step"], prm["tn_top_k"],
                                    prm["max_path"], prm["min_sim"], prm["min_length"], prm["max_iou"], p["boxes"], p["counts"], p["maxsim"],
                                    stream)

    def reference(inp):
        flat = inp["sims"].numpy()
        boxes, counts, maxsim = np.zeros((n, slots, 4), np.int32), np.zeros(n, np.int32), np.zeros((n, slots), np.float32)
        for i, (off, q, r) in enumerate(inp["h_pairs"]):
            m = flat[off:off + q * r].reshape(q, r)
            b, _ = tn_contract.tn_contract(m, 0.5, **prm)
            counts[i] = len(b)
            for j, (x1, y1, x2, y2) in enumerate(b):
                boxes[i, j] = (x1, y1, x2, y2)
                maxsim[i, j] = np.float32((m + np.float32(0.5))[x1:x2, y1:y2].max() - np.float32(0.5))
        return {"boxes": boxes, "counts": counts, "maxsim": maxsim}

    _add(name="tn_align/6_pairs_odd_offsets", entry="vsc_tn_align_f32", make=make,
         outputs={"boxes": ((n, slots, 4), I32), "counts": ((n,), I32), "maxsim": ((n, slots), F32)}, call=call, reference=reference,
         tol={"boxes": None, "counts": None, "maxsim": None},
         cite="test_gpu_tn_align.py::test_fixture_boxes_identical / ::test_maxsim_bit_equal_to_host (tests/tn_contract.py)", scratch=True)


_tn_case()


def _segments_case():
    import seg_cases
    import seg_contract
    by = seg_cases.by_name()
    picks = [by[k] for k in ("edge_1x1", "edge_4x4", "clean_00_40x50", "clean_02_48x48", "edge_3x60")]
    passes = seg_cases.PASSES
    n, T, S = len(picks), len(passes), 8
    thr = np.array([p[0] for p in passes], np.float32)
    ratio = np.array([p[1] for p in passes], np.float64)

    def make(seed):
        mats = [seg_cases.matrix(c) for c in picks]
        if seed != SEED:
            mats = [np.ascontiguousarray(m[::-1]) for m in mats]
        flat, offs = _pack(mats)
        table = np.array([[o, m.shape[0], m.shape[1]] for o, m in zip(offs, mats)], np.int64)
        return {"maps": torch.from_numpy(flat), "h_items": table}

    def call(lib, p, inp, stream):
        return lib.vsc_match_segments_f32(p["maps"], inp["maps"].numel(), _hp(inp["h_items"]), n, _hp(thr), _hp(ratio), T, S, p["segments"],
                                          p["scores"], p["counts"], stream)

    def ref(inp):
        flat = inp["maps"].numpy()
        seg, sc, cnt = np.zeros((n, T, S, 4), np.int32), np.zeros((n, T, S), np.float64), np.zeros((n, T), np.int32)
        for i, (off, h, w) in enumerate(inp["h_items"]):
            m = flat[off:off + h * w].reshape(h, w)
            for t, (th, ra) in enumerate(passes):
                rows, _ = seg_contract.segments(m, th, ra)
                cnt[i, t] = len(rows)
                for j, row in enumerate(rows[:S]):
                    seg[i, t, j], sc[i, t, j] = row[:4], row[4]
        return seg, sc, cnt

    def reference(inp):
        seg, sc, cnt = ref(inp)
        return {"segments": seg.reshape(-1, 4), "scores": sc.reshape(-1), "counts": cnt.reshape(-1)}

    def leave(inp):     # the header promises the FOUND segments; slots behind the count are the caller's (ops.match_segments zeroes them)
        cnt = ref(inp)[2]
        mask = np.arange(S)[None, None, :] >= cnt[:, :, None]
        return {"segments": np.repeat(mask[..., None], 4, -1).reshape(-1, 4), "scores": mask.reshape(-1)}

    _add(name="match_segments/5_maps_odd_offsets", entry="vsc_match_segments_f32", make=make,
         outputs={"segments": ((n * T * S, 4), I32), "scores": ((n * T * S,), F64), "counts": ((n * T,), I32)}, call=call,
         reference=reference, tol={"segments": None, "scores": (0, 1e-9), "counts": None},
         cite="test_gpu_match_segments.py::test_kernel_equals_contract_on_every_fixture_entry (SCORE_TOL 1e-9, tests/seg_contract.py)",
         leave=leave, scratch=True)


_segments_case()


def _match_maps_case(R, with_transpose):
    import match_maps_cases as MC
    import match_maps_contract as C
    keep = ("single_smaller", "single_both", "single_fewer_rows_than_frames", "single_r1", "multi_r1", "multi_f3_v2", "multi_f10_v3",
            "identical_views", "sum_order", "edge_31x33", "edge_33x31")
    items = [it for it in MC.planted(R) if it[0] in keep]
    n, slices = len(items), 2 if with_transpose else 1

    def make(seed):
        its = items if seed == SEED else [(nm, np.ascontiguousarray(m[::-1] * np.float32(0.5)), f) for nm, m, f in items]
        flat, table = MC.pack(its)
        return {"sims": torch.from_numpy(flat), "h_items": table}

    def call(lib, p, inp, stream):
        return lib.vsc_match_maps_f32(p["sims"], inp["sims"].numel(), _hp(inp["h_items"]), n, R, int(with_transpose), p["view_start"], p["out"],
                                      stream)

    def reference(inp):
        starts, out = C.match_maps(inp["sims"].numpy(), inp["h_items"], R, with_transpose)
        return {"view_start": starts, "out": out}

    def leave(inp):     # view_start of single-view items (q_rows <= frames)
        t = inp["h_items"]
        return {"view_start": t[:, 1] <= t[:, 3]}

    _add(name=f"match_maps/R{R}_{'t' if with_transpose else 'n'}", entry="vsc_match_maps_f32", make=make,
         outputs={"view_start": ((n,), I32), "out": ((n * slices, R, R, 3), F32)}, call=call, reference=reference,
         tol={"view_start": None, "out": None}, cite="test_gpu_match_maps.py (bit for bit against tests/match_maps_contract.py)",
         leave=leave, enqueue_only=True)


_match_maps_case(32, True)
_match_maps_case(33, False)


def _view_frames(seed):
    import view_cases
    case = {c["name"]: c for c in view_cases.cases()}["plain"]
    case = dict(case, n=5, size=[37, 53], panels=[[0, 37, 0, 53]], seed=case["seed"] + (0 if seed == SEED else 1))
    return view_cases.frames(case)      # uint8 [5, 37, 53, 3]: odd sizes, a drifting dark square (edges)


def _view_cases():
    import canny_cpu
    n, h, w = 5, 37, 53
    idx = np.array([0, 2, 4, 2], np.int32)
    boxes = np.array([[0, 37, 0, 53], [5, 30, 3, 4], [1, 2, 0, 53]], np.int32)
    size = 17

    def make(seed):
        return {"frames": torch.from_numpy(_view_frames(seed))}

    _add(name="frame_var/5x37x53", entry="vsc_frame_var_u8", make=make, outputs={"out": ((h, w), F64)},
         call=lambda lib, p, inp, stream: lib.vsc_frame_var_u8(p["frames"], n, h, w, p["out"], stream),
         reference=lambda inp: {"out": np.stack(inp["frames"].numpy()).var(axis=0).sum(-1)}, tol={"out": None},
         cite="test_gpu_view_preprocess.py::test_frame_var_is_bit_identical_to_numpy", enqueue_only=True)

    def canny_ref(inp):
        fr = inp["frames"].numpy()
        out = np.zeros((h, w), np.uint16)
        for i, k in zip(*np.unique(idx, return_counts=True)):
            out += (canny_cpu.canny(fr[i]) > 0).astype(np.uint16) * np.uint16(k)
        return {"out": out}

    _add(name="canny_count/5x37x53", entry="vsc_canny_count_u8", make=make, outputs={"out": ((h, w), U16)},
         call=lambda lib, p, inp, stream: lib.vsc_canny_count_u8(p["frames"], n, _hp(idx), len(idx), h, w, 50.0, 400.0, p["out"], stream),
         reference=canny_ref, tol={"out": None}, cite="test_gpu_view_preprocess.py::test_canny_count_equals_the_restatement (tests/canny_cpu.py)",
         scratch=True)

    def resize_ref(inp):
        from PIL import Image
        fr = inp["frames"].numpy()
        out = np.empty((len(boxes) * n, size, size, 3), np.uint8)
        for b, (y0, y1, x0, x1) in enumerate(boxes):
            for i in range(n):
                out[b * n + i] = np.asarray(Image.fromarray(np.ascontiguousarray(fr[i, y0:y1, x0:x1])).resize((size, size), Image.BICUBIC))
        return {"out": out}

    _add(name="resize_bicubic/5x37x53_to17", entry="vsc_resize_bicubic_u8", make=make, outputs={"out": ((len(boxes) * n, size, size, 3), U8)},
         call=lambda lib, p, inp, stream: lib.vsc_resize_bicubic_u8(p["frames"], n, h, w, _hp(boxes), len(boxes), size, p["out"], stream),
         reference=resize_ref, tol={"out": None}, cite="test_gpu_view_preprocess.py::test_resize_is_bit_identical_to_pil", scratch=True)


_view_cases()


# ---- PCA fit: one case = a fresh handle, one update of n rows at ld = d + 3, the moments and the covariance read back ---------------
def _pca_case(d, n=129):
    ld = d + 3
    U = 2.0 ** -52

    def make(seed):
        buf = synth.normalish(seed * 100 + 7000 + d, (n, ld)) * (1.0 + synth.uniform(seed + 3 * d, (1, ld), 0.0, 2.0))
        return {"x": torch.from_numpy(np.ascontiguousarray(buf, dtype=np.float32))}

    def call(lib, p, inp, stream):
        h = ctypes.c_void_p()
        rc = lib.vsc_pca_fit_create(d, ctypes.byref(h))
        if rc:
            return rc
        seen = ctypes.c_int64(-1)
        try:
            rc = (lib.vsc_pca_fit_update_f32(h, p["x"], n, ld, stream) or lib.vsc_pca_fit_moments_f64(h, p["sum"], p["s2"], ctypes.byref(seen), stream)
                  or lib.vsc_pca_fit_covariance_f64(h, p["mean"], p["cov"], stream))
            if not rc:
                torch.cuda.synchronize()       # the handle's partial-sum scratch goes with it
        finally:
            lib.vsc_pca_fit_destroy(h)
        return rc, {"h_n": np.array([seen.value], np.int64)}

    def reference(inp):
        import pca_contract
        x32 = inp["x"].numpy()[:, :d]
        x = x32.astype(np.float64)
        a = np.abs(x)
        mean, cov = pca_contract.covariance(np.ascontiguousarray(x32))
        s2_bound = 2 * n * U * (a.T @ a)
        return {"sum": (x.sum(axis=0), 2 * n * U * a.sum(axis=0)), "s2": (x.T @ x, s2_bound), "mean": (mean, 2 * U * a.sum(axis=0)),
                "cov": (cov, s2_bound / (n - 1)), "h_n": np.array([n], np.int64)}

    def relations(out, inp):
        assert torch.equal(out["s2"], out["s2"].t()) and torch.equal(out["cov"], out["cov"].t()), "S2 / covariance not symmetric bit for bit"

    _add(name=f"pca_fit/d{d}_n{n}_ld{ld}", entry=("vsc_pca_fit_update_f32", "vsc_pca_fit_moments_f64", "vsc_pca_fit_covariance_f64"),
         make=make, outputs={"sum": ((d,), F64), "s2": ((d, d), F64), "mean": ((d,), F64), "cov": ((d, d), F64)}, call=call,
         reference=reference, tol={"sum": "bound", "s2": "bound", "mean": "bound", "cov": "bound", "h_n": None},
         cite="test_gpu_pca_fit.py::test_moments_match_float64_numpy / ::test_common_offset_covariance (2 n 2^-52 |X|^T |X|)",
         relations=relations)


_pca_case(16)
_pca_case(80)


# ======================================================================================================================
# Matching-track CNN layers (tests/test_gpu_cnn.py): NHWC fp32.  One convolution per kernel family, at that family's
# smallest parameter row.
# ======================================================================================================================
ACT = {None: 0, "relu": 1, "hard_swish": 2, "hard_sigmoid": 3}
ACT_FN = {None: lambda v: v, "relu": F.relu, "hard_swish": F.hardswish, "hard_sigmoid": F.hardsigmoid}


def _packed_k(cin, kh, kw):
    return (cin * kh * kw + 31) // 32 * 32


def _pack_weight(w):
    """torch [cout, cin, kh, kw] -> [cout, packed_k] in (kh, kw, cin) order, rows zero-padded (vsc_conv_pack_weight_f32 on the host)"""
    cout, cin, kh, kw = w.shape
    out = torch.zeros(cout, _packed_k(cin, kh, kw))
    out[:, : cin * kh * kw] = w.permute(0, 2, 3, 1).reshape(cout, -1)
    return out


def _conv_case(tag, n, h, w, cin, cout, k, stride, act, res, f64=False):
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1

    def make(seed):
        rng = np.random.RandomState(seed * 1000 + n * 100 + cin)
        wt = torch.from_numpy((rng.randn(cout, cin, k, k) / np.sqrt(cin * k * k)).astype(np.float32))
        d = {"x": torch.from_numpy(rng.randn(n, h, w, cin).astype(np.float32)), "wp": _pack_weight(wt),
             "b": torch.from_numpy(rng.randn(cout).astype(np.float32) * 0.1)}
        if res:
            d["res"] = torch.from_numpy(rng.randn(n, ho, wo, cout).astype(np.float32))
        return d

    def call(lib, p, inp, stream):
        return lib.vsc_conv2d_f32(p["x"], n, h, w, cin, cin, p["wp"], p["b"], cout, k, k, stride, pad, p.get("res"), cout, ACT[act], p["out"],
                                  cout, stream)

    def reference(inp):
        t = torch.float64 if f64 else torch.float32
        wt = inp["wp"][:, : cin * k * k].reshape(cout, k, k, cin).permute(0, 3, 1, 2)
        y = F.conv2d(inp["x"].to(t).permute(0, 3, 1, 2), wt.to(t), inp["b"].to(t), stride=stride, padding=pad)
        if res:
            y = y + inp["res"].to(t).permute(0, 3, 1, 2)
        return {"out": ACT_FN[act](y).permute(0, 2, 3, 1).contiguous()}

    _add(name=f"conv2d/{tag}/{n}x{h}x{w}_{cin}to{cout}_k{k}s{stride}", entry="vsc_conv2d_f32", make=make,
         outputs={"out": ((n, ho, wo, cout), F32)}, call=call, reference=reference, tol={"out": (0, 2e-5) if f64 else (1e-5, 2e-5)},
         cite="test_gpu_cnn.py::test_conv2d_matches_torch and the per-kernel tests behind it (atol 2e-5, rtol 1e-5; 2e-5 against float64 "
              "for the split-bf16 kernels)", enqueue_only=True, scratch=True)


_conv_case("stem", 1, 5, 4, 3, 8, 3, 2, "relu", False)                      # conv_stem3_kernel
_conv_case("stem_ragged", 2, 9, 7, 3, 16, 3, 2, "hard_swish", False)
_conv_case("tile_res", 1, 16, 16, 18, 18, 3, 1, "relu", True)               # cin % 4 != 0: the fp32 tile kernels on a patch matrix
_conv_case("expand64", 3, 5, 6, 64, 256, 1, 1, "relu", True)                # conv1x1_expand64_kernel
_conv_case("implicit_s2", 2, 12, 10, 36, 72, 3, 2, None, False)             # implicit gather, stride 2
_conv_case("5x5", 2, 7, 7, 24, 8, 5, 1, "hard_sigmoid", False)
_conv_case("direct_x3", 1, 5, 3, 20, 18, 3, 1, "relu", False, f64=True)     # conv3x3_direct_x3_kernel, an image smaller than one tile
_conv_case("direct_x3_ragged", 3, 21, 45, 20, 20, 3, 1, "relu", True, f64=True)
_conv_case("pointwise_stream", 48, 40, 40, 16, 72, 1, 1, "relu", False)     # conv1x1_stream_kernel
_conv_case("tap_x3", 4, 128, 128, 64, 64, 3, 1, "relu", False, f64=True)    # conv3x3_tap_x3_kernel: 65 536 pixels is its threshold
_conv_case("x3_gemm", 5, 47, 39, 144, 72, 3, 1, None, False, f64=True)      # conv_x3_gemm_kernel, ragged last pixel tile


def _cnn_small_cases():
    # depthwise
    def dw(c, k, stride, n, h, w, tag):
        pad = k // 2
        ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1

        def make(seed):
            rng = np.random.RandomState(seed * 1000 + c)
            return {"x": torch.from_numpy(rng.randn(n, h, w, c).astype(np.float32)),
                    "w": torch.from_numpy(rng.randn(c, k * k).astype(np.float32) * 0.2), "b": torch.from_numpy(rng.randn(c).astype(np.float32))}

        def reference(inp):
            y = F.conv2d(inp["x"].permute(0, 3, 1, 2), inp["w"].reshape(c, 1, k, k), inp["b"], stride=stride, padding=pad, groups=c)
            return {"out": F.hardswish(y).permute(0, 2, 3, 1).contiguous()}

        _add(name=f"dwconv2d/{tag}/{n}x{h}x{w}x{c}_k{k}s{stride}", entry="vsc_dwconv2d_f32", make=make, outputs={"out": ((n, ho, wo, c), F32)},
             call=lambda lib, p, inp, stream: lib.vsc_dwconv2d_f32(p["x"], n, h, w, c, p["w"], p["b"], k, k, stride, pad, ACT["hard_swish"],
                                                                  p["out"], stream),
             reference=reference, tol={"out": (1e-5, 1e-5)}, cite="test_gpu_cnn.py::test_depthwise_pool_scale_upsample (atol 1e-5)",
             enqueue_only=True)

    dw(16, 3, 2, 2, 11, 9, "rows")
    dw(7, 5, 2, 2, 11, 9, "scalar")       # c % 4 != 0
    dw(16, 3, 1, 3, 6, 7, "small")        # dwconv_small_kernel

    # squeeze-excite in one launch
    n, h, w, c, cr = 2, 7, 9, 96, 24

    def se_make(seed):
        rng = np.random.RandomState(seed * 1000 + 9)
        return {"x": torch.from_numpy(rng.randn(n, h, w, c).astype(np.float32)),
                "w1": _pack_weight(torch.from_numpy((rng.randn(cr, c, 1, 1) / np.sqrt(c)).astype(np.float32))),
                "b1": torch.from_numpy(rng.randn(cr).astype(np.float32) * 0.1),
                "w2": _pack_weight(torch.from_numpy((rng.randn(c, cr, 1, 1) / np.sqrt(cr)).astype(np.float32))),
                "b2": torch.from_numpy(rng.randn(c).astype(np.float32) * 0.1)}

    def se_ref(inp):
        xt = inp["x"].permute(0, 3, 1, 2)
        g = F.relu(F.conv2d(xt.mean((2, 3), keepdim=True), inp["w1"][:, :c].reshape(cr, c, 1, 1), inp["b1"]))
        g = F.hardsigmoid(F.conv2d(g, inp["w2"][:, :cr].reshape(c, cr, 1, 1), inp["b2"]))
        return {"x": (xt * g).permute(0, 2, 3, 1).contiguous()}

    _add(name=f"se_block/{n}x{h}x{w}x{c}_r{cr}", entry="vsc_se_block_f32", make=se_make, outputs={}, inout=("x",),
         call=lambda lib, p, inp, stream: lib.vsc_se_block_f32(p["x"], n, h * w, c, p["w1"], p["b1"], cr, p["w2"], p["b2"], ACT["relu"],
                                                              ACT["hard_sigmoid"], stream),
         reference=se_ref, tol={"x": (1e-5, 1e-5)}, cite="test_gpu_cnn.py::test_squeeze_excite_one_launch_equals_the_four_launch_form",
         enqueue_only=True)

    # nearest upsampling into a channel window, accumulating
    def up_make(seed):
        rng = np.random.RandomState(seed * 1000 + 1)
        return {"src": torch.from_numpy(rng.randn(2, 3, 4, 18).astype(np.float32)), "out": torch.from_numpy(rng.randn(2, 12, 16, 30).astype(np.float32))}

    def up_ref(inp):
        want = inp["out"].clone()
        want[..., 5:23] = F.relu(want[..., 5:23] + F.interpolate(inp["src"].permute(0, 3, 1, 2), scale_factor=4, mode="nearest").permute(0, 2, 3, 1))
        return {"out": want}

    _add(name="upsample_add/2x12x16_c18_into30", entry="vsc_upsample_add_f32", make=up_make, outputs={}, inout=("out",),
         call=lambda lib, p, inp, stream: lib.vsc_upsample_add_f32(p["src"], 2, 12, 16, 18, 4, p["out"], 30, 5, 1, ACT["relu"], stream),
         reference=up_ref, tol={"out": None}, cite="test_gpu_cnn.py::test_depthwise_pool_scale_upsample (torch.equal)", enqueue_only=True)

    # one HRNet fuse node
    fn, fh, fw, fc = 2, 16, 24, 20

    def sum_make(seed):
        rng = np.random.RandomState(seed * 1000 + 5)
        d = {"base": torch.from_numpy(rng.randn(fn, fh, fw, fc).astype(np.float32))}
        for i, f in enumerate((1, 2, 8)):
            d[f"s{i}"] = torch.from_numpy(rng.randn(fn, fh // f, fw // f, fc).astype(np.float32))
        return d

    def sum_ref(inp):
        want = inp["base"].clone()
        for i, f in enumerate((1, 2, 8)):
            want = want + F.interpolate(inp[f"s{i}"].permute(0, 3, 1, 2), scale_factor=f, mode="nearest").permute(0, 2, 3, 1)
        return {"out": F.relu(want)}

    _add(name="upsample_sum/2x16x24x20_3_terms", entry="vsc_upsample_sum_f32", make=sum_make, outputs={"out": ((fn, fh, fw, fc), F32)},
         call=lambda lib, p, inp, stream: lib.vsc_upsample_sum_f32(p["base"], fc, p["s0"], 1, p["s1"], 2, p["s2"], 8, fn, fh, fw, fc, ACT["relu"],
                                                                  p["out"], fc, stream),
         reference=sum_ref, tol={"out": None}, cite="test_gpu_cnn.py::test_upsample_sum_is_the_chain_of_upsample_adds (torch.equal)",
         enqueue_only=True)

    # global average pool, channel scale
    _add(name="global_avgpool/3x30x70", entry="vsc_global_avgpool_f32",
         make=lambda seed: {"x": torch.from_numpy(np.random.RandomState(seed).randn(3, 30, 70).astype(np.float32))},
         outputs={"out": ((3, 70), F32)}, call=lambda lib, p, inp, stream: lib.vsc_global_avgpool_f32(p["x"], 3, 30, 70, p["out"], stream),
         reference=lambda inp: {"out": inp["x"].mean(1)}, tol={"out": (1e-5, 1e-6)},
         cite="test_gpu_cnn.py::test_depthwise_pool_scale_upsample (torch.allclose atol 1e-6)", enqueue_only=True)

    def scale_make(seed):
        rng = np.random.RandomState(seed + 77)
        return {"x": torch.from_numpy(rng.randn(3, 30, 70).astype(np.float32)), "scale": torch.from_numpy(rng.rand(3, 70).astype(np.float32))}

    _add(name="channel_scale/3x30x70", entry="vsc_channel_scale_f32", make=scale_make, outputs={}, inout=("x",),
         call=lambda lib, p, inp, stream: lib.vsc_channel_scale_f32(p["x"], p["scale"], 3, 30, 70, stream),
         reference=lambda inp: {"x": inp["x"] * inp["scale"][:, None, :]}, tol={"x": (1e-5, 1e-5)},
         cite="test_gpu_cnn.py::test_squeeze_excite_one_launch_equals_the_four_launch_form (the four-launch form ends in it; atol, rtol 1e-5)",
         enqueue_only=True)

    # the weight packer: 27 -> 32 floats per row, and a whole multiple
    for cout, kk in ((16, 27), (5, 64)):
        def pk_ref(inp, kk=kk, cout=cout):
            out = torch.zeros(cout, (kk + 31) // 32 * 32)
            out[:, :kk] = inp["w"]
            return {"out": out}

        _add(name=f"conv_pack_weight/{cout}x{kk}", entry="vsc_conv_pack_weight_f32",
             make=lambda seed, kk=kk, cout=cout: {"w": torch.from_numpy(np.random.RandomState(seed + kk).randn(cout, kk).astype(np.float32))},
             outputs={"out": ((cout, (kk + 31) // 32 * 32), F32)},
             call=lambda lib, p, inp, stream, kk=kk, cout=cout: lib.vsc_conv_pack_weight_f32(p["w"], p["out"], cout, kk, stream),
             reference=pk_ref, tol={"out": None}, cite="include/vsc_hip.h (rows zero-padded to a multiple of 32 floats: a copy)",
             enqueue_only=True)


_cnn_small_cases()


# ======================================================================================================================
# Whole encoders: presets tiny / tiny_swin, max_batch = 3, n = 7 (three chunks: with lanes = 2 the fork / join events).
# Reference: the fp32 oracles at the suite's descriptor tolerance (tests/test_gpu_encoder.py DESC_L2_ATOL = 1e-3).
# ======================================================================================================================
ENC_N, ENC_MAX_BATCH = 7, 3


def _vit_case(tag, entry, lanes, fuse_ln, u8=False, debug=False):
    from oracle import vit_oracle
    from vsc_hip.config import get_config
    cfg = get_config("tiny")
    weights = synth.encoder_weights(7, cfg)
    mean = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    std = (ctypes.c_float * 3)(0.5, 0.5, 0.5)

    def make(seed):
        if u8:
            return {"frames": torch.from_numpy(synth.uniform(seed + 17, (ENC_N, cfg.image_size, cfg.image_size, 3), 0.0, 256.0).astype(np.uint8))}
        return {"frames": torch.from_numpy(synth.frames(seed + 11, ENC_N, cfg))}

    def open_(lib):
        from vsc_hip.encoder import HipEncoder
        return HipEncoder(cfg, weights, max_batch=ENC_MAX_BATCH, l2_normalize=True, lanes=lanes, fuse_ln=fuse_ln)

    def call(lib, p, inp, stream):
        h = p["ctx"]._h
        if u8:
            return lib.vsc_encoder_forward_u8(h, p["frames"], ENC_N, mean, std, p["desc"], stream)
        if debug:
            return lib.vsc_encoder_forward_debug(h, p["frames"], ENC_N, p["desc"], p["tokens"], stream)
        return lib.vsc_encoder_forward(h, p["frames"], ENC_N, p["desc"], stream)

    def reference(inp):
        x = inp["frames"]
        if u8:
            x = (x.permute(0, 3, 1, 2).float() / 255.0 - 0.5) / 0.5
        wt = {k: torch.from_numpy(v) for k, v in weights.items()}
        with torch.no_grad():
            out = {"desc": vit_oracle.descriptors(wt, cfg, x)}
            if debug:
                out["tokens"] = vit_oracle.encode_tokens(wt, cfg, x)
        return out

    outs = {"desc": ((ENC_N, cfg.desc_dim), F32)}
    if debug:
        outs["tokens"] = ((ENC_N, cfg.tokens, cfg.width), F32)
    _add(name=f"encoder/{tag}", entry=entry, make=make, outputs=outs, call=call, reference=reference,
         tol={"desc": (0, 1e-3), "tokens": (0, 0.08)},
         cite="test_gpu_encoder.py (DESC_L2_ATOL = 1e-3 against oracle/vit_oracle.py; tokens 0.08 as ::test_encoder_matches_golden)",
         enqueue_only=not debug, open=open_)


_vit_case("forward_lanes1", "vsc_encoder_forward", 1, 0)
_vit_case("forward_lanes2", "vsc_encoder_forward", 2, 0)
_vit_case("forward_lanes2_fuse_ln", "vsc_encoder_forward", 2, 1)
_vit_case("forward_u8_lanes2", "vsc_encoder_forward_u8", 2, 0, u8=True)
_vit_case("forward_debug_lanes2", "vsc_encoder_forward_debug", 2, 0, debug=True)


def _swin_case(tag, entry, u8=False, debug=False):
    from oracle import swin_oracle
    from vsc_hip.swin_config import get_swin_config
    cfg = get_swin_config("tiny_swin")
    weights = synth.swin_weights(9, cfg)
    mean = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    std = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    last = cfg.stages - 1

    def make(seed):
        if u8:
            return {"frames": torch.from_numpy(synth.uniform(seed + 19, (ENC_N, cfg.image_size, cfg.image_size, 3), 0.0, 256.0).astype(np.uint8))}
        return {"frames": torch.from_numpy(synth.swin_frames(seed + 10, ENC_N, cfg))}

    def open_(lib):
        from vsc_hip.swin_encoder import SwinHipEncoder
        return SwinHipEncoder(cfg, weights, max_batch=ENC_MAX_BATCH, l2_normalize=True)

    def call(lib, p, inp, stream):
        h = p["ctx"]._h
        if u8:
            return lib.vsc_swin_forward_u8(h, p["frames"], ENC_N, mean, std, p["desc"], stream)
        if debug:
            return lib.vsc_swin_forward_debug(h, p["frames"], ENC_N, p["desc"], p["tokens"], stream)
        return lib.vsc_swin_forward(h, p["frames"], ENC_N, p["desc"], stream)

    def reference(inp):
        x = inp["frames"]
        if u8:
            x = (x.permute(0, 3, 1, 2).float() / 255.0 - 0.5) / 0.5
        wt = {k: torch.from_numpy(v) for k, v in weights.items()}
        with torch.no_grad():
            out = {"desc": swin_oracle.descriptors(wt, cfg, x)}
            if debug:
                out["tokens"] = swin_oracle.encode_tokens(wt, cfg, x)
        return out

    outs = {"desc": ((ENC_N, cfg.out_dim), F32)}
    if debug:
        outs["tokens"] = ((ENC_N, cfg.resolution(last) ** 2, cfg.dim(last)), F32)
    _add(name=f"swin/{tag}", entry=entry, make=make, outputs=outs, call=call, reference=reference, tol={"desc": (0, 1e-3), "tokens": (0, 0.1)},
         cite="test_gpu_swin.py::test_swin_encoder_vs_oracle_and_batching (atol 1e-3 against oracle/swin_oracle.py; tokens 0.1 as "
              "::test_swin_encoder_matches_golden)", enqueue_only=not debug, open=open_)


_swin_case("forward", "vsc_swin_forward")
_swin_case("forward_u8", "vsc_swin_forward_u8", u8=True)
_swin_case("forward_debug", "vsc_swin_forward_debug", debug=True)


# ======================================================================================================================
# Comparison helpers shared by the CPU and the GPU test
# ======================================================================================================================
def tensor(v):
    """reference value -> CPU torch tensor"""
    return v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))


def raw_bytes(t):
    """a tensor's bytes, one row per element: [numel, itemsize] uint8"""
    t = t.contiguous()
    return t.reshape(-1).view(torch.uint8).reshape(-1, t.element_size())


def same_bits(a, b):
    a, b = tensor(a), tensor(b)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(raw_bytes(a), raw_bytes(b))


def keep_mask(case, inp, name, shape):
    """bool tensor of `shape`: True where the header says the call writes the element"""
    left = case.leave(inp).get(name) if case.leave else None
    if left is None:
        return torch.ones(shape, dtype=torch.bool)
    return ~tensor(np.asarray(left, bool)).reshape(shape)


def check_against_reference(case, inp, out, ref=None):
    """`out`: name -> CPU tensor (device outputs) or numpy array (host results).  Every written element within the case's tolerance
    of the reference, then the relations between outputs."""
    ref = case.reference(inp) if ref is None else ref
    for name, want in ref.items():
        tol = case.tol[name]
        got = tensor(out[name])
        bound = None
        if tol == "bound":
            want, bound = want
            bound = tensor(bound).reshape(got.shape)
        want = tensor(want).reshape(got.shape)
        keep = keep_mask(case, inp, name, got.shape)
        if tol is None:
            if want.dtype != got.dtype:
                want = want.to(got.dtype)
            bad = (raw_bytes(got) != raw_bytes(want)).any(dim=1).reshape(got.shape) & keep
            assert not bool(bad.any()), (f"{case.name}: {name} differs from the reference in {int(bad.sum())} of {int(keep.sum())} elements, "
                                         f"first at {bad.nonzero()[0].tolist()}")
            continue
        g, w = got.double()[keep], want.double()[keep]
        assert bool(torch.isfinite(g).all()), f"{case.name}: {name} holds non-finite values"
        if bound is not None:
            lim = bound.double()[keep]
        else:
            lim = tol[1] + tol[0] * w.abs()
        err = (g - w).abs()
        bad = err > lim
        assert not bool(bad.any()), (f"{case.name}: {name} outside its tolerance {tol} in {int(bad.sum())} of {g.numel()} elements, "
                                     f"largest error {float(err.max()):.3e}, largest error / limit {float((err / lim.clamp_min(1e-300)).max()):.3f}")
    missing = [n for n in case.written() if n not in ref and not case.relations]
    assert not missing, f"{case.name}: no reference and no relation covers {missing}"
    if case.relations:
        case.relations({k: tensor(v) for k, v in out.items()}, inp)
