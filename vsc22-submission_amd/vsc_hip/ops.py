"""Thin torch-tensor wrappers over the C ABI building blocks (used by the parity
tests and by vsc/index.py).  torch here is device memory + streams only."""
from __future__ import annotations

import torch

from . import _lib
from ._lib import check, current_stream, ptr


_PRECISION = "bf16"


class operands:
    """with ops.operands("fp16"): ...  -- the kernel-level wrappers below then call libvsc_hip_f16.so and their 16-bit tensors are
    torch.float16 (vsc_operand_dtype, include/vsc_hip.h).  Default: the bf16 library."""

    def __init__(self, precision: str):
        assert precision in _lib.LIB_PATHS, precision
        self.precision, self._saved = precision, None

    def __enter__(self):
        global _PRECISION
        self._saved, _PRECISION = _PRECISION, self.precision
        return self

    def __exit__(self, *exc):
        global _PRECISION
        _PRECISION = self._saved
        return False


def lp_dtype():
    """torch dtype of the current library's 16-bit operands"""
    return torch.float16 if _PRECISION == "fp16" else torch.bfloat16


def _rd():
    return _lib.require_device(_PRECISION)


def _dev(t: torch.Tensor, dtype) -> torch.Tensor:
    assert t.is_cuda, "operand must live on the GPU"
    return t.to(dtype).contiguous()


def gemm_bf16(a, w, bias=None, *, epilogue=_lib.EPI_BF16, aux=None, tokens=0, out=None):
    """out = epi(a @ w.T + bias); a [M,K] bf16, w [N,K] bf16."""
    lib = _rd()
    a, w = _dev(a, lp_dtype()), _dev(w, lp_dtype())
    m, k = a.shape
    n = w.shape[0]
    assert w.shape[1] == k
    bias = None if bias is None else _dev(bias, torch.float32)
    aux = None if aux is None else _dev(aux, torch.float32)
    if out is None:
        if epilogue in (_lib.EPI_BF16, _lib.EPI_GELU_BF16, _lib.EPI_QGELU_BF16):
            out = torch.empty((m, n), dtype=lp_dtype(), device=a.device)
        elif epilogue in (_lib.EPI_RESADD_F32, _lib.EPI_F32):
            out = torch.empty((m, n), dtype=torch.float32, device=a.device)
        else:
            frames = m // (tokens - 1)
            out = torch.zeros((frames * tokens, n), dtype=torch.float32, device=a.device)
    check(lib.vsc_gemm_bf16(ptr(a), ptr(w), ptr(bias), ptr(aux), ptr(out), m, n, k, epilogue, tokens,
                            current_stream()))
    return out


GEMM_KERNELS = ("V1", "V2_A", "V2_B", "V2_C", "V2_D", "V3", "V4")


def gemm_plan(m: int, n: int, k: int, epilogue=_lib.EPI_BF16) -> dict:
    """the plan gemm_bf16 would execute for this shape now (csrc/gemm_plan.h): kernel (a name of GEMM_KERNELS), tiles_m, tiles_n,
    group_n, grid, block, lds_bytes.  Launches nothing."""
    import ctypes
    out = (ctypes.c_int32 * 8)()
    check(_rd().vsc_gemm_plan(m, n, k, epilogue, out))
    keys = ("kernel", "tiles_m", "tiles_n", "group_n", "grid", "block", "lds_bytes")
    plan = dict(zip(keys, out[:7]))
    plan["kernel"] = GEMM_KERNELS[plan["kernel"]]
    return plan


def attention_bf16(qkv, frames: int, tokens: int, heads: int):
    lib = _rd()
    qkv = _dev(qkv, lp_dtype())
    assert qkv.shape == (frames * tokens, 3 * heads * 64)
    out = torch.empty((frames * tokens, heads * 64), dtype=lp_dtype(), device=qkv.device)
    check(lib.vsc_attention_bf16(ptr(qkv), ptr(out), frames, tokens, heads, current_stream()))
    return out


def attention_stream_bf16(qkv, frames: int, tokens: int, heads: int):
    """attention_bf16 at any token count up to _lib.ATTENTION_STREAM_MAX_TOKENS: key blocks of _lib.ATTENTION_STREAM_KEY_BLOCK and
    an online softmax (vsc_attention_stream_bf16)."""
    lib = _rd()
    qkv = _dev(qkv, lp_dtype())
    assert qkv.shape == (frames * tokens, 3 * heads * 64)
    out = torch.empty((frames * tokens, heads * 64), dtype=lp_dtype(), device=qkv.device)
    check(lib.vsc_attention_stream_bf16(current_stream(), ptr(qkv), ptr(out), frames, tokens, heads))
    return out


def attention_f32(qkv, tokens: int, heads: int, head_dim: int, seqs: int = 1, row_offsets=None, out=None):
    """fp32 softmax(q k^T / sqrt(head_dim)) v of the video-score head; qkv [rows, 3 * heads * head_dim] float32 as q | k | v.
    `seqs` sequences of `tokens` rows back to back (vsc_attention_f32 / vsc_attention_f32_batch), or, with row_offsets (int32
    [seqs + 1] on the device), sequences of different lengths with `tokens` the longest one (vsc_attention_f32_varlen).
    out: an [rows, heads * head_dim] float32 device tensor to write into (rows outside the sequences are left alone)."""
    lib = _rd()
    qkv = _dev(qkv, torch.float32)
    width = heads * head_dim
    assert qkv.dim() == 2 and qkv.shape[1] == 3 * width
    if out is None:
        out = torch.empty((qkv.shape[0], width), dtype=torch.float32, device=qkv.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (qkv.shape[0], width)
    if row_offsets is not None:
        row_offsets = _dev(row_offsets, torch.int32)
        assert row_offsets.shape == (seqs + 1,)
        check(lib.vsc_attention_f32_varlen(ptr(qkv), ptr(out), ptr(row_offsets), seqs, tokens, heads, head_dim, current_stream()))
        return out
    assert qkv.shape[0] == seqs * tokens
    if seqs == 1:
        check(lib.vsc_attention_f32(ptr(qkv), ptr(out), tokens, heads, head_dim, current_stream()))
    else:
        check(lib.vsc_attention_f32_batch(ptr(qkv), ptr(out), tokens, heads, head_dim, seqs, current_stream()))
    return out


def layernorm(x, gamma, beta, eps: float, out_f32: bool = False):
    lib = _rd()
    x, gamma, beta = (_dev(t, torch.float32) for t in (x, gamma, beta))
    rows, width = x.shape
    out = torch.empty((rows, width), dtype=torch.float32 if out_f32 else lp_dtype(), device=x.device)
    check(lib.vsc_layernorm_f32(ptr(x), ptr(gamma), ptr(beta), ptr(out), rows, width, eps,
                                int(out_f32), current_stream()))
    return out


def gemm_resadd_ln_bf16(a, w, bias, x, gamma, beta, eps: float, y=None, rows=None):
    """x[:rows] += a[:rows] @ w.T + bias IN PLACE (float32), y[:rows] = LayerNorm(x[:rows]) * gamma + beta in the operand type:
    one persistent launch with the LayerNorm as its tail where that form exists, otherwise GEMM + LayerNorm launches -- the same
    bits (gemm_resadd_ln_last_path() says which ran).  rows < len(x): the rows behind are left alone.  -> y"""
    lib = _rd()
    assert a.dtype == lp_dtype() and w.dtype == lp_dtype() and x.dtype == torch.float32 and x.is_contiguous() and a.is_contiguous()
    m = a.shape[0] if rows is None else rows
    k, n = a.shape[1], w.shape[0]
    assert w.shape[1] == k and x.shape[1] == n and m <= a.shape[0] and m <= x.shape[0]
    bias = None if bias is None else _dev(bias, torch.float32)
    gamma, beta = _dev(gamma, torch.float32), _dev(beta, torch.float32)
    if y is None:
        y = torch.empty((x.shape[0], n), dtype=lp_dtype(), device=x.device)
    assert y.dtype == lp_dtype() and y.is_contiguous() and y.shape[0] >= m
    check(lib.vsc_gemm_resadd_ln_bf16(ptr(a), ptr(w.contiguous()), ptr(bias), ptr(x), ptr(gamma), ptr(beta), ptr(y), m, n, k, eps,
                                      current_stream()))
    return y


def gemm_resadd_ln_last_path() -> int:
    """1: the last residual GEMM + LayerNorm ran as one launch with the LayerNorm tail, 2: as two launches"""
    return int(_rd().vsc_gemm_resadd_ln_last_path())


def patchify_bf16(frames, patch: int, kpad: int):
    lib = _rd()
    frames = _dev(frames, torch.float32)
    n, c, h, w = frames.shape
    assert h == w
    g = h // patch
    out = torch.empty((n * g * g, kpad), dtype=lp_dtype(), device=frames.device)
    check(lib.vsc_patchify_bf16(ptr(frames), ptr(out), n, c, h, patch, kpad, current_stream()))
    return out


def l2_normalize_(x):
    """In place, sklearn.preprocessing.normalize semantics."""
    lib = _rd()
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2
    if x.shape[0]:
        check(lib.vsc_l2_normalize_f32(ptr(x), x.shape[0], x.shape[1], current_stream()))
    return x


def _rows_f32(t, what: str):
    """(pointer, rows, width, row stride) of a float32 [n, d] device tensor whose rows are dense: the score-normalisation entries
    take a row stride >= the width, so a column slice of a wider tensor passes without a copy."""
    assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] >= 1, f"{what}: a float32 [n, d] device tensor"
    n, d = t.shape
    assert d == 1 or t.stride(1) == 1, f"{what}: rows must be dense"
    ld = t.stride(0) if n > 1 else d
    assert ld >= d, f"{what}: row stride {ld} below the width {d}"
    return _lib.c_void_p(t.data_ptr()), n, d, ld


_score_norm_handles = {}


def score_norm_handle():
    """The vsc_score_norm handle of the current library on the current stream (made on first use, kept for the process: it is the
    stream and owns no device memory)."""
    import ctypes
    lib = _rd()
    stream = current_stream()
    key = (_PRECISION, stream.value or 0)
    if key not in _score_norm_handles:
        h = ctypes.c_void_p()
        check(lib.vsc_score_norm_create(stream, ctypes.byref(h)))
        _score_norm_handles[key] = h
    return _score_norm_handles[key]


def column_var(x):
    """numpy's x.var(axis=0) of float32 rows [n, d] (row stride >= d), bit for bit (vsc_column_var_f32) -> float32 [d] on the device."""
    lib = _rd()
    px, n, d, ld = _rows_f32(x, "column_var")
    if n < 1:
        raise ValueError("column_var: the variance of no rows")
    var = torch.empty(d, dtype=torch.float32, device=x.device)
    check(lib.vsc_column_var_f32(score_norm_handle(), px, n, d, ld, ptr(var)))
    return var


def score_norm_rows(x, drop: int = -1, normalize: bool = True, append: int = 0, last=None, out=None):
    """concatenate([l2_normalize(delete(x, drop, axis=1)), last], axis=1) into a second buffer (vsc_score_norm_rows_f32): drop -1 keeps
    every column, append 0 / 1 / 2 = no column / the constant 1.0f / last[row].  out: a float32 [n, width] device tensor (row stride
    >= width) that does not overlap x; allocated when None."""
    lib = _rd()
    px, n, d, ldx = _rows_f32(x, "score_norm_rows: x")
    width = d - (drop >= 0) + (append != 0)
    if append == 2:
        assert last is not None and last.is_cuda and last.dtype == torch.float32 and last.is_contiguous() and last.numel() == n
    if out is None:
        out = torch.empty((n, width), dtype=torch.float32, device=x.device)
    po, no, wo, ldo = _rows_f32(out, "score_norm_rows: out")
    assert (no, wo) == (n, width), f"score_norm_rows: out is {tuple(out.shape)}, not {(n, width)}"
    check(lib.vsc_score_norm_rows_f32(score_norm_handle(), px, n, d, ldx, int(drop), int(bool(normalize)), int(append),
                                      ptr(last) if append == 2 else None, po, ldo))
    return out


def score_norm_bias(topk, nk: int, beta: float, gate=None):
    """-beta * topk[:, :nk].mean(axis=1) with numpy's bits (vsc_score_norm_bias_f32); gate: uint8 [nq] on the device, a non-zero entry
    makes the row -100.0f.  -> float32 [nq] on the device."""
    import numpy as np
    lib = _rd()
    pk, nq, width, ldk = _rows_f32(topk, "score_norm_bias")
    assert nk <= width, f"score_norm_bias: nk {nk} of {width} columns"
    if gate is not None:
        assert gate.is_cuda and gate.dtype == torch.uint8 and gate.is_contiguous() and gate.numel() == nq
    bias = torch.empty(nq, dtype=torch.float32, device=topk.device)
    check(lib.vsc_score_norm_bias_f32(score_norm_handle(), pk, nq, ldk, int(nk), float(np.float32(-beta)), ptr(gate), ptr(bias)))
    return bias


def knn_ip(q, r, k: int, ref_id_offset: int = 0, floor=None):
    """Exact inner-product top-k.  q [nq,d], r [nr,d] float32 on the GPU ->
    (scores [nq,k] float32 descending, ids [nq,k] int64).  Empty inputs follow
    faiss: nq == 0 -> empty outputs; nr == 0 -> all (-FLT_MAX, -1).
    floor [nq] float32: only references with <q, r> >= floor[q] (vsc_knn_ip_floor_f32; unused slots (-FLT_MAX, -1))."""
    lib = _rd()
    q, r = _dev(q, torch.float32), _dev(r, torch.float32)
    nq, d = q.shape
    nr = r.shape[0]
    assert r.shape[1] == d, "query / reference dimension mismatch"
    scores = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    ids = torch.empty((nq, k), dtype=torch.int64, device=q.device)
    if nq == 0:
        return scores, ids
    if nr == 0:
        scores.fill_(torch.finfo(torch.float32).min)
        ids.fill_(-1)
        return scores, ids
    if floor is not None:
        floor = _dev(floor, torch.float32)
        assert floor.shape == (nq,)
        check(lib.vsc_knn_ip_floor_f32(ptr(q), nq, ptr(r), nr, d, k, ref_id_offset, ptr(floor), ptr(scores), ptr(ids), current_stream()))
        return scores, ids
    check(lib.vsc_knn_ip_f32(ptr(q), nq, ptr(r), nr, d, k, ref_id_offset, ptr(scores), ptr(ids),
                             current_stream()))
    return scores, ids


def knn_merge_parts(scores, ids):
    """scores / ids [parts, nq, k]: per-shard results of knn_ip (each with its ref_id_offset) -> the k best of the union, in the
    search's order (score descending, equal scores by ascending id)."""
    lib = _rd()
    scores, ids = _dev(scores, torch.float32), _dev(ids, torch.int64)
    parts, nq, k = scores.shape
    assert ids.shape == scores.shape and 1 <= parts <= 64
    out_s = torch.empty((nq, k), dtype=torch.float32, device=scores.device)
    out_i = torch.empty((nq, k), dtype=torch.int64, device=scores.device)
    check(lib.vsc_knn_merge_parts_f32(ptr(scores), ptr(ids), parts, nq, k, ptr(out_s), ptr(out_i), current_stream()))
    return out_s, out_i


def range_search_ip(q, r, radius: float, ref_id_offset: int = 0, capacity: int = 1 << 20):
    """All pairs with <q, r> > radius.  -> (lims [nq+1] int64, scores, ids), hits of query i in
    lims[i]:lims[i+1], ascending reference id (faiss range_search layout)."""
    import ctypes
    lib = _rd()
    q, r = _dev(q, torch.float32), _dev(r, torch.float32)
    nq, d = q.shape
    nr = r.shape[0]
    assert r.shape[1] == d, "query / reference dimension mismatch"
    lims = torch.zeros(nq + 1, dtype=torch.int64, device=q.device)
    empty = (lims, torch.empty(0, dtype=torch.float32, device=q.device),
             torch.empty(0, dtype=torch.int64, device=q.device))
    if nq == 0 or nr == 0:
        return empty
    total = ctypes.c_int64(0)
    while True:
        scores = torch.empty(capacity, dtype=torch.float32, device=q.device)
        ids = torch.empty(capacity, dtype=torch.int64, device=q.device)
        check(lib.vsc_range_search_ip_f32(ptr(q), nq, ptr(r), nr, d, float(radius), ref_id_offset, ptr(lims),
                                          ptr(scores), ptr(ids), capacity, ctypes.byref(total),
                                          current_stream()))
        if total.value <= capacity:
            return lims, scores[: total.value], ids[: total.value]
        capacity = int(total.value)


def range_count_ip(q, r, radius: float) -> int:
    """Number of pairs with <q, r> > radius: the counting pass of vsc_range_search_ip_f32 alone (capacity 0)."""
    import ctypes
    lib = _rd()
    q, r = _dev(q, torch.float32), _dev(r, torch.float32)
    nq, d = q.shape
    nr = r.shape[0]
    assert r.shape[1] == d, "query / reference dimension mismatch"
    if nq == 0 or nr == 0:
        return 0
    lims = torch.zeros(nq + 1, dtype=torch.int64, device=q.device)
    total = ctypes.c_int64(0)
    check(lib.vsc_range_search_ip_f32(ptr(q), nq, ptr(r), nr, d, float(radius), 0, ptr(lims), None, None, 0,
                                      ctypes.byref(total), current_stream()))
    return int(total.value)


def l2_augment(x, as_query: bool = False):
    """Augmented rows of the L2 search's sweep (vsc_l2_augment_f32): x [n, d] float32 on the GPU -> (aug [n, d + 2], norms [n] = |x|^2,
    max_norm [1] = the largest of them).  Bank rows [x, |x|^2, 1], or with as_query [2x, -1, -|x|^2].  Once per bank: the pair
    (aug, max_norm) is the `bank=` of knn_l2 / range_search_l2."""
    lib = _rd()
    x = _dev(x, torch.float32)
    n, d = x.shape
    aug = torch.empty((n, d + 2), dtype=torch.float32, device=x.device)
    norms = torch.empty(n, dtype=torch.float32, device=x.device)
    max_norm = torch.zeros(1, dtype=torch.float32, device=x.device)
    check(lib.vsc_l2_augment_f32(current_stream(), ptr(x) if n else None, n, d, int(bool(as_query)), ptr(aug) if n else None,
                                 ptr(norms) if n else None, ptr(max_norm)))
    return aug, norms, max_norm


def _l2_bank(bank, nr, d):
    if bank is None:
        return None, None
    aug, max_norm = bank
    assert aug.is_cuda and aug.dtype == torch.float32 and tuple(aug.shape) == (nr, d + 2), "bank: l2_augment's rows of these references"
    assert max_norm.is_cuda and max_norm.dtype == torch.float32 and max_norm.numel() == 1
    return ptr(aug) if nr else None, ptr(max_norm) if nr else None


def knn_l2(q, r, k: int, ref_id_offset: int = 0, bank=None):
    """Exact squared-L2 top-k (vsc_knn_l2_f32).  q [nq, d], r [nr, d] float32 on the GPU (plain rows) -> (distances [nq, k] float32
    ascending, ids [nq, k] int64; equal distances by ascending id, unused slots (FLT_MAX, -1)).  bank: (aug, max_norm) of
    l2_augment(r), or None: the bank is augmented for this call."""
    lib = _rd()
    q, r = _dev(q, torch.float32), _dev(r, torch.float32)
    nq, d = q.shape
    nr = r.shape[0]
    assert r.shape[1] == d, "query / reference dimension mismatch"
    dist = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    ids = torch.empty((nq, k), dtype=torch.int64, device=q.device)
    aug, max_norm = _l2_bank(bank, nr, d)
    check(lib.vsc_knn_l2_f32(current_stream(), ptr(q) if nq else None, nq, ptr(r) if nr else None, nr, d, k, ref_id_offset, aug, max_norm,
                             ptr(dist) if nq else None, ptr(ids) if nq else None))
    return dist, ids


def knn_l2_last_path():
    """Query rows of the last knn_l2 call by path: (certified at the first probe, at a wider probe, direct) -- vsc_knn_l2_last_path."""
    import ctypes
    out = (ctypes.c_int64 * 3)()
    check(_rd().vsc_knn_l2_last_path(out))
    return tuple(int(v) for v in out)


def range_search_l2(q, r, radius: float, ref_id_offset: int = 0, capacity: int = 1 << 20, bank=None):
    """All pairs with squared L2 distance < radius (vsc_range_search_l2_f32).  -> (lims [nq+1] int64, distances, ids), hits of query i
    in lims[i]:lims[i+1], ascending reference id.  capacity 0: count only -> (lims, empty, empty) with lims[-1] the total."""
    import ctypes
    lib = _rd()
    q, r = _dev(q, torch.float32), _dev(r, torch.float32)
    nq, d = q.shape
    nr = r.shape[0]
    assert r.shape[1] == d, "query / reference dimension mismatch"
    lims = torch.zeros(nq + 1, dtype=torch.int64, device=q.device)
    aug, max_norm = _l2_bank(bank, nr, d)
    total = ctypes.c_int64(0)
    count_only = capacity == 0
    while True:
        dist = torch.empty(capacity, dtype=torch.float32, device=q.device)
        ids = torch.empty(capacity, dtype=torch.int64, device=q.device)
        check(lib.vsc_range_search_l2_f32(current_stream(), ptr(q) if nq else None, nq, ptr(r) if nr else None, nr, d, float(radius),
                                          ref_id_offset, aug, max_norm, ptr(lims), ptr(dist) if capacity else None,
                                          ptr(ids) if capacity else None, capacity, ctypes.byref(total)))
        if total.value <= capacity or count_only:
            n = 0 if count_only else total.value
            return lims, dist[:n], ids[:n]
        capacity = int(total.value)


def range_count_l2(q, r, radius: float, bank=None) -> int:
    """Number of pairs with squared L2 distance < radius: vsc_range_search_l2_f32 with capacity 0."""
    lims, _, _ = range_search_l2(q, r, radius, capacity=0, bank=bank)
    return int(lims[-1].item())


GLOBAL_TOPK_TILE = 2048     # VSC_GLOBAL_TOPK_TILE (include/vsc_hip.h): entries per workgroup of the compaction passes


def global_topk(scores, ids, want: int, rows=None):
    """The min(want, valid) best entries of a probe, best first, equal scores in input order (vsc_global_topk_f32).
    scores float32 / ids int64 of one shape, on the GPU; entries with ids < 0 are padding.  rows: int64 like ids, or None: the
    row of an entry is its index along the first axis of a 2-d [nq, k] probe (its position, for a flat list).
    -> (rows, ids, scores), device tensors cut to the count; synchronises once, to read that count."""
    lib = _rd()
    scores, ids = _dev(scores, torch.float32), _dev(ids, torch.int64)
    assert scores.shape == ids.shape and scores.ndim in (1, 2), "scores / ids: one flat list or one [nq, k] probe"
    n = scores.numel()
    stride = scores.shape[1] if scores.ndim == 2 and rows is None else 1
    if rows is not None:
        rows = _dev(rows, torch.int64)
        assert rows.shape == ids.shape
    want = int(want)
    assert want >= 0 and n < 1 << 31
    cap = min(want, n)
    out_rows = torch.empty(cap, dtype=torch.int64, device=scores.device)
    out_ids = torch.empty(cap, dtype=torch.int64, device=scores.device)
    out_scores = torch.empty(cap, dtype=torch.float32, device=scores.device)
    count = torch.empty(1, dtype=torch.int64, device=scores.device)
    check(lib.vsc_global_topk_f32(ptr(scores), ptr(rows), ptr(ids), n, max(stride, 1), want, ptr(out_rows), ptr(out_ids),
                                  ptr(out_scores), ptr(count), current_stream()))
    m = int(count.item())
    return out_rows[:m], out_ids[:m], out_scores[:m]


def pair_first_hits(rows, ids, q_video, r_video, n_r_videos: int, limit=None):
    """Positions, ascending, of the first hit of every distinct (q_video[rows[p]], r_video[ids[p]]) pair of a best-first hit list,
    the first `limit` of them (None: all) -- vsc_pair_first_hits.  rows / ids int64 [n], q_video / r_video int32 tables on the
    GPU; every row / id >= 0 must index its table (the kernel has no table lengths: the lists are the search's and the selection's
    own, nothing is checked here).  -> int64 device tensor; synchronises once, to read the count."""
    lib = _rd()
    rows, ids = _dev(rows, torch.int64), _dev(ids, torch.int64)
    q_video, r_video = _dev(q_video, torch.int32), _dev(r_video, torch.int32)
    n = rows.numel()
    assert rows.shape == ids.shape == (n,) and n < 1 << 31 and n_r_videos >= 1
    limit = n if limit is None or limit < 0 else min(int(limit), n)
    out = torch.empty(limit, dtype=torch.int64, device=rows.device)
    if n == 0 or limit == 0:
        return out[:0]
    count = torch.empty(1, dtype=torch.int64, device=rows.device)
    check(lib.vsc_pair_first_hits(ptr(rows), ptr(ids), n, ptr(q_video), ptr(r_video), int(n_r_videos), limit, ptr(out), ptr(count),
                                  current_stream()))
    return out[: int(count.item())]


def pair_similarity(q, r, pairs):
    """Frame x frame similarity matrices of candidate (query video, reference video) pairs.
    q [nq, d], r [nr, d]: frame banks; pairs: int64 [n, 4] rows (q_row0, q_rows, r_row0, r_rows) on the host.
    -> (flat f32 device tensor, offsets int64 numpy [n + 1]); matrix p = flat[off[p]:off[p+1]].view(q_rows, r_rows)."""
    import numpy as np
    lib = _rd()
    q, r = _dev(q, torch.float32), _dev(r, torch.float32)
    assert q.dim() == 2 and r.dim() == 2 and q.shape[1] == r.shape[1], "query / reference dimension mismatch"
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 4))
    n = pairs.shape[0]
    offsets = np.zeros(n + 1, dtype=np.int64)
    total = int((pairs[:, 1] * pairs[:, 3]).sum())
    out = torch.empty(total, dtype=torch.float32, device=q.device)
    if q.shape[0] == 0 or r.shape[0] == 0:
        if total:
            raise ValueError("pairs reference rows of an empty bank")
        return out, offsets
    check(lib.vsc_pair_similarity_f32(ptr(q), q.shape[0], ptr(r), r.shape[0], q.shape[1], pairs.ctypes.data, n,
                                      offsets.ctypes.data, ptr(out) if total else None, total, current_stream()))
    return out, offsets


def tn_align(sims, pairs, bias: float, max_step: int, top_k: int, max_path: int, min_sim: float, min_length: int,
             max_iou: float):
    """Temporal-network alignment (VCSL `tn`) of every matrix of a flat fp32 device tensor, one launch.
    sims: flat float32 device tensor; pairs: int64 [n, 3] rows (element offset, q_rows, r_rows) on the host; every element is
    used as s + bias.  -> (boxes int32 [n, max_path + 1, 4], counts int32 [n], maxsim float32 [n, max_path + 1]) on the
    device: the first counts[p] boxes of pair p in acceptance order, maxsim = max of (s + bias) over the half-open box
    minus bias.  Contract and limits: vsc_tn_align_f32 in include/vsc_hip.h."""
    import numpy as np
    lib = _rd()
    sims = _dev(sims, torch.float32).reshape(-1)
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 3))
    n = pairs.shape[0]
    boxes = torch.empty((n, max_path + 1, 4), dtype=torch.int32, device=sims.device)
    counts = torch.empty(n, dtype=torch.int32, device=sims.device)
    maxsim = torch.empty((n, max_path + 1), dtype=torch.float32, device=sims.device)
    check(lib.vsc_tn_align_f32(ptr(sims) if sims.numel() else None, sims.numel(), pairs.ctypes.data, n, float(bias),
                               int(max_step), int(top_k), int(max_path), float(min_sim), int(min_length), float(max_iou),
                               ptr(boxes), ptr(counts), ptr(maxsim), current_stream()))
    return boxes, counts, maxsim


class AlignHandle:
    """The device handle of the DP / HV alignments (vsc_align_*): bound to the stream that is current when it is made (or to
    `stream`); owns no device memory.  `scratch(cap_bytes)` sets the scratch cap of a launch (0 keeps it) and returns
    (launches, arena bytes) of the handle's last call."""

    def __init__(self, lib=None, stream=None):
        import ctypes
        self._lib = lib or _rd()
        handle = ctypes.c_void_p()
        check(self._lib.vsc_align_create(stream if stream is not None else current_stream(), ctypes.byref(handle)))
        self._h = handle

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vsc_align_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def scratch(self, cap_bytes: int = 0):
        import ctypes
        launches, used = ctypes.c_int64(), ctypes.c_int64()
        check(self._lib.vsc_align_scratch(self._h, int(cap_bytes), ctypes.byref(launches), ctypes.byref(used)))
        return launches.value, used.value


def _align_call(entry: str, sims, pairs, slots: int, args, handle):
    import numpy as np
    slots = int(slots)
    if not 1 <= slots <= 4096:          # the library refuses it by name too; here before the outputs are sized by it
        raise ValueError(f"{entry}: {slots} box slots per pair outside [1, 4096]")
    sims = _dev(sims, torch.float32).reshape(-1)
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 3))
    n = pairs.shape[0]
    boxes = torch.empty((n, slots, 4), dtype=torch.int32, device=sims.device)
    counts = torch.empty(n, dtype=torch.int32, device=sims.device)
    maxsim = torch.empty((n, slots), dtype=torch.float32, device=sims.device)
    own = handle is None
    h = AlignHandle() if own else handle
    try:
        check(getattr(h._lib, entry)(h._h, ptr(sims) if sims.numel() else None, sims.numel(), pairs.ctypes.data, n, *args, slots,
                                     ptr(boxes), ptr(counts), ptr(maxsim)))
    finally:
        if own:
            h.close()
    return boxes, counts, maxsim


def dp_align(sims, pairs, bias: float, discontinue: int, min_sim: float, ave_sim: float, min_length: int, diagonal_thres: int,
             max_boxes: int = 100, handle: AlignHandle = None):
    """DP alignment (VCSL `dp`) of every matrix of a flat fp32 device tensor; `sims`, `pairs`, `bias` as in tn_align.
    -> (boxes int32 [n, max_boxes, 4], counts int32 [n], maxsim float32 [n, max_boxes]) on the device: counts[p] is the
    number of boxes FOUND for pair p, of which the first max_boxes are stored, in the reference's order.  `handle`: an
    AlignHandle (its stream, its scratch cap); None makes one on the current stream for the call.  Contract and limits:
    vsc_align_dp_f32 in include/vsc_hip.h."""
    return _align_call("vsc_align_dp_f32", sims, pairs, max_boxes,
                       (float(bias), int(discontinue), float(min_sim), float(ave_sim), int(min_length), int(diagonal_thres)), handle)


def hv_align(sims, pairs, bias: float, min_sim: float, iou_thresh: float, max_peaks: int, handle: AlignHandle = None):
    """HV alignment (VCSL `hv`) of every matrix of a flat fp32 device tensor; `sims`, `pairs`, `bias` as in tn_align.
    -> (boxes int32 [n, max_peaks, 4], counts int32 [n] <= max_peaks, maxsim float32 [n, max_peaks]) on the device; maxsim
    is -inf for a box with an empty half-open extent (a one-cell diagonal).  Contract and limits: vsc_align_hv_f32 in
    include/vsc_hip.h."""
    return _align_call("vsc_align_hv_f32", sims, pairs, max_peaks, (float(bias), float(min_sim), float(iou_thresh)), handle)


def match_segments(maps, items, thresholds, std_ratios, max_segments: int = 8):
    """Connected components + RANSAC localisation of every probability map of a flat fp32 device tensor at every threshold,
    one launch.  maps: flat float32 device tensor; items: int64 [n, 3] rows (element offset, h, w) on the host; thresholds /
    std_ratios: sequences of equal length T.  -> (segments int32 [n, T, S, 4] = (x first, y first, x last, y last), scores
    float64 [n, T, S], counts int32 [n, T]) on the device with S >= max_segments: the launch is repeated wider when an item
    found more segments than S, so counts <= S on return (one device -> host copy of the counts per launch).  Contract and
    limits: vsc_match_segments_f32 in include/vsc_hip.h."""
    import numpy as np
    lib = _rd()
    maps = _dev(maps, torch.float32).reshape(-1)
    items = np.ascontiguousarray(np.asarray(items, dtype=np.int64).reshape(-1, 3))
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float32).reshape(-1))
    ratio = np.ascontiguousarray(np.asarray(std_ratios, dtype=np.float64).reshape(-1))
    assert thr.size == ratio.size and thr.size >= 1, "one std_ratio per threshold"
    cap = max(int(max_segments), 1)
    segments, scores, counts = match_segments_once(maps, items, thr, ratio, cap, lib)
    most = int(counts.max().item()) if counts.numel() else 0
    if most > cap:                    # the counts do not depend on the slots: the second launch holds every segment
        segments, scores, counts = match_segments_once(maps, items, thr, ratio, most, lib)
    return segments, scores, counts


def match_segments_once(maps, items, thr, ratio, max_segments: int, lib=None):
    """One vsc_match_segments_f32 launch with exactly `max_segments` slots per item; the counts are NOT capped."""
    lib = lib or _rd()
    n, t = items.shape[0], thr.size
    segments = torch.zeros((n, t, max_segments, 4), dtype=torch.int32, device=maps.device)
    scores = torch.zeros((n, t, max_segments), dtype=torch.float64, device=maps.device)
    counts = torch.zeros((n, t), dtype=torch.int32, device=maps.device)
    check(lib.vsc_match_segments_f32(ptr(maps) if maps.numel() else None, maps.numel(), items.ctypes.data, n, thr.ctypes.data,
                                     ratio.ctypes.data, t, int(max_segments), ptr(segments), ptr(scores), ptr(counts),
                                     current_stream()))
    return segments, scores, counts


def match_maps(sims, items, resolution: int, with_transpose: bool, out=None):
    """Best query view + padded 3-channel network inputs of every matrix of a flat fp32 device tensor, without a host
    synchronisation.  sims: flat float32 device tensor (ops.pair_similarity's); items: int64 [n, 4] rows (element offset, q_rows,
    r_rows, frames per view) on the host.  -> (maps [n * (1 + with_transpose), 3, R, R] float32 on the device -- a permuted view
    of the channels-last buffer the kernel writes, i.e. what the networks' NHWC conversion takes without a copy; with the
    transpose the order is map, transposed map, map, ... --, view_start int32 [n] on the device).  `out`: a contiguous
    [n * (1 + with_transpose), R, R, 3] float32 device tensor to write into (default: a new one; every element is written).
    Contract and refusals: vsc_match_maps_f32 in include/vsc_hip.h."""
    import numpy as np
    lib = _rd()
    sims = _dev(sims, torch.float32).reshape(-1)
    items = np.ascontiguousarray(np.asarray(items, dtype=np.int64).reshape(-1, 4))
    n, r, slices = items.shape[0], int(resolution), 2 if with_transpose else 1
    if out is None:
        out = torch.empty((n * slices, max(r, 0), max(r, 0), 3), dtype=torch.float32, device=sims.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (n * slices, r, r, 3), \
        "out must be a contiguous float32 [n * (1 + with_transpose), R, R, 3] device tensor"
    view_start = torch.empty(n, dtype=torch.int32, device=sims.device)
    check(lib.vsc_match_maps_f32(ptr(sims) if sims.numel() else None, sims.numel(), items.ctypes.data, n, r, int(bool(with_transpose)),
                                 ptr(view_start) if n else None, ptr(out) if out.numel() else None, current_stream()))
    return out.permute(0, 3, 1, 2), view_start


FRAME_FILTER_MAX_ROWS = 4096      # VSC_FRAME_FILTER_MAX_ROWS of include/vsc_hip.h
_frame_filter_handles = {}


def frame_filter_handle():
    """The vsc_frame_filter handle of the current library on the current stream (made on first use, kept for the process: it is
    the stream and owns no device memory)."""
    import ctypes
    lib = _rd()
    stream = current_stream()
    key = (_PRECISION, stream.value or 0)
    if key not in _frame_filter_handles:
        h = ctypes.c_void_p()
        check(lib.vsc_frame_filter_create(stream, ctypes.byref(h)))
        _frame_filter_handles[key] = h
    return _frame_filter_handles[key]


def frame_filter(sims, items, threshold: float, want_means: bool = False):
    """Greedy near-duplicate frame filter of every frame x frame matrix of a flat fp32 device tensor, one launch per 128 videos and
    no host synchronisation.  sims: flat float32 device tensor (ops.pair_similarity's); items: int64 [n, 2] rows (element offset,
    rows) on the host; threshold: compared as float32.  -> (kept int32 [sum rows], counts int32 [n]) on the device, and with
    want_means also (means float32 [sum rows], order int32 [sum rows]): video p owns the slice at the prefix sum of the rows; the
    first counts[p] entries of its kept slice are the kept rows ascending, the rest -1.  Equal frame means are visited in
    descending index.  Contract, limits and refusals: vsc_frame_filter_f32 in include/vsc_hip.h."""
    import numpy as np
    lib = _rd()
    sims = _dev(sims, torch.float32).reshape(-1)
    items = np.ascontiguousarray(np.asarray(items, dtype=np.int64).reshape(-1, 2))
    n = items.shape[0]
    total = int(items[:, 1].clip(min=0).sum())
    kept = torch.empty(total, dtype=torch.int32, device=sims.device)
    counts = torch.empty(n, dtype=torch.int32, device=sims.device)
    means = torch.empty(total, dtype=torch.float32, device=sims.device) if want_means else None
    order = torch.empty(total, dtype=torch.int32, device=sims.device) if want_means else None
    opt = lambda t: ptr(t) if t is not None and t.numel() else None     # noqa: E731
    check(lib.vsc_frame_filter_f32(frame_filter_handle(), opt(sims), sims.numel(), items.ctypes.data, n, float(threshold), opt(kept),
                                   opt(counts), opt(means), opt(order)))
    return (kept, counts, means, order) if want_means else (kept, counts)


def _frames_u8(frames):
    assert frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3, \
        "frames must be uint8 [n, H, W, 3] on the GPU"
    return frames.contiguous()


def frame_var(frames):
    """np.stack(frames).var(axis=0).sum(-1) of uint8 device frames [n, H, W, 3], bit-identical -> float64 [H, W] on the device
    (vsc_frame_var_u8)."""
    lib = _rd()
    frames = _frames_u8(frames)
    n, h, w = frames.shape[:3]
    out = torch.empty((h, w), dtype=torch.float64, device=frames.device)
    check(lib.vsc_frame_var_u8(ptr(frames), n, h, w, ptr(out), current_stream()))
    return out


def canny_count(frames, idx, low: float = 50, high: float = 400):
    """Per pixel, the number of frames[idx] where Canny(low, high) marks an edge -> uint16 [H, W] on the device.
    Contract: vsc_canny_count_u8."""
    import numpy as np
    lib = _rd()
    frames = _frames_u8(frames)
    n, h, w = frames.shape[:3]
    idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int32).reshape(-1))
    out = torch.empty((h, w), dtype=torch.uint16, device=frames.device)
    check(lib.vsc_canny_count_u8(ptr(frames), n, idx.ctypes.data, idx.size, h, w, float(low), float(high), ptr(out), current_stream()))
    return out


def view_maps(frames, idx, low: float = 50, high: float = 400):
    """Both maps the view decisions read (src/image_preprocess.py), with ONE device -> host copy: -> (variance float64 [H, W],
    edge count uint16 [H, W]) as numpy arrays."""
    import numpy as np
    lib = _rd()
    frames = _frames_u8(frames)
    n, h, w = frames.shape[:3]
    idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int32).reshape(-1))
    buf = torch.empty(h * w * 10, dtype=torch.uint8, device=frames.device)     # float64 map, then the uint16 map
    var, count = buf[:h * w * 8], buf[h * w * 8:]
    check(lib.vsc_frame_var_u8(ptr(frames), n, h, w, ptr(var), current_stream()))
    check(lib.vsc_canny_count_u8(ptr(frames), n, idx.ctypes.data, idx.size, h, w, float(low), float(high), ptr(count),
                                 current_stream()))
    host = buf.cpu().numpy()
    return host[:h * w * 8].view(np.float64).reshape(h, w), host[h * w * 8:].view(np.uint16).reshape(h, w)


def view_maps_dev(frames, idx, low: float = 50, high: float = 400):
    """view_maps without the copy: -> (variance float64 [H, W], edge count uint16 [H, W]) as views of ONE device buffer (the
    float64 map first), for ops.view_decide."""
    import numpy as np
    lib = _rd()
    frames = _frames_u8(frames)
    n, h, w = frames.shape[:3]
    idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int32).reshape(-1))
    buf = torch.empty(h * w * 10, dtype=torch.uint8, device=frames.device)     # float64 map, then the uint16 map
    var, count = buf[:h * w * 8], buf[h * w * 8:]
    check(lib.vsc_frame_var_u8(ptr(frames), n, h, w, ptr(var), current_stream()))
    check(lib.vsc_canny_count_u8(ptr(frames), n, idx.ctypes.data, idx.size, h, w, float(low), float(high), ptr(count),
                                 current_stream()))
    return var.view(torch.float64).reshape(h, w), count.view(torch.uint16).reshape(h, w)


VIEW_DECIDE_MAX_VIEWS = 64        # VSC_VIEW_DECIDE_MAX_VIEWS of include/vsc_hip.h
VIEW_DECIDE_MAX_SIDE = 4096       # VSC_VIEW_DECIDE_MAX_SIDE
_view_decide_handles = {}


def view_decide_handle():
    """The vsc_view_decide handle of the current library on the current stream (made on first use, kept for the process: it is
    the stream and owns no device memory)."""
    import ctypes
    lib = _rd()
    stream = current_stream()
    key = (_PRECISION, stream.value or 0)
    if key not in _view_decide_handles:
        h = ctypes.c_void_p()
        check(lib.vsc_view_decide_create(stream, ctypes.byref(h)))
        _view_decide_handles[key] = h
    return _view_decide_handles[key]


def view_decide(var, count, items, max_views: int = VIEW_DECIDE_MAX_VIEWS, trace: bool = False):
    """The view decisions of src/image_preprocess.py (decide_views) on maps that stay on the device, one launch per 64 videos and
    no host synchronisation.  var: float64 device tensor, count: uint16 device tensor (any shapes: read flat); items: int64 [n, 6]
    rows (element offset of the video's [h, w] variance map in var, of its count map in count, h, w, Canny samples m, frames n) on
    the host.  -> (boxes int32 [n, max_views, 4] = (y0, y1, x0, x1) in the reference's order with -1 tails, counts int32 [n],
    status int32 [n]: 1 = the video needs more views or pending regions than the kernel holds and is left to the host) on the
    device, and with trace also float64 [n, 8] (rows of videos under 5 frames are not written).  Contract, limits and refusals:
    vsc_view_decide_f64 in include/vsc_hip.h."""
    import numpy as np
    lib = _rd()
    var = _dev(var, torch.float64).reshape(-1)
    assert count.is_cuda and count.dtype == torch.uint16, "count must be a uint16 device tensor"
    count = count.contiguous().reshape(-1)
    items = np.ascontiguousarray(np.asarray(items, dtype=np.int64).reshape(-1, 6))
    n, k = items.shape[0], max(int(max_views), 0)
    boxes = torch.empty((n, k, 4), dtype=torch.int32, device=var.device)
    counts = torch.empty(n, dtype=torch.int32, device=var.device)
    status = torch.empty(n, dtype=torch.int32, device=var.device)
    tr = torch.empty((n, 8), dtype=torch.float64, device=var.device) if trace else None
    opt = lambda t: ptr(t) if t is not None and t.numel() else None     # noqa: E731
    check(lib.vsc_view_decide_f64(view_decide_handle(), opt(var), var.numel(), opt(count), count.numel(), items.ctypes.data, n,
                                  int(max_views), opt(boxes), opt(counts), opt(status), opt(tr)))
    return (boxes, counts, status, tr) if trace else (boxes, counts, status)


def resize_bicubic(frames, boxes, size: int, out=None):
    """Crop every box (y0, y1, x0, x1) out of every uint8 device frame [n, H, W, 3] and resize it to size x size, PIL-exact
    (Image.fromarray(crop).resize((size, size), Image.BICUBIC)) -> uint8 [len(boxes) * n, size, size, 3], view-major
    (vsc_resize_bicubic_u8)."""
    import numpy as np
    lib = _rd()
    frames = _frames_u8(frames)
    n, h, w = frames.shape[:3]
    boxes = np.ascontiguousarray(np.asarray(boxes, dtype=np.int32).reshape(-1, 4))
    k = boxes.shape[0]
    if out is None:
        out = torch.empty((k * n, size, size, 3), dtype=torch.uint8, device=frames.device)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (k * n, size, size, 3)
    check(lib.vsc_resize_bicubic_u8(ptr(frames) if n else None, n, h, w, boxes.ctypes.data, k, int(size), ptr(out) if out.numel() else None,
                                    current_stream()))
    return out


_frame_inputs_handles = {}


def frame_inputs_handle():
    """The vsc_frame_inputs handle of the current library on the current stream (made on first use, kept for the process: it is
    the stream and owns no device memory)."""
    import ctypes
    lib = _rd()
    stream = current_stream()
    key = (_PRECISION, stream.value or 0)
    if key not in _frame_inputs_handles:
        h = ctypes.c_void_p()
        check(lib.vsc_frame_inputs_create(stream, ctypes.byref(h)))
        _frame_inputs_handles[key] = h
    return _frame_inputs_handles[key]


def frame_inputs(frames, targets, outs=None):
    """Every model input of a video from its uint8 device frames [n, H, W, 3] in one call: per target row (y0, y1, x0, x1, out_h,
    out_w, top, left, crop_h, crop_w) -- src.dataset.square_target / clip_target build the loaders' -- the box of every frame
    resized with Pillow's BICUBIC to out_w x out_h, of which the window is kept -> a list of uint8 device tensors [n, crop_h,
    crop_w, 3], PIL-exact.  ``outs``: contiguous uint8 device tensors of those shapes to write into (e.g. slices of a group's
    buffer).  Contract and refusals: vsc_frame_inputs_u8 in include/vsc_hip.h."""
    import ctypes

    import numpy as np
    lib = _rd()
    frames = _frames_u8(frames)
    n, h, w = frames.shape[:3]
    targets = np.ascontiguousarray(np.asarray(targets, dtype=np.int32).reshape(-1, 10))
    k = targets.shape[0]
    if outs is None:
        outs = [torch.empty((n, max(int(t[8]), 0), max(int(t[9]), 0), 3), dtype=torch.uint8, device=frames.device) for t in targets]
    assert len(outs) == k
    for o, t in zip(outs, targets):
        assert o.is_cuda and o.dtype == torch.uint8 and o.is_contiguous() and tuple(o.shape) == (n, int(t[8]), int(t[9]), 3), \
            "outs[t] must be a contiguous uint8 device tensor [n, crop_h, crop_w, 3]"
    ptrs = (ctypes.c_void_p * max(k, 1))(*[ptr(o) if o.numel() else None for o in outs])
    check(lib.vsc_frame_inputs_u8(frame_inputs_handle(), ptr(frames) if n else None, n, h, w, targets.ctypes.data, k, ptrs))
    return list(outs)


_jpeg_decode_handles = {}


def jpeg_decode_handle():
    """The vsc_jpeg_decode handle of the current library on the current stream (made on first use, kept for the process: it owns
    the plane scratch and the uploaded tables of its stream's calls)."""
    import ctypes
    lib = _rd()
    stream = current_stream()
    key = (_PRECISION, torch.cuda.current_device(), stream.value or 0)
    if key not in _jpeg_decode_handles:
        h = ctypes.c_void_p()
        check(lib.vsc_jpeg_decode_create(stream, ctypes.byref(h)))
        _jpeg_decode_handles[key] = h
    return _jpeg_decode_handles[key]


def jpeg_decode_split_mode(split):
    """``split`` of jpeg_decode -> (mode, sub_bytes, rounds, item_bytes) for vsc_jpeg_decode_split: one of vsc_hip.jpeg.SPLITS, or a
    dict with "mode" (a name or 0 .. 3) and any of the three numbers; a number that is not given is vsc_hip.jpeg's default, never
    what an earlier call left in the handle"""
    from . import jpeg
    if isinstance(split, str):
        split = {"mode": split}
    mode = split.get("mode", "all")
    if isinstance(mode, str):
        if mode not in jpeg.SPLITS:
            raise ValueError(f"split must be one of {jpeg.SPLITS}, not {mode!r}")
        mode = jpeg.SPLITS.index(mode)
    return (int(mode), int(split.get("sub_bytes", jpeg.SPLIT_SUB_BYTES)), int(split.get("rounds", jpeg.SPLIT_ROUNDS)),
            int(split.get("item_bytes", jpeg.SPLIT_ITEM_BYTES)))


def jpeg_decode_stats():
    """vsc_jpeg_decode_stats of the current handle's last jpeg_decode(split=...) call (waits for its stream): (frames cut at
    restart markers, frames cut into sub-streams, frames the mode wanted cut that were decoded as one item, items launched)"""
    import numpy as np
    out = np.zeros(4, np.int64)
    check(_rd().vsc_jpeg_decode_stats(jpeg_decode_handle(), out.ctypes.data))
    return tuple(int(v) for v in out)


def jpeg_decode(data, rows, tables, out_len: int, out=None, restarts=None, split=None, scans=None):
    """Baseline JPEG frames decoded on the device in one call (vsc_jpeg_decode_u8): ``data`` uint8 device tensor holding the files'
    bytes, ``rows`` int64 [n, 10] the frame table and ``tables`` uint8 [s, 1608] its table sets, both host arrays as
    vsc_hip.jpeg.frame_rows / TableSets.array build them -> (uint8 device tensor [out_len] with frame i packed at its row's output
    offset, bit for bit Pillow's ``convert("RGB")`` array; int32 device tensor [n], 0 or the VSC_JPEG_STATUS_* of a damaged scan).
    Contract and refusals: vsc_jpeg_decode_u8 in include/vsc_hip.h.
    ``split`` (None or "none": one wave per frame, the default): frames are decoded in parallel inside (vsc_jpeg_decode_split_u8, the
    same bytes and status) -- "markers", "substreams", "all" or a dict (jpeg_decode_split_mode); ``restarts`` is then the CSR of
    restart-marker offsets (int64 ptr [n + 1], int32 off) as vsc_hip.jpeg.restart_rows builds it, None: no frame has markers.
    ``scans`` (None: every frame is one sequential scan): (int64 [m, 10] scan table, int64 ptr [n + 1]) as vsc_hip.jpeg.scan_rows
    builds them with ``rows``, and ``tables`` are then uint8 [s, 2696] (ScanTableSets): the frames -- progressive, several scans,
    Huffman table ids 0 .. 3, single-scan ones beside them -- go through vsc_jpeg_decode_scans_u8, one wave per frame; not with ``split``."""
    import numpy as np
    lib = _rd()
    assert data.is_cuda and data.dtype == torch.uint8 and data.is_contiguous() and data.dim() == 1
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, 10))
    tables = np.ascontiguousarray(np.asarray(tables, dtype=np.uint8).reshape(-1, 1608 if scans is None else 2696))
    n = rows.shape[0]
    if out is None:
        out = torch.empty(int(out_len), dtype=torch.uint8, device=data.device)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == int(out_len)
    status = torch.empty(n, dtype=torch.int32, device=data.device)
    if scans is not None:
        if split is not None and split != "none":
            raise ValueError("jpeg_decode: frames of several scans are decoded one wave per frame; pass the single-scan frames to a call of their own to split them")
        srows = np.ascontiguousarray(np.asarray(scans[0], dtype=np.int64).reshape(-1, 10))
        sptr = np.ascontiguousarray(np.asarray(scans[1], dtype=np.int64))
        assert sptr.shape == (n + 1,) and srows.shape[0] == int(sptr[-1]), "scans must be (int64 [m, 10], int64 ptr [n + 1]) with ptr[n] == m"
        check(lib.vsc_jpeg_decode_scans_u8(jpeg_decode_handle(), ptr(data) if data.numel() else None, data.numel(), rows.ctypes.data if n else None, n,
                                           srows.ctypes.data if len(srows) else None, sptr.ctypes.data, tables.ctypes.data if len(tables) else None, len(tables),
                                           ptr(out) if out.numel() else None, out.numel(), ptr(status) if n else None))
        return out, status
    if split is not None and split != "none":
        h = jpeg_decode_handle()
        check(lib.vsc_jpeg_decode_split(h, *jpeg_decode_split_mode(split)))
        rptr = roff = None
        if restarts is not None:
            rptr = np.ascontiguousarray(np.asarray(restarts[0], dtype=np.int64))
            roff = np.ascontiguousarray(np.asarray(restarts[1], dtype=np.int32))
            assert rptr.shape == (n + 1,) and roff.shape == (int(rptr[-1]),), "restarts must be (int64 ptr [n + 1], int32 off [ptr[n]])"
        check(lib.vsc_jpeg_decode_split_u8(h, ptr(data) if data.numel() else None, data.numel(), rows.ctypes.data if n else None, n,
                                           tables.ctypes.data if len(tables) else None, len(tables), rptr.ctypes.data if rptr is not None else None,
                                           roff.ctypes.data if roff is not None and len(roff) else None, ptr(out) if out.numel() else None, out.numel(),
                                           ptr(status) if n else None))
        return out, status
    check(lib.vsc_jpeg_decode_u8(jpeg_decode_handle(), ptr(data) if data.numel() else None, data.numel(), rows.ctypes.data if n else None, n,
                                 tables.ctypes.data if len(tables) else None, len(tables), ptr(out) if out.numel() else None, out.numel(),
                                 ptr(status) if n else None))
    return out, status


def video_pair_max(q, q_video, n_q_videos: int, r, r_video, n_r_videos: int, threshold: float, capacity: int = 1 << 20):
    """Largest frame score above ``threshold`` per (query video, reference video).
    q [nq, d], r [nr, d] float32; q_video [nq], r_video [nr] int32 video index of every row.
    -> (lims [n_q_videos + 1] int64, ref_video int32, score float32): pairs of query video v in
    lims[v]:lims[v+1], ascending reference video."""
    import ctypes
    lib = _rd()
    q, r = _dev(q, torch.float32), _dev(r, torch.float32)
    assert q.dim() == 2 and r.dim() == 2 and q.shape[1] == r.shape[1], "query / reference dimension mismatch"
    q_video, r_video = _dev(q_video, torch.int32), _dev(r_video, torch.int32)
    assert q_video.shape == (q.shape[0],) and r_video.shape == (r.shape[0],)
    # the sweep indexes a dense [n_q_videos, n_r_videos] table with these ids (atomic max): reject ids outside it here
    if q.shape[0] and (int(q_video.min()) < 0 or int(q_video.max()) >= n_q_videos):
        raise ValueError(f"q_video ids outside [0, {n_q_videos})")
    if r.shape[0] and (int(r_video.min()) < 0 or int(r_video.max()) >= n_r_videos):
        raise ValueError(f"r_video ids outside [0, {n_r_videos})")
    lims = torch.zeros(n_q_videos + 1, dtype=torch.int64, device=q.device)
    if q.shape[0] == 0 or r.shape[0] == 0 or n_q_videos == 0 or n_r_videos == 0:
        return (lims, torch.empty(0, dtype=torch.int32, device=q.device),
                torch.empty(0, dtype=torch.float32, device=q.device))
    total = ctypes.c_int64(0)
    while True:
        rv = torch.empty(capacity, dtype=torch.int32, device=q.device)
        sc = torch.empty(capacity, dtype=torch.float32, device=q.device)
        check(lib.vsc_video_pair_max_f32(ptr(q), q.shape[0], ptr(q_video), n_q_videos, ptr(r), r.shape[0], ptr(r_video),
                                         n_r_videos, q.shape[1], float(threshold), ptr(lims), ptr(rv), ptr(sc), capacity,
                                         ctypes.byref(total), current_stream()))
        if total.value <= capacity:
            return lims, rv[: total.value], sc[: total.value]
        capacity = int(total.value)


def window_attention_bf16(qkv, bias, scale, frames: int, res: int, window: int, shift: int, heads: int, bounded: bool = False):
    """Swin-V2 windowed cosine attention (head_dim 32) on image-ordered tokens.  bounded: fold every head's logit upper bound
    scale + max(bias) into its table and pass -scale where the head's logits span <= 69 (vsc_hip.h: the kernel then skips the
    softmax's row maximum), as vsc_swin_finalize does for its own tables."""
    lib = _rd()
    qkv = _dev(qkv, lp_dtype())
    bias, scale = _dev(bias, torch.float32), _dev(scale, torch.float32)
    if bounded:
        bmax, bmin = bias.max(dim=1).values, bias.min(dim=1).values
        ok = (2 * scale + (bmax - bmin)) <= 69.0
        bias = torch.where(ok[:, None], bias - (bmax + scale)[:, None], bias).contiguous()
        scale = torch.where(ok, -scale, scale).contiguous()
    assert qkv.shape == (frames * res * res, 3 * heads * 32)
    assert bias.shape == (heads, (2 * window - 1) ** 2) and scale.shape == (heads,)   # compact table
    out = torch.empty((frames * res * res, heads * 32), dtype=lp_dtype(), device=qkv.device)
    check(lib.vsc_window_attention_bf16(ptr(qkv), ptr(out), ptr(bias), ptr(scale), frames, res, window, shift, heads,
                                        current_stream()))
    return out


def ln_residual(t, gamma, beta, eps: float, x_in=None):
    """-> (x fp32, xb bf16) with x = (x_in or 0) + LayerNorm(t)."""
    lib = _rd()
    t, gamma, beta = (_dev(a, torch.float32) for a in (t, gamma, beta))
    x_in = None if x_in is None else _dev(x_in, torch.float32)
    rows, width = t.shape
    x = torch.empty_like(t)
    xb = torch.empty((rows, width), dtype=lp_dtype(), device=t.device)
    check(lib.vsc_ln_residual_f32(ptr(t), ptr(gamma), ptr(beta), ptr(x_in), ptr(x), ptr(xb), rows, width, eps,
                                  current_stream()))
    return x, xb


def gemm_ln_bf16(a, w, bias, gamma, beta, eps: float, x_in=None):
    """-> (x fp32, xb bf16) with x = (x_in or 0) + LayerNorm(a @ w.T + bias); w is [n, k], n in {128, 256, 512}."""
    lib = _rd()
    a, w = _dev(a, lp_dtype()), _dev(w, lp_dtype())
    gamma, beta = _dev(gamma, torch.float32), _dev(beta, torch.float32)
    bias = None if bias is None else _dev(bias, torch.float32)
    x_in = None if x_in is None else _dev(x_in, torch.float32)
    m, k = a.shape
    n = w.shape[0]
    assert w.shape[1] == k
    x = torch.empty((m, n), dtype=torch.float32, device=a.device)
    xb = torch.empty((m, n), dtype=lp_dtype(), device=a.device)
    check(lib.vsc_gemm_ln_bf16(ptr(a), ptr(w), ptr(bias), ptr(gamma), ptr(beta), ptr(x_in), ptr(x), ptr(xb), m, n, k,
                               eps, current_stream()))
    return x, xb


def swin_mlp_bf16(x, w1, b1, w2, b2, gamma, beta, eps: float):
    """Fused Swin-V2 MLP, widths 128 / 256 / 512: -> (x + LayerNorm(gelu(bf16(x) @ w1.T + b1) @ w2.T + b2), its bf16 shadow).
    w1 [4c, c], w2 [c, 4c] as the module holds them (the hidden-axis reordering the kernel wants is done here)."""
    import numpy as np
    lib = _rd()
    x = _dev(x, torch.float32).clone()
    m, c = x.shape
    xb = x.to(lp_dtype())
    w2h = np.ascontiguousarray(w2.detach().float().cpu().numpy())
    assert w2h.shape == (c, 4 * c) and tuple(w1.shape) == (4 * c, c)
    w2p = np.empty_like(w2h)
    check(lib.vsc_swin_mlp_permute_hidden_f32(w2h.ctypes.data, w2p.ctypes.data, c))
    w1d = _dev(w1.to(x.device), lp_dtype())
    w2d = torch.from_numpy(w2p).to(x.device).to(lp_dtype())
    b1, b2 = _dev(b1.to(x.device), torch.float32), _dev(b2.to(x.device), torch.float32)
    gamma, beta = _dev(gamma.to(x.device), torch.float32), _dev(beta.to(x.device), torch.float32)
    check(lib.vsc_swin_mlp_bf16(ptr(w1d), ptr(b1), ptr(w2d), ptr(b2), ptr(gamma), ptr(beta), ptr(x), ptr(xb), m, c, eps,
                                current_stream()))
    return x, xb


def swin_proj_mlp_bf16(x, att, wp, bp, gamma1, beta1, w1, b1, w2, b2, gamma2, beta2, eps: float):
    """The second half of a Swin-V2 block in one launch, widths 128 / 256 / 512:
    x1 = x + LN(att @ wp.T + bp) * gamma1 + beta1;  -> (x1 + LN(gelu(bf16(x1) @ w1.T + b1) @ w2.T + b2) * gamma2 + beta2, its bf16 shadow).
    att [m, c] (rounded to bf16 here); weights as the module holds them."""
    import numpy as np
    lib = _rd()
    x = _dev(x, torch.float32).clone()
    m, c = x.shape
    dev = x.device
    xb = torch.empty((m, c), dtype=lp_dtype(), device=dev)
    attd = _dev(att.to(dev), lp_dtype())
    w2h = np.ascontiguousarray(w2.detach().float().cpu().numpy())
    w2p = np.empty_like(w2h)
    check(lib.vsc_swin_mlp_permute_hidden_f32(w2h.ctypes.data, w2p.ctypes.data, c))
    wpd, w1d = _dev(wp.to(dev), lp_dtype()), _dev(w1.to(dev), lp_dtype())
    w2d = torch.from_numpy(w2p).to(dev).to(lp_dtype())
    f = [_dev(t.to(dev), torch.float32) for t in (bp, gamma1, beta1, b1, b2, gamma2, beta2)]
    check(lib.vsc_swin_proj_mlp_bf16(ptr(attd), ptr(wpd), ptr(f[0]), ptr(f[1]), ptr(f[2]), ptr(w1d), ptr(f[3]), ptr(w2d), ptr(f[4]), ptr(f[5]),
                                     ptr(f[6]), ptr(x), ptr(xb), m, c, eps, current_stream()))
    return x, xb


def swin_proj_mlp_qkv_bf16(x, att, wp, bp, gamma1, beta1, w1, b1, w2, b2, gamma2, beta2, wq, bq, eps: float):
    """swin_proj_mlp_bf16 with the next block's qkv Linear behind it (width 512): -> (x_out fp32, qkv_next = bf16(x_out) @ wq.T + bq as bf16)."""
    import numpy as np
    lib = _rd()
    x = _dev(x, torch.float32).clone()
    m, c = x.shape
    dev = x.device
    qkv = torch.empty((m, 3 * c), dtype=lp_dtype(), device=dev)
    attd = _dev(att.to(dev), lp_dtype())
    w2h = np.ascontiguousarray(w2.detach().float().cpu().numpy())
    w2p = np.empty_like(w2h)
    check(lib.vsc_swin_mlp_permute_hidden_f32(w2h.ctypes.data, w2p.ctypes.data, c))
    wpd, w1d, wqd = (_dev(t.to(dev), lp_dtype()) for t in (wp, w1, wq))
    w2d = torch.from_numpy(w2p).to(dev).to(lp_dtype())
    f = [_dev(t.to(dev), torch.float32) for t in (bp, gamma1, beta1, b1, b2, gamma2, beta2, bq)]
    check(lib.vsc_swin_proj_mlp_qkv_bf16(ptr(attd), ptr(wpd), ptr(f[0]), ptr(f[1]), ptr(f[2]), ptr(w1d), ptr(f[3]), ptr(w2d), ptr(f[4]), ptr(f[5]),
                                         ptr(f[6]), ptr(wqd), ptr(f[7]), ptr(x), ptr(qkv), m, c, eps, current_stream()))
    return x, qkv


def merge_gather_bf16(xb, frames: int, res: int):
    lib = _rd()
    xb = _dev(xb, lp_dtype())
    c = xb.shape[1]
    assert xb.shape[0] == frames * res * res
    out = torch.empty((frames * (res // 2) ** 2, 4 * c), dtype=lp_dtype(), device=xb.device)
    check(lib.vsc_merge_gather_bf16(ptr(xb), ptr(out), frames, res, c, current_stream()))
    return out
