"""tests/abi_cases.py held to itself, without a GPU: every export of include/vsc_hip.h that takes a stream has a case (or a stated
exclusion), every case builds its operands deterministically, its decoy is another valid problem of the same shapes with another
result, and every reference runs and has the shape the case declares."""
import math
import os
import re

import numpy as np
import pytest
import torch

import abi_cases as A
from vsc_hip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vsc_hip.h")
CASES = A.by_name()


def _stream_taking_exports():
    """names of the header's prototypes whose last parameter is `void *stream`"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(vsc_\w+)\s*\([^;{]*?void\s*\*\s*stream\s*\)\s*;", text)))


def test_every_stream_taking_export_has_a_case_or_an_exclusion():
    exports = _stream_taking_exports()
    assert len(exports) >= 45 and "vsc_gemm_bf16" in exports and "vsc_pair_first_hits" in exports, exports
    covered = {e for c in A.CASES for e in c.entry}
    for name in exports:
        assert name in _lib.SIGNATURES, f"{name} is in the header and not in vsc_hip/_lib.py SIGNATURES"
        assert _lib.SIGNATURES[name][1][-1] is _lib.c_void_p, f"{name}: the signature table does not end in the stream"
        assert name in covered or name in A.EXCLUDED, f"{name} takes a stream and has neither a case in tests/abi_cases.py nor an exclusion"
    for name, reason in A.EXCLUDED.items():
        assert name in exports and name not in covered and len(reason) > 20, name
    assert covered <= set(exports), sorted(covered - set(exports))


def test_names_are_unique_and_flags_are_consistent():
    assert len(CASES) == len(A.CASES)
    enqueue_only = {"vsc_encoder_forward", "vsc_swin_forward", "vsc_knn_merge_parts_f32", "vsc_global_topk_f32", "vsc_pair_first_hits",
                    "vsc_match_maps_f32"}       # the header's own words: "only enqueues", "asynchronous on `stream`"
    synchronising = {"vsc_range_search_ip_f32", "vsc_video_pair_max_f32", "vsc_tn_align_f32", "vsc_match_segments_f32"}     # "Synchronises `stream` once"
    for c in A.CASES:
        if set(c.entry) & enqueue_only:
            assert c.enqueue_only, c.name
        if set(c.entry) & synchronising:
            assert not c.enqueue_only, c.name
        assert set(c.tol) >= {n for n in c.written() if n not in ("xb", "qkv")}, c.name
        assert c.placement_bits or c.placement_reason, c.name
    exact = [c for c in A.CASES if c.entry == ("vsc_knn_ip_f32",) and not c.options]
    assert exact and all(c.enqueue_only for c in exact)       # the exact path only enqueues


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and A.same_bits(a, b)
    return np.array_equal(np.asarray(a), np.asarray(b))


def _differs(a, b):
    a, b = (x[0] if isinstance(x, tuple) else x for x in (a, b))
    return not A.same_bits(A.tensor(a), A.tensor(b))


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_is_deterministic_and_its_decoy_gives_another_result(name):
    case = CASES[name]
    inp = case.inputs()
    A._big.cache_clear()
    again = case.inputs()
    assert inp.keys() == again.keys() and all(_same(inp[k], again[k]) for k in inp), "make(seed) is not deterministic"
    decoy = case.decoy()
    assert decoy.keys() == inp.keys()
    for k, v in inp.items():
        if k.startswith("h_"):
            assert isinstance(v, np.ndarray) and _same(v, decoy[k]), f"host operand {k} must be the input's in the decoy too"
        else:
            assert isinstance(v, torch.Tensor) and v.is_contiguous() and v.dtype == decoy[k].dtype and v.shape == decoy[k].shape, k
    assert any(not _same(inp[k], decoy[k]) for k in inp if not k.startswith("h_")), "the decoy is the input"
    for n in case.inout:
        assert n in inp, f"in-out operand {n} is not among the operands"
    # the reference runs, has the declared shapes, and tells the input from the decoy
    ref, ref_decoy = case.reference(inp), case.reference(decoy)
    spec = {**{n: (tuple(inp[n].shape), inp[n].dtype) for n in case.inout}, **case.outputs}
    for n, want in ref.items():
        assert n in case.tol, f"no tolerance for {n}"
        value = want[0] if case.tol[n] == "bound" else want
        if n.startswith("h_"):
            continue
        assert n in spec, f"the reference names {n}, which the call does not write"
        assert A.tensor(value).numel() == math.prod(spec[n][0]), (n, tuple(A.tensor(value).shape), spec[n][0])
        written = A.keep_mask(case, inp, n, A.tensor(value).shape)
        assert bool(torch.isfinite(A.tensor(value).double()[written]).all()), f"reference {n} is not finite"
        if case.tol[n] == "bound":
            bound = A.tensor(want[1]).double()
            keep = A.keep_mask(case, inp, n, bound.shape)
            assert bool((bound[keep] > 0).all()) and bool(torch.isfinite(bound[keep]).all()), n
    assert any(_differs(ref[n], ref_decoy[n]) for n in ref if n in ref_decoy), "input and decoy have the same reference: a call that read the decoy would pass"
    if case.leave:
        for n, mask in case.leave(inp).items():
            assert n in spec and np.asarray(mask).size == math.prod(spec[n][0]), n
            assert not np.asarray(mask).all(), f"{n}: the call may leave every element alone -- nothing is checked"
