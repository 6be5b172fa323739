"""Where a call of the C ABI puts its results, and when: every case of tests/abi_cases.py four ways.

  plain    exact-size tensors, null stream: the result is the reference's at the case's tolerance (the baseline of the other legs)
  guarded  every operand inside a larger allocation with 4 KiB of guard on both sides, body aligned to 256 bytes and poisoned with
           all-ones bytes: no guard byte changes, no input changes, every element the header says is written is written, and the
           body is bit-identical to the plain result
  stream   on a fresh side stream behind a spinning wave: the inputs hold a DECOY until copies on that stream replace them, the
           outputs are copied away on that stream -- anything the library issued on another stream ran during the delay, saw the
           decoy or was overwritten, and the result differs; a call the header says only enqueues must return before the delay ends
  scratch  (users of the shared grow-only scratch) after a release, after every other scratch user (largest first), and directly
           after another entry point: the same bits three times

Every leg also holds its own result to the reference.  Three tests at the end show that the harness reports each kind of
failure: a null-stream operation inside the delayed region, a write into a guard, a row left unwritten.
"""
import contextlib
import ctypes
import math
import os
import time

import numpy as np
import pytest
import torch

import abi_cases as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, ALIGN = 4096, 256
PATTERN, POISON = 0xA5, 0xFF          # guard bytes; body bytes (NaN for floats, -1 for integers)
MIN_DELAY_MS, DELAY_FACTOR = 30.0, 20.0
NAMES = [c.name for c in A.CASES]
SCRATCH_NAMES = [c.name for c in A.CASES if c.scratch]
CASES = A.by_name()

_inputs, _refs, _plain, _ctx, _scratch_arenas = {}, {}, {}, {}, {}
_delay = {}


@pytest.fixture(scope="module")
def dev():
    from vsc_hip import _lib
    _lib.require_device()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    for h in _ctx.values():
        h.close()
    _ctx.clear()
    _scratch_arenas.clear()
    _lib.load().vsc_search_release_scratch()


def _lib_():
    from vsc_hip import _lib
    return _lib


def _inp(case):
    if case.name not in _inputs:
        _inputs[case.name] = case.inputs()
    return _inputs[case.name]


def _ref(case):
    if case.name not in _refs:
        _refs[case.name] = case.reference(_inp(case))
    return _refs[case.name]


def _context(case):
    if case.open is not None and case.name not in _ctx:
        _ctx[case.name] = case.open(_lib_().load())
    return _ctx.get(case.name)


@contextlib.contextmanager
def _options(case):
    with contextlib.ExitStack() as stack:
        for k, v in case.options.items():
            stack.enter_context(_lib_().option(k, v))
        yield


class Arena:
    """Device memory of one case: every device operand and output, exact-size or between guards."""

    def __init__(self, case, inp, dev, guarded):
        self.case, self.guarded = case, guarded
        self.view, self.raw = {}, {}
        spec = {k: (tuple(v.shape), v.dtype) for k, v in inp.items() if not k.startswith("h_")}
        spec.update({k: (tuple(s), d) for k, (s, d) in case.outputs.items()})
        for name, (shape, dtype) in spec.items():
            nbytes = math.prod(shape) * torch.empty(0, dtype=dtype).element_size()
            if guarded:
                raw = torch.empty(nbytes + 2 * GUARD + ALIGN, dtype=torch.uint8, device=dev)
                off = GUARD + (-(raw.data_ptr() + GUARD)) % ALIGN
                assert off % 8 == 0, "the allocator's blocks are at least 8-byte aligned"
                raw.fill_(PATTERN)
                self.raw[name] = (raw, off, nbytes)
                self.view[name] = raw[off:off + nbytes].view(dtype).reshape(shape)
                assert self.view[name].data_ptr() % ALIGN == 0
            else:
                self.view[name] = torch.empty(shape, dtype=dtype, device=dev)

    def bytes_of(self, name):
        v = self.view[name]
        return v.reshape(-1).view(torch.uint8)

    def load(self, values, names=None):
        for name in (names if names is not None else [k for k in values if not k.startswith("h_")]):
            self.view[name].copy_(values[name])

    def poison(self):
        for name in self.case.outputs:
            self.bytes_of(name).fill_(POISON)

    def pointers(self):
        p = {name: (ctypes.c_void_p(v.data_ptr()) if v.numel() else None) for name, v in self.view.items()}
        p["_arena"] = self
        return p

    def read(self, names):
        return {name: self.view[name].cpu() for name in names}

    def guard_errors(self):
        bad = []
        for name, (raw, off, nbytes) in self.raw.items():
            for side, part in (("before", raw[:off]), ("after", raw[off + nbytes:])):
                hit = (part != PATTERN).nonzero()
                if hit.numel():
                    first = int(hit[0]) - (off if side == "before" else 0)
                    bad.append(f"{name}: {hit.numel()} guard bytes {side} the tensor changed, first at byte {first:+d} from its "
                               f"{'start' if side == 'before' else 'end'}")
        return bad


def _invoke(case, arena, inp, stream):
    """one call; -> (host results, host-side milliseconds of the call)"""
    p = arena.pointers()
    p["ctx"] = _context(case)
    t0 = time.perf_counter()
    r = case.call(_lib_().load(), p, inp, stream)
    ms = (time.perf_counter() - t0) * 1e3
    rc, host = r if isinstance(r, tuple) else (r, None)
    _lib_().check(rc)
    return host or {}, ms


def _poison_errors(case, inp, out, ref):
    """elements the header says are written that still hold the poison (where the reference's own bits are all ones -- an id of -1 --
    the element cannot tell)"""
    bad = []
    for name in case.written():
        if name in case.inout:
            continue
        got = out[name]
        still = (A.raw_bytes(got) == POISON).all(dim=1).reshape(got.shape) & A.keep_mask(case, inp, name, got.shape)
        want = ref.get(name)
        if want is not None and case.tol.get(name) is None:
            want = A.tensor(want).reshape(got.shape).to(got.dtype)
            still &= ~(A.raw_bytes(want) == POISON).all(dim=1).reshape(got.shape)
        if bool(still.any()):
            bad.append(f"{name}: {int(still.sum())} elements were never written, first at {still.nonzero()[0].tolist()}")
    return bad


def _input_errors(case, arena, inp):
    bad = []
    for name, v in inp.items():
        if name.startswith("h_") or name in case.inout:
            continue
        if not A.same_bits(arena.view[name].cpu(), v):
            bad.append(f"input {name} was modified")
    return bad


def _bit_errors(case, inp, got, want, what):
    bad = []
    for name in got:
        a, b = A.tensor(got[name]), A.tensor(want[name])
        keep = A.keep_mask(case, inp, name, a.shape) if name in case.written() else torch.ones(a.shape, dtype=torch.bool)
        ne = (A.raw_bytes(a) != A.raw_bytes(b)).any(dim=1).reshape(a.shape) & keep
        if bool(ne.any()):
            bad.append(f"{name}: {int(ne.sum())} of {int(keep.sum())} elements differ from {what}, first at {ne.nonzero()[0].tolist()}")
    return bad


def _run(case, arena, inp, stream=None, reload=True):
    """load, poison, call on `stream` (None: the null stream), wait -> (outputs on the host, host ms)"""
    if reload:
        arena.load(inp)
    else:
        arena.load(inp, case.inout)
    arena.poison()
    torch.cuda.synchronize()
    with _options(case):
        host, ms = _invoke(case, arena, inp, stream)
    torch.cuda.synchronize()
    out = arena.read(case.written())
    out.update(host)
    return out, ms


def plain_result(case, dev):
    if case.name not in _plain:
        inp = _inp(case)
        arena = Arena(case, inp, dev, guarded=False)
        first, _ = _run(case, arena, inp)             # takes the one-time costs: code objects, workspaces, scratch growth
        out, ms = _run(case, arena, inp)
        problems = _input_errors(case, arena, inp) + _poison_errors(case, inp, out, _ref(case))
        if case.placement_bits:
            problems += _bit_errors(case, inp, first, out, "the same call repeated")
        assert not problems, f"{case.name} (plain): " + "; ".join(problems)
        A.check_against_reference(case, inp, out, _ref(case))
        _plain[case.name] = (out, ms)
    return _plain[case.name]


@pytest.mark.parametrize("name", NAMES)
def test_plain(dev, name):
    plain_result(CASES[name], dev)


def guarded_leg(case, dev, plain_out):
    inp = _inp(case)
    arena = Arena(case, inp, dev, guarded=True)
    out, _ = _run(case, arena, inp)
    problems = arena.guard_errors() + _input_errors(case, arena, inp) + _poison_errors(case, inp, out, _ref(case))
    if case.placement_bits:
        problems += _bit_errors(case, inp, out, plain_out, "the plain result")
    assert not problems, f"{case.name} (guarded): " + "; ".join(problems)
    A.check_against_reference(case, inp, out, _ref(case))


@pytest.mark.parametrize("name", NAMES)
def test_guarded(dev, name):
    case = CASES[name]
    guarded_leg(case, dev, plain_result(case, dev)[0])


# ---- the delay ------------------------------------------------------------------------------------------------------------------
def _spin_ms(lib, ticks, out):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    _lib_().check(lib.vsc_debug_spin_ticks(ticks, ctypes.c_void_p(out.data_ptr()), None))
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def delay_ticks(dev):
    """ticks of vsc_debug_spin_ticks for the stream leg's delay: the larger of 30 ms and 20 times the longest host-side duration
    of any plain call so far.  The tick rate is measured, once: two spins of different lengths, the launch cost cancels."""
    lib = _lib_().load()
    if "rate" not in _delay:
        out = torch.zeros(1, dtype=torch.int64, device=dev)
        _spin_ms(lib, 1000, out)
        short, long_ = 200_000, 2_000_000
        a, b = min(_spin_ms(lib, short, out) for _ in range(3)), min(_spin_ms(lib, long_, out) for _ in range(3))
        assert b > a, (a, b)
        _delay["rate"] = (long_ - short) / (b - a)          # ticks per millisecond
    longest = max([ms for _, ms in _plain.values()] or [0.0])
    want_ms = max(MIN_DELAY_MS, DELAY_FACTOR * longest)
    if want_ms != _delay.get("ms"):
        _delay["ms"] = want_ms
        if all(n in _plain for n in NAMES):       # the whole table ran: this is the figure of record
            slowest = max(NAMES, key=lambda k: _plain[k][1])
            try:
                with open(os.path.join(ROOT, "profiles", "abi_placement_delay.txt"), "w") as f:
                    f.write("tests/test_gpu_abi_placement.py: the delay in front of every stream leg\n"
                            f"vsc_debug_spin_ticks rate   {_delay['rate']:.1f} ticks per millisecond (two spins, HIP events)\n"
                            f"longest plain host call     {longest:.3f} ms ({slowest})\n"
                            f"delay                       {want_ms:.1f} ms = max({MIN_DELAY_MS:.0f} ms, {DELAY_FACTOR:.0f} x longest) "
                            f"= {int(want_ms * _delay['rate'])} ticks\n")
            except OSError:
                pass
    return int(want_ms * _delay["rate"])


def stream_leg(case, dev, plain_out, ticks):
    """-> list of problems"""
    inp, decoy = _inp(case), case.decoy()
    lib = _lib_().load()
    arena = Arena(case, inp, dev, guarded=False)
    staged = {k: v.to(dev) for k, v in inp.items() if not k.startswith("h_")}
    holding = {name: torch.empty_like(arena.view[name]) for name in case.written()}
    for h in holding.values():
        h.reshape(-1).view(torch.uint8).fill_(POISON)
    spin_out = torch.zeros(1, dtype=torch.int64, device=dev)
    arena.load(decoy)
    arena.poison()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    sp = ctypes.c_void_p(side.cuda_stream)
    started = torch.cuda.Event()
    with _options(case):
        _lib_().check(lib.vsc_debug_spin_ticks(ticks, ctypes.c_void_p(spin_out.data_ptr()), sp))
        started.record(side)
        with torch.cuda.stream(side):
            for name, v in staged.items():
                arena.view[name].copy_(v, non_blocking=True)
        host, _ = _invoke(case, arena, inp, sp)
        returned_in_time = not started.query()
        with torch.cuda.stream(side):
            for name, h in holding.items():
                h.copy_(arena.view[name], non_blocking=True)
    side.synchronize()
    torch.cuda.synchronize()
    out = {name: h.cpu() for name, h in holding.items()}
    out.update(host)
    problems = []
    if case.enqueue_only and not returned_in_time:
        problems.append("stream: the call returned only after the delay had ended (the header says it only enqueues)")
    if case.placement_bits:
        problems += ["stream: " + p for p in _bit_errors(case, inp, out, plain_out, "the plain result")]
    else:
        try:
            A.check_against_reference(case, inp, out, _ref(case))
        except AssertionError as e:
            problems.append(f"stream: {e}")
    return problems, out


@pytest.mark.parametrize("name", NAMES)
def test_stream(dev, name):
    case = CASES[name]
    plain_out, _ = plain_result(case, dev)
    problems, out = stream_leg(case, dev, plain_out, delay_ticks(dev))
    assert not problems, f"{case.name}: " + "; ".join(problems)
    A.check_against_reference(case, _inp(case), out, _ref(case))


# ---- the shared scratch -----------------------------------------------------------------------------------------------------------
def _weight(case):
    inp = _inp(case)
    total = sum(v.numel() * v.element_size() for k, v in inp.items() if not k.startswith("h_"))
    return total + sum(math.prod(s) * torch.empty(0, dtype=d).element_size() for s, d in case.outputs.values())


def _scratch_run(case, dev):
    if case.name not in _scratch_arenas:
        arena = Arena(case, _inp(case), dev, guarded=False)
        arena.load(_inp(case))
        _scratch_arenas[case.name] = arena
    out, _ = _run(case, _scratch_arenas[case.name], _inp(case), reload=False)
    return out


@pytest.mark.parametrize("name", SCRATCH_NAMES)
def test_scratch(dev, name):
    case = CASES[name]
    inp = _inp(case)
    lib = _lib_().load()
    others = sorted((c for c in A.CASES if c.scratch and c.name != name), key=_weight, reverse=True)
    try:
        torch.cuda.synchronize()
        lib.vsc_search_release_scratch()
        first = _scratch_run(case, dev)
        for o in others:
            _scratch_run(o, dev)
        second = _scratch_run(case, dev)
        _scratch_run(next(o for o in others if o.entry != case.entry), dev)
        third = _scratch_run(case, dev)
    finally:
        torch.cuda.synchronize()
        lib.vsc_search_release_scratch()
    A.check_against_reference(case, inp, first, _ref(case))
    problems = _bit_errors(case, inp, second, first, "the run on a fresh scratch") + \
        _bit_errors(case, inp, third, first, "the run on a fresh scratch (after another entry point)")
    assert not problems, f"{case.name} (scratch): " + "; ".join(problems)


def test_residual_gemm_layernorm_tail_stores_the_two_launch_bits(dev):
    """the plain results of the tail form and of the two launches on the same problem"""
    tail, two = (plain_result(CASES[f"gemm_resadd_ln/{k}/{A.RESADD_LN_M}"], dev)[0] for k in ("tail", "plain"))
    assert A.same_bits(tail["x"], two["x"]) and A.same_bits(tail["y"], two["y"])


# ---- the harness reports what it is there to report ------------------------------------------------------------------------------
def _torch_case(name, body):
    """out = x + 1 as torch operations: body(x, out, arena, stream) issues them (stream: the torch stream the call was given)"""
    def call(lib, p, inp, stream):
        arena = p["_arena"]
        s = torch.cuda.default_stream() if stream is None or not stream.value else torch.cuda.ExternalStream(stream.value)
        body(arena.view["x"], arena.view["out"], arena, s)
        return 0

    return A.Case(name=name, entry=("torch",), make=lambda seed: {"x": A._n(seed, (64, 33))}, outputs={"out": ((64, 33), torch.float32)},
                  call=call, reference=lambda inp: {"out": inp["x"] + 1}, tol={"out": None}, cite="x + 1", enqueue_only=True)


def _add_one(x, out, arena, s):
    with torch.cuda.stream(s):
        out.copy_(x)
        out.add_(1)


def test_harness_passes_a_correct_operation(dev):
    case = _torch_case("harness/good", _add_one)
    out, _ = plain_result(case, dev)
    guarded_leg(case, dev, out)
    problems, _ = stream_leg(case, dev, out, delay_ticks(dev))
    assert not problems, problems


def test_harness_reports_an_operation_on_the_null_stream(dev):
    def body(x, out, arena, s):
        with torch.cuda.stream(s):
            out.copy_(x)
        out.add_(1)                  # on the null stream: inside the delayed region it runs before the copy and is overwritten

    case = _torch_case("harness/null_stream", body)
    good, _ = plain_result(_torch_case("harness/good", _add_one), dev)
    problems, _ = stream_leg(case, dev, good, delay_ticks(dev))
    assert len(problems) == 1 and "differ from the plain result" in problems[0], problems


def test_harness_reports_a_host_synchronisation(dev):
    def body(x, out, arena, s):
        _add_one(x, out, arena, s)
        s.synchronize()

    good, _ = plain_result(_torch_case("harness/good", _add_one), dev)
    problems, _ = stream_leg(_torch_case("harness/sync", body), dev, good, delay_ticks(dev))
    assert len(problems) == 1 and "only after the delay had ended" in problems[0], problems


def test_harness_reports_a_write_into_a_guard(dev):
    def body(x, out, arena, s):
        _add_one(x, out, arena, s)
        if arena.guarded:
            raw, off, nbytes = arena.raw["out"]
            raw[off + nbytes + 3] = 0        # one element, three bytes past the end

    case = _torch_case("harness/guard", body)
    good, _ = plain_result(_torch_case("harness/good", _add_one), dev)
    with pytest.raises(AssertionError, match=r"out: 1 guard bytes after the tensor changed, first at byte \+3 from its end"):
        guarded_leg(case, dev, good)


def test_harness_reports_an_unwritten_row(dev):
    def body(x, out, arena, s):
        with torch.cuda.stream(s):
            out[:40].copy_(x[:40] + 1)
            out[41:].copy_(x[41:] + 1)

    case = _torch_case("harness/unwritten", body)
    good, _ = plain_result(_torch_case("harness/good", _add_one), dev)
    with pytest.raises(AssertionError, match=r"out: 33 elements were never written, first at \[40, 0\]"):
        guarded_leg(case, dev, good)


# ---- alignment: refused on the host, before anything is launched ------------------------------------------------------------------
# (entry, the argument the message must name, the bytes the header states for it)
MISALIGNED = [("gemm_bf16/bf16/257x132x64", "a", "a", 16), ("gemm_bf16/bf16/257x132x64", "w", "w", 16),
              ("gemm_bf16/bf16/257x132x64", "bias", "bias", 16), ("gemm_bf16/resadd/257x132x64", "aux", "aux", 16),
              ("gemm_bf16/f32/257x132x64", "out", "out", 16), ("gemm_bf16/bf16/257x132x64", "out", "out", 16),
              (f"gemm_resadd_ln/plain/{A.RESADD_LN_M + 1}", "x", "x_inout", 16), (f"gemm_resadd_ln/plain/{A.RESADD_LN_M + 1}", "y", "y_out", 8),
              ("gemm_ln/129x128x32", "x_in", "x_in", 16), ("gemm_ln/129x128x32", "xb", "xb", 8),
              ("attention_bf16/2x17x2", "qkv", "qkv", 16), ("attention_bf16/2x17x2", "out", "out", 16),
              ("window_attention/w8_r8_s0", "qkv", "qkv", 16), ("window_attention/w8_r8_s0", "out", "out", 16),
              ("layernorm/bf16/5x128", "x", "x", 16), ("layernorm/bf16/5x128", "g", "g", 16), ("layernorm/bf16/5x128", "out", "out", 8),
              ("layernorm/f32/5x128", "out", "out", 16), ("ln_residual/7x64", "t", "t", 16), ("ln_residual/7x64", "xb", "xb", 8),
              ("patchify/tiny", "frames", "frames", 16), ("patchify/tiny", "out", "patches", 16),
              ("merge_gather/3x8x64", "xb", "xb", 16), ("merge_gather/3x8x64", "out", "out", 16),
              ("swin_mlp/129x128", "w1", "w1", 16), ("swin_mlp/129x128", "x", "x", 16), ("swin_proj/129x128", "att", "att", 16),
              ("swin_qkv/129x512", "qkv", "qkv_next", 16), ("swin_qkv/129x512", "wq", "wq", 16),
              ("encoder/forward_lanes1", "frames", "frames", 16), ("encoder/forward_debug_lanes2", "tokens", "tokens_out", 16),
              ("swin/forward", "frames", "frames", 16)]


@pytest.mark.parametrize("name,operand,argument,bytes_", MISALIGNED)
def test_misaligned_pointer_is_refused_before_any_launch(dev, name, operand, argument, bytes_):
    """the pointer moved by ONE element (2 or 4 bytes): VSC_ERR_INVALID with the argument's name in the message.  The poisoned outputs
    are untouched afterwards: nothing ran."""
    case = CASES[name]
    inp = _inp(case)
    arena = Arena(case, inp, dev, guarded=True)
    arena.load(inp)
    arena.poison()
    torch.cuda.synchronize()
    p = arena.pointers()
    p["ctx"] = _context(case)
    step = arena.view[operand].element_size()
    assert step < bytes_
    p[operand] = ctypes.c_void_p(p[operand].value + step)
    with _options(case):
        r = case.call(_lib_().load(), p, inp, None)
    rc = r[0] if isinstance(r, tuple) else r
    message = _lib_().load().vsc_last_error().decode()
    torch.cuda.synchronize()
    assert rc == -1, (rc, message)           # VSC_ERR_INVALID
    assert f"{argument} must be {bytes_}-byte aligned" in message, message
    for out in case.outputs:
        assert bool((arena.bytes_of(out) == POISON).all()), f"{out} was written by a refused call"
    assert not arena.guard_errors()


def test_search_accepts_rows_at_any_dword_and_refuses_narrow_float4_rows(dev):
    """d = 5 from a pointer one float past an allocation's start is legal (rows start on any dword); d = 8 there is refused: the
    pre-filter path's re-scoring reads rows narrower than 32 floats as float4"""
    from oracle import knn_oracle
    lib = _lib_().load()
    nq, nr, k = 9, 70, 3
    scores, ids = torch.empty((nq, k), device=dev), torch.empty((nq, k), dtype=torch.int64, device=dev)
    for d, ok in ((5, True), (8, False)):
        q, r = A._bank(31, nq, d), A._bank(32, nr, d)
        qd = torch.from_numpy(q).to(dev)
        buf = torch.zeros(nr * d + 1, device=dev)
        buf[1:].copy_(torch.from_numpy(r).reshape(-1))
        rc = lib.vsc_knn_ip_f32(ctypes.c_void_p(qd.data_ptr()), nq, ctypes.c_void_p(buf.data_ptr() + 4), nr, d, k, 0,
                                ctypes.c_void_p(scores.data_ptr()), ctypes.c_void_p(ids.data_ptr()), None)
        torch.cuda.synchronize()
        if ok:
            assert rc == 0, lib.vsc_last_error().decode()
            D, I = knn_oracle.knn_ip(q, r, k)
            assert np.array_equal(ids.cpu().numpy(), I) and np.array_equal(scores.cpu().numpy().view(np.uint32), D.view(np.uint32))
        else:
            assert rc == -1 and "r_dev must be 16-byte aligned" in lib.vsc_last_error().decode()
    lib.vsc_search_release_scratch()
