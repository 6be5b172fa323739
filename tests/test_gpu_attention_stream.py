"""The streaming ViT attention kernel (csrc/attention_stream.hip, vsc_attention_stream_bf16) on a real MI355X, in both operand
builds: every check of tests/attention_stream_cases.py at every token count of its list (tests/test_attention_stream_cases_cpu.py
shows that a torch emulation passes them and that six defects do not), isolation, more work items than CUs, the refusals, the
entry's placement contract (stream first: tests/abi_cases.py holds the stream-last entries) and a full-size repeat."""
import ctypes

import pytest
import torch

import attention_stream_cases as sc

pytestmark = pytest.mark.gpu
PRECISIONS = ("bf16", "fp16")
GUARD, SENTINEL = 64, 0x5A5A


@pytest.fixture(scope="module")
def dev():
    from vsc_hip import _lib
    for precision in PRECISIONS:
        _lib.require_device(precision)
    return torch.device("cuda:0")


def _run(dev, precision):
    from vsc_hip import ops

    def run(qkv, frames, tokens, heads):
        with ops.operands(precision):
            return ops.attention_stream_bf16(qkv.to(dev), frames, tokens, heads).cpu()
    return run


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tokens", sc.STREAM_TOKENS)
def test_stream_attention_within_error_model(dev, precision, tokens):
    """|got - float64| <= 4 u A + tokens eta Vmax + ceil(tokens / 128) 2^-23 A element-wise on N(0, 1) and N(0, 2) operands, and the
    mean bound of the register-row kernel's test; the kernel's own figure is printed with every case."""
    report = []
    try:
        sc.check_stream_random(_run(dev, precision), precision, tokens, report=report)
    finally:
        print(f"stream random {precision}: (check, tokens, worst error / bound, mean |d|) {report}")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tokens", sc.STREAM_TOKENS)
def test_stream_attention_exact_cases(dev, precision, tokens):
    """bit for bit: constant V rows (a leaked pad key takes the row), the row sum of the rounded probabilities, the rising and the
    falling staircase (every block rescales / none does), a spike in the first, a middle and the last key block."""
    run = _run(dev, precision)
    sc.check_vit_constant_v(run, precision, tokens)
    sc.check_vit_biased_p(run, precision, tokens)
    sc.check_stream_staircase(run, precision, tokens)
    sc.check_stream_spike(run, precision, tokens)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tokens", [33, 577, 1025])
def test_stream_attention_frames_and_heads_are_isolated(dev, precision, tokens):
    sc.check_vit_isolation(_run(dev, precision), precision, tokens)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_stream_attention_more_work_items_than_cus(dev, precision):
    """9 frames x 32 heads x 5 query blocks at 577 tokens: 1440 workgroups"""
    run = _run(dev, precision)
    report = []
    try:
        sc.check_stream_random(run, precision, 577, frames=9, heads=32, report=report)
    finally:
        print(f"stream random {precision}, 9 x 32: {report}")
    sc.check_vit_constant_v(run, precision, 577, frames=9, heads=32)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_stream_attention_refusals_name_the_argument(dev, precision):
    from vsc_hip import _lib
    lib = _lib.require_device(precision)
    qkv = torch.zeros(64 * 192 + 8, dtype=torch.int16, device=dev)
    out = torch.full((64 * 64 + 8,), SENTINEL, dtype=torch.int16, device=dev)
    st = _lib.current_stream()
    call = lambda q, o, f, t, h: _lib.check(lib.vsc_attention_stream_bf16(st, ctypes.c_void_p(q), ctypes.c_void_p(o), f, t, h))
    with pytest.raises(_lib.VscHipError, match=r"attention_stream: 0 tokens outside 1\.\.%d" % _lib.ATTENTION_STREAM_MAX_TOKENS):
        call(qkv.data_ptr(), out.data_ptr(), 1, 0, 1)
    with pytest.raises(_lib.VscHipError, match=r"attention_stream: %d tokens outside" % (_lib.ATTENTION_STREAM_MAX_TOKENS + 1)):
        call(qkv.data_ptr(), out.data_ptr(), 1, _lib.ATTENTION_STREAM_MAX_TOKENS + 1, 1)
    with pytest.raises(_lib.VscHipError, match=r"attention_stream: 0 frames, 1 heads"):
        call(qkv.data_ptr(), out.data_ptr(), 0, 64, 1)
    with pytest.raises(_lib.VscHipError, match=r"attention_stream: 1 frames, 0 heads"):
        call(qkv.data_ptr(), out.data_ptr(), 1, 64, 0)
    with pytest.raises(_lib.VscHipError, match=r"attention_stream: qkv must be 16-byte aligned"):
        call(qkv.data_ptr() + 2, out.data_ptr(), 1, 64, 1)
    with pytest.raises(_lib.VscHipError, match=r"attention_stream: out must be 16-byte aligned"):
        call(qkv.data_ptr(), out.data_ptr() + 8, 1, 64, 1)
    with pytest.raises(_lib.VscHipError, match=r"attention_stream: null operand"):
        call(None, out.data_ptr(), 1, 64, 1)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call wrote to its output"


def _filled_on(side, host):
    """a device tensor that holds zeros until `side` has run its copy from (pinned) `host`"""
    t = torch.zeros(host.shape, dtype=host.dtype, device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        t.copy_(host, non_blocking=True)
    return t


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tokens", [65, 577])
def test_stream_attention_placement_contract(dev, precision, tokens):
    """the output lies between intact guard bands, and the launch runs on the caller's stream behind the caller's producer: the bits
    of the default stream after a synchronise, and not the bits that zeros give"""
    from vsc_hip import _lib
    lib = _lib.require_device(precision)
    frames, heads = 2, 2
    host = sc.vit_random(5 + tokens, frames, tokens, heads, 1.0, sc.LP[precision]["dtype"]).pin_memory()
    count = frames * tokens * heads * 64
    outs = {}
    for where in ("default", "zeros", "side"):
        buf = torch.full((count + 2 * GUARD,), SENTINEL, dtype=torch.int16, device=dev)
        out_ptr = ctypes.c_void_p(buf.data_ptr() + 2 * GUARD)
        if where == "side":
            side = torch.cuda.Stream()
            x = _filled_on(side, host)
            _lib.check(lib.vsc_attention_stream_bf16(ctypes.c_void_p(side.cuda_stream), _lib.ptr(x), out_ptr, frames, tokens, heads))
            side.synchronize()
        else:
            x = host.to(dev) if where == "default" else torch.zeros(host.shape, dtype=host.dtype, device=dev)
            _lib.check(lib.vsc_attention_stream_bf16(_lib.current_stream(), _lib.ptr(x), out_ptr, frames, tokens, heads))
        torch.cuda.synchronize()
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), f"guard band overwritten ({where})"
        outs[where] = buf[GUARD:-GUARD].clone()
    assert torch.equal(outs["side"], outs["default"])
    assert not torch.equal(outs["zeros"], outs["default"])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_stream_attention_full_size_repeat_is_bit_identical(dev, precision):
    """ViT-B/16-384 at its aligned batch: 113 frames x 577 tokens x 12 heads, three runs"""
    from vsc_hip import ops
    frames, tokens, heads = 113, 577, 12
    g = torch.Generator(device=dev).manual_seed(3)
    qkv = torch.randn(frames * tokens, 3 * heads * 64, generator=g, device=dev).to(sc.LP[precision]["dtype"])
    with ops.operands(precision):
        first = ops.attention_stream_bf16(qkv, frames, tokens, heads).clone()
        assert bool(torch.isfinite(first.float()).all())
        for _ in range(2):
            assert torch.equal(sc.bits(ops.attention_stream_bf16(qkv, frames, tokens, heads)), sc.bits(first))
