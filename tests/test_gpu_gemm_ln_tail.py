"""LayerNorm as a tail of the persistent residual GEMM (csrc/gemm_bf16.hip, RESADD_LN): bit for bit what the GEMM launch followed
by the LayerNorm launch stores.  Every comparison is on the raw words; one side is the tail form (opt-in: VSC_GEMM_LN_TAIL=1), the
other runs under VSC_GEMM_LN_TAIL=0 (the two launches).  Both builds of the library."""
import pytest
import torch

from tools import synth
from vsc_hip.config import get_config

pytestmark = pytest.mark.gpu

N = 768
EPS = 1e-6
TAIL, TWO_LAUNCHES = 1, 2


@pytest.fixture(scope="module")
def dev():
    from vsc_hip import _lib
    _lib.require_device()
    return torch.device("cuda:0")


def _words(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(got, want, what):
    """bit equality, with the extent of a difference in the message (a few elements: arithmetic; whole rows or blocks: a stale read
    or a block nobody normalised)"""
    a, b = _words(got), _words(want)
    if torch.equal(a, b):
        return
    ne = a != b
    rows = ne.any(dim=1).nonzero().flatten()
    raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} words differ, in {len(rows)} rows (first {rows[:8].tolist()}, "
                         f"row blocks {sorted(set((rows // 256).tolist()))[:16]})")


def _problem(dev, precision, rows, k, seed):
    """a, w, bias, x0, gamma, beta: x of scale ~1 with one channel offset by ~100 (the residual stream's outlier channel)"""
    lp = torch.float16 if precision == "fp16" else torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(seed)
    a = torch.randn(rows, k, generator=g, device=dev).to(lp)
    w = (torch.randn(N, k, generator=g, device=dev) * 0.05).to(lp)
    bias = torch.randn(N, generator=g, device=dev)
    x0 = torch.randn(rows, N, generator=g, device=dev)
    x0[:, 301] += 100.0
    gamma = torch.randn(N, generator=g, device=dev)
    beta = torch.randn(N, generator=g, device=dev)
    return a, w, bias, x0, gamma, beta


def _run(prob, rows=None, sentinel=None):
    """-> (x, y, path) of one call on fresh copies, with the tail form switched on"""
    from vsc_hip import _lib
    with _lib.option("VSC_GEMM_LN_TAIL", "1"):
        return _call(prob, rows, sentinel)


def _call(prob, rows=None, sentinel=None):
    from vsc_hip import ops
    a, w, bias, x0, gamma, beta = prob
    x = x0.clone()
    y = None
    if sentinel is not None:
        y = torch.full((x0.shape[0], N), sentinel, dtype=a.dtype, device=a.device)
    y = ops.gemm_resadd_ln_bf16(a, w, bias, x, gamma, beta, EPS, y=y, rows=rows)
    return x, y, ops.gemm_resadd_ln_last_path()


def _two_launches(prob, rows=None, sentinel=None):
    from vsc_hip import _lib
    with _lib.option("VSC_GEMM_LN_TAIL", "0"):
        x, y, path = _call(prob, rows, sentinel)
    assert path == TWO_LAUNCHES
    return x, y


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("k", [768, 3072])
def test_smallest_eligible_shape(dev, precision, k):
    """88 row blocks x 3 = 264 tiles: more tiles than CUs, 33 per XCD (trios straddle the rounds), 8 CUs with a second tile"""
    from vsc_hip import ops
    with ops.operands(precision):
        prob = _problem(dev, precision, 88 * 256, k, 3)
        xr, yr = _two_launches(prob)
        x, y, path = _run(prob)
        assert path == TAIL, "the case fell back to two launches"
        assert torch.isfinite(yr.float()).all()
        _same(x, xr, "x")
        _same(y, yr, "y")


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_ragged_last_block_leaves_the_rows_behind_alone(dev, precision):
    from vsc_hip import ops
    with ops.operands(precision):
        rows = 88 * 256 - 100
        prob = _problem(dev, precision, 88 * 256, 768, 4)
        x0 = prob[3]
        x0[rows:] = -7.0                       # sentinel rows of x
        xr, yr = _two_launches(prob, rows=rows, sentinel=3.0)
        x, y, path = _run(prob, rows=rows, sentinel=3.0)
        assert path == TAIL
        _same(x, xr, "x")
        _same(y, yr, "y")
        assert bool((x[rows:] == -7.0).all()) and bool((y[rows:] == 3.0).all())
        assert not bool((y[:rows] == 3.0).all(dim=1).any())


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_ineligible_shape_takes_two_launches(dev, precision):
    """90 row blocks: an XCD's range of tiles would end inside a row block"""
    from vsc_hip import ops
    with ops.operands(precision):
        prob = _problem(dev, precision, 90 * 256, 768, 5)
        xr, yr = _two_launches(prob)
        x, y, path = _run(prob)
        assert path == TWO_LAUNCHES
        _same(x, xr, "x")
        _same(y, yr, "y")


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("k", [768, 3072])
def test_benchmark_shape_repeats(dev, precision, k):
    """332 frames x 197 tokens: 20 launches on the same inputs, each equal to the two-launch result (a stale line or a block
    nobody normalised differs in some run)"""
    from vsc_hip import ops
    with ops.operands(precision):
        prob = _problem(dev, precision, 65404, k, 6)
        xr, yr = _two_launches(prob)
        for _ in range(20):
            x, y, path = _run(prob)
            assert path == TAIL
            _same(x, xr, "x")
            _same(y, yr, "y")
    del prob
    torch.cuda.empty_cache()


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_two_streams_at_once(dev, precision):
    """two independent problems in flight on two streams (each stream has a workspace of its own)"""
    from vsc_hip import ops
    with ops.operands(precision):
        probs = [_problem(dev, precision, 88 * 256, 768, 7), _problem(dev, precision, 88 * 256, 3072, 8)]
        alone = [_run(p) for p in probs]
        assert all(r[2] == TAIL for r in alone)
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        got = [None, None]
        for _ in range(3):
            for i in (0, 1):
                with torch.cuda.stream(streams[i]):
                    got[i] = _run(probs[i])
        torch.cuda.synchronize()
        for i in (0, 1):
            assert got[i][2] == TAIL
            _same(got[i][0], alone[i][0], f"x of stream {i}")
            _same(got[i][1], alone[i][1], f"y of stream {i}")


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_encoder_descriptors_do_not_change(dev, precision):
    """ViT-B/16, 664 frames as two 332-frame chunks on two lanes (the benchmarked step), and 40 frames (one ragged chunk whose
    residual GEMMs have no tail form): the descriptors with the tail and with VSC_GEMM_LN_TAIL=0 are the same words"""
    from vsc_hip import _lib, ops
    from vsc_hip.encoder import HipEncoder
    cfg = get_config("vit_b16_224")
    with _lib.option("VSC_GEMM_LN_TAIL", "1"):      # (the encoder allocates the tail's buffers when the switch is on at finalize)
        enc = HipEncoder(cfg, synth.encoder_weights(7, cfg), max_batch=332, l2_normalize=True, lanes=2, precision=precision)
    base = torch.from_numpy(synth.frames(21, 8, cfg)).to(dev)
    x = (base.repeat(83, 1, 1, 1) + 0.001 * torch.arange(664, device=dev).view(-1, 1, 1, 1)).contiguous()
    with ops.operands(precision):
        with _lib.option("VSC_GEMM_LN_TAIL", "0"):
            ref = enc(x).clone()
            for _ in range(2):
                assert torch.equal(_words(enc(x)), _words(ref))
            ref40 = enc(x[:40]).clone()
            _call(_problem(dev, precision, 256, 768, 9))     # (the path query now says "two launches": the check below is the encoder's)
            assert ops.gemm_resadd_ln_last_path() == TWO_LAUNCHES
        assert torch.isfinite(ref).all()
        with _lib.option("VSC_GEMM_LN_TAIL", "1"):
            for _ in range(3):
                assert torch.equal(_words(enc(x)), _words(ref))
            assert ops.gemm_resadd_ln_last_path() == TAIL
            assert torch.equal(_words(enc(x[:40])), _words(ref40))
        assert torch.equal(_words(enc(x)), _words(ref))          # and the default: the switch unset
        assert ops.gemm_resadd_ln_last_path() == TAIL            # (untouched: the default path never asks for the tail form)
    enc.close()
