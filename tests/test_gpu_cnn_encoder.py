"""GPU parity of the CNN descriptor backbone (csrc/conv16.hip, csrc/cnn_encoder.hip) through ctypes, in both builds of the
library: the convolution, the stem rows and the max-pool alone, the whole model against the fixtures
(tests/golden/cnn_<preset>.npz: HF ResNetModel + the reference's head classes), composition independence, the full-size repeat,
the entry point and the refusals."""
import ctypes
import os
import sys
import zipfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cnn_encoder_bounds as B
import sscd_resnet_contract as C
from tools import synth
from vsc_hip import weights as W
from vsc_hip.cnn_config import IMAGENET_MEAN, IMAGENET_STD, get_cnn_config

pytestmark = pytest.mark.gpu
PRECISIONS = ["bf16", "fp16"]
LP = {"bf16": torch.bfloat16, "fp16": torch.float16}
UNIT = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
GUARD, SENTINEL = 64, 0x5A5A


@pytest.fixture(scope="module")
def dev():
    from vsc_hip import _lib
    _lib.require_device()
    return torch.device("cuda:0")


def _lib_of(precision):
    from vsc_hip import _lib
    return _lib.require_device(precision)


def _check(rc):
    from vsc_hip import _lib
    _lib.check(rc)


def _stream():
    from vsc_hip import _lib
    return _lib.current_stream()


def _guarded(dev, count):
    """int16 buffer of `count` elements between two guard bands of sentinels -> (buffer, pointer to element 0)"""
    buf = torch.full((count + 2 * GUARD,), SENTINEL, dtype=torch.int16, device=dev)
    return buf, ctypes.c_void_p(buf.data_ptr() + 2 * GUARD)


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------- the convolution alone
CONV_CASES = [(1, 1, 1, 64, 64, 3, 1), (1, 5, 7, 64, 64, 3, 1), (2, 9, 6, 64, 128, 3, 2), (3, 5, 7, 128, 256, 1, 1),
              (2, 7, 5, 256, 512, 1, 2), (1, 4, 4, 512, 512, 3, 1), (2, 6, 6, 64, 68, 1, 1)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n,h,w,cin,cout,ks,stride", CONV_CASES)
def test_conv2d_against_float64_of_the_same_operands(dev, precision, n, h, w, cin, cout, ks, stride):
    """|d| <= u |y| + 2 K 2^-24 sum |a||w|: products of 16-bit operands are exact in fp32, K fp32 additions each round by 2^-24 of a
    partial sum that sum |a||w| bounds, the factor 2 covers the pipe's internal order; u (2^-8 bf16, 2^-11 fp16) covers the one
    rounding to the operand type at the store.  Derived, not measured."""
    lib, lp, u = _lib_of(precision), LP[precision], UNIT[precision]
    k = ks * ks * cin
    seed = 1000 + n * 7 + h * 13 + cin + cout + ks
    a = torch.from_numpy(synth.normalish(seed, (n, h, w, cin), 1.0)).to(lp)
    wt = torch.from_numpy(synth.normalish(seed + 1, (cout, ks, ks, cin), 1.0 / np.sqrt(k))).to(lp)
    bias = torch.from_numpy(synth.normalish(seed + 2, (cout,), 0.5))
    pad = (ks - 1) // 2
    ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    res = torch.from_numpy(synth.normalish(seed + 3, (n, ho, wo, cout), 1.0)).to(lp)
    a64, w64 = a.double().permute(0, 3, 1, 2), wt.double().permute(0, 3, 1, 2)
    acc = F.conv2d(a64, w64, None, stride, pad).permute(0, 2, 3, 1)
    mag = F.conv2d(a64.abs(), w64.abs(), None, stride, pad).permute(0, 2, 3, 1)
    assert acc.shape == (n, ho, wo, cout)
    a_d, w_d, b_d, r_d = a.to(dev), wt.to(dev), bias.to(dev), res.to(dev)
    for with_res, relu in ((False, 0), (False, 1), (True, 1)):
        y = acc + bias.double() + (res.double() if with_res else 0.0)
        y = y.clamp(min=0.0) if relu else y
        buf, out_ptr = _guarded(dev, n * ho * wo * cout)
        _check(lib.vsc_conv2d_nhwc_bf16(_stream(), a_d.data_ptr(), w_d.data_ptr(), b_d.data_ptr(), r_d.data_ptr() if with_res else None, out_ptr,
                                        n, h, w, cin, cout, ks, stride, relu))
        torch.cuda.synchronize()
        assert _guards_intact(buf), "guard band overwritten"
        out = buf[GUARD:-GUARD].view(lp).double().cpu().view(n, ho, wo, cout)
        bound = u * y.abs() + 2.0 * k * 2.0 ** -24 * mag
        excess = ((out - y).abs() - bound).max()
        print(f"{precision} {(n, h, w, cin, cout, ks, stride)} res {with_res} relu {relu}: max |d| {float((out - y).abs().max()):.3e}, "
              f"max (|d| - bound) {float(excess):.3e}")
        assert float(excess) <= 0.0


@pytest.mark.parametrize("precision", PRECISIONS)
def test_conv2d_refusals_name_the_argument_and_write_nothing(dev, precision):
    from vsc_hip._lib import VscHipError
    lib, lp = _lib_of(precision), LP[precision]
    a = torch.zeros((1, 4, 4, 64), dtype=lp, device=dev)
    wt = torch.zeros((64, 3, 3, 64), dtype=lp, device=dev)
    buf, out_ptr = _guarded(dev, 4 * 4 * 64)
    for args, text in (((1, 4, 4, 64, 64, 5, 1, 0), "kernel size 5"), ((1, 4, 4, 64, 64, 3, 3, 0), "stride 3"),
                       ((1, 4, 4, 48, 64, 3, 1, 0), "cin 48"), ((1, 4, 4, 64, 66, 3, 1, 0), "cout 66"), ((1, 0, 4, 64, 64, 3, 1, 0), "h 0")):
        with pytest.raises(VscHipError, match=text):
            _check(lib.vsc_conv2d_nhwc_bf16(_stream(), a.data_ptr(), wt.data_ptr(), None, None, out_ptr, *args))
    with pytest.raises(VscHipError, match="null operand"):
        _check(lib.vsc_conv2d_nhwc_bf16(_stream(), None, wt.data_ptr(), None, None, out_ptr, 1, 4, 4, 64, 64, 3, 1, 0))
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------- stem rows and max-pool
@pytest.mark.parametrize("precision", PRECISIONS)
def test_stem_rows_equal_the_contract(dev, precision):
    """(2, 37, 45) -> 19 x 23: the uint8 form normalises in the reference's fp32 order, so the rows are the contract's rounded once to
    the operand type, bit for bit; the float32-frames form gives the same rows"""
    lib, lp = _lib_of(precision), LP[precision]
    n, h, w = 2, 37, 45
    u8 = torch.from_numpy(synth.frames_u8(77, n, h, w))
    x = C.normalize_u8(u8, IMAGENET_MEAN, IMAGENET_STD)
    want = C.stem_rows(x).to(lp)
    assert want.shape == (n * 19 * 23, 192)
    mean, std = (ctypes.c_float * 3)(*IMAGENET_MEAN), (ctypes.c_float * 3)(*IMAGENET_STD)
    u8_d, x_d = u8.to(dev), x.to(dev)
    for form in ("u8", "f32"):
        buf, out_ptr = _guarded(dev, want.numel())
        if form == "u8":
            _check(lib.vsc_stem_rows_u8(_stream(), u8_d.data_ptr(), None, n, h, w, mean, std, out_ptr))
        else:
            _check(lib.vsc_stem_rows_u8(_stream(), None, x_d.data_ptr(), n, h, w, None, None, out_ptr))
        torch.cuda.synchronize()
        assert _guards_intact(buf)
        got = buf[GUARD:-GUARD].view(lp).cpu().view_as(want)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"{form}: max |d| {float((got.float() - want.float()).abs().max())}"


@pytest.mark.parametrize("precision", PRECISIONS)
def test_maxpool_never_lets_the_padding_win(dev, precision):
    """(2, 19, 23, 64) -> 10 x 12 with NEGATIVE inputs: a zero-padded maximum would be 0 along every edge"""
    lib, lp = _lib_of(precision), LP[precision]
    n, h, w, c = 2, 19, 23, 64
    x = (-0.1 - torch.from_numpy(synth.uniform(91, (n, h, w, c), 0.0, 4.0))).to(lp)
    want = F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous().to(lp)
    assert want.shape == (n, 10, 12, c) and float(want.float().max()) < 0.0
    buf, out_ptr = _guarded(dev, want.numel())
    _check(lib.vsc_maxpool3x3s2_nhwc_bf16(_stream(), x.to(dev).data_ptr(), out_ptr, n, h, w, c))
    torch.cuda.synchronize()
    assert _guards_intact(buf)
    got = buf[GUARD:-GUARD].view(lp).cpu().view_as(want)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


# ---------------------------------------------------------------------------------------------------------- the whole model
_states, _encoders, _fixtures = {}, {}, {}
FULL_PIXELS = 64 * 320 * 320


def _state(preset, wseed):
    key = (preset, wseed)
    if key not in _states:
        _states[key] = synth.resnet_weights(wseed, get_cnn_config(preset))
    return _states[key]


def _encoder(preset, wseed, precision, l2=True):
    """one encoder per (preset, weights, build, l2) for the whole module"""
    from vsc_hip.cnn_encoder import CnnHipEncoder
    key = (preset, wseed, precision, l2)
    if key not in _encoders:
        cfg = get_cnn_config(preset)
        _encoders[key] = CnnHipEncoder(cfg, W.from_sscd_torchvision(_state(preset, wseed), cfg), precision=precision, l2_normalize=l2,
                                       max_pixels=FULL_PIXELS if preset == "sscd_resnet50" else 5 * 72 * 88)
    return _encoders[key]


def _fixture(golden_dir, preset):
    if preset not in _fixtures:
        _fixtures[preset] = np.load(os.path.join(golden_dir, f"cnn_{preset}.npz"))
    return _fixtures[preset]


FIXTURE_CASES = [("cnn_tiny", 0), ("cnn_tiny", 1), ("sscd_resnet50", 0), ("sscd_resnet50", 1), ("sscd_resnet50", 2)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("preset,case", FIXTURE_CASES)
def test_descriptors_match_the_fixture(dev, golden_dir, precision, preset, case):
    """L2 descriptors against the fixture: fp16 operands within DESC_L2_ATOL = 1e-3, bf16 operands within max(1e-3, 1.5 x measured);
    both within the mean bounds of cnn_encoder_bounds.py.  The uint8 and the float32 form of the input give the same bits."""
    fx = _fixture(golden_dir, preset)
    n, h, w, wseed, fseed = (int(v) for v in fx[f"c{case}_meta"])
    u8 = torch.from_numpy(synth.frames_u8(fseed, n, h, w))
    enc = _encoder(preset, wseed, precision)
    got = enc(u8.to(dev))
    got32 = enc(C.normalize_u8(u8, IMAGENET_MEAN, IMAGENET_STD).to(dev))
    assert torch.equal(got, got32), "uint8 and float32 frames disagree"
    B.check(f"{precision}/{preset}/{case}", got.cpu().numpy(), fx[f"c{case}_desc_l2"])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_mean_bound_sees_a_one_percent_scale_error(dev, golden_dir, precision):
    """layer3.2.conv2.weight x 1.01 on sscd_resnet50: no normalisation follows a folded BatchNorm, so the error reaches the descriptor.
    fp16 operands: mean |d| 1.89e-5 against the bound 1.22e-5 -- the bound breaks, asserted.  bf16 operands: measured 8.62e-5 against the
    bound 9.36e-5 (unperturbed 8.14e-5) -- the shift, about 1.6e-5, is below bf16's own rounding noise, so the bound does NOT see it;
    the number is reported (printed here, recorded in cnn_encoder_bounds.py and DESIGN), and what is asserted is only that the
    perturbation moves the descriptors at all."""
    from vsc_hip.cnn_encoder import CnnHipEncoder
    preset, case = "sscd_resnet50", 0
    fx = _fixture(golden_dir, preset)
    n, h, w, wseed, fseed = (int(v) for v in fx[f"c{case}_meta"])
    cfg = get_cnn_config(preset)
    state = dict(_state(preset, wseed))
    state["backbone.layer3.2.conv2.weight"] = state["backbone.layer3.2.conv2.weight"] * np.float32(1.01)
    enc = CnnHipEncoder(cfg, W.from_sscd_torchvision(state, cfg), precision=precision, max_pixels=n * h * w)
    u8 = torch.from_numpy(synth.frames_u8(fseed, n, h, w)).to(dev)
    got = enc(u8).cpu().numpy()
    enc.close()
    _, mean_abs, _ = B.stats(got, fx[f"c{case}_desc_l2"])
    bound = B.mean_bounds(f"{precision}/{preset}/{case}")[0]
    print(f"{precision}: perturbed mean |d| {mean_abs:.3e} against the bound {bound:.3e}")
    if precision == "fp16":
        assert mean_abs > bound
    else:
        assert not np.array_equal(got, _encoder(preset, wseed, precision)(u8).cpu().numpy())


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_frame_alone_equals_the_frame_inside_a_call_of_five(dev, precision):
    """bit for bit; and l2 = 0 is l2 = 1 up to the normalisation"""
    preset, wseed = "cnn_tiny", 41
    u8 = torch.from_numpy(synth.frames_u8(303, 5, 72, 88)).to(dev)
    enc = _encoder(preset, wseed, precision)
    five, one = enc(u8), enc(u8[:1])
    assert torch.equal(five[:1], one)
    assert not torch.equal(five[0], five[1])
    raw = _encoder(preset, wseed, precision, l2=False)(u8)
    assert float((raw.norm(dim=1) - 1.0).abs().min()) > 1e-3, "the raw projection is not normalised"
    assert float((F.normalize(raw) - five).abs().max()) <= 2e-6


def _filled_on(side, host):
    """a device tensor that holds zeros until `side` has run its copy from (pinned) `host`: whatever is enqueued on another stream,
    with no synchronisation in between, reads the zeros"""
    t = torch.zeros(host.shape, dtype=host.dtype, device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        t.copy_(host, non_blocking=True)
    return t


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("form", ["u8", "f32"])
def test_forward_runs_on_the_callers_stream(dev, precision, form):
    """both forwards on a stream of the caller's, behind a producer on that stream and with no synchronisation in between"""
    enc = _encoder("cnn_tiny", 41, precision)
    u8 = torch.from_numpy(synth.frames_u8(606, 3, 64, 64))
    host = (u8 if form == "u8" else C.normalize_u8(u8, IMAGENET_MEAN, IMAGENET_STD)).pin_memory()
    want = enc(host.to(dev))
    side = torch.cuda.Stream()
    frames = _filled_on(side, host)
    with torch.cuda.stream(side):
        got = enc(frames)
    side.synchronize()
    assert torch.equal(got, want) and not torch.equal(want, enc(torch.zeros_like(frames)))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_building_blocks_run_on_the_callers_stream(dev, precision):
    """vsc_conv2d_nhwc_bf16, vsc_maxpool3x3s2_nhwc_bf16 and vsc_stem_rows_u8 on a side stream behind the caller's own producer: the
    same bits as on the default stream after a synchronise, and not the bits that zeros give"""
    lib, lp = _lib_of(precision), LP[precision]
    mean, std = (ctypes.c_float * 3)(*IMAGENET_MEAN), (ctypes.c_float * 3)(*IMAGENET_STD)
    n, h, w, c = 2, 9, 6, 64
    wt = torch.from_numpy(synth.normalish(712, (128, 3, 3, c), 1.0 / 24.0)).to(lp).to(dev)
    bias = torch.from_numpy(synth.normalish(713, (128,), 0.5)).to(dev)
    calls = {
        "conv2d": (torch.from_numpy(synth.normalish(711, (n, h, w, c), 1.0)).to(lp), n * 5 * 3 * 128,
                   lambda st, x, out: lib.vsc_conv2d_nhwc_bf16(st, x.data_ptr(), wt.data_ptr(), bias.data_ptr(), None, out, n, h, w, c, 128, 3, 2, 1)),
        "maxpool": (torch.from_numpy(synth.normalish(714, (n, h, w, c), 1.0)).to(lp), n * 5 * 3 * c,
                    lambda st, x, out: lib.vsc_maxpool3x3s2_nhwc_bf16(st, x.data_ptr(), out, n, h, w, c)),
        "stem_rows": (torch.from_numpy(synth.frames_u8(715, n, h, w)), n * 5 * 3 * 192,
                      lambda st, x, out: lib.vsc_stem_rows_u8(st, x.data_ptr(), None, n, h, w, mean, std, out)),
    }
    for name, (host, count, call) in calls.items():
        host = host.pin_memory()
        outs = {}
        for where in ("default", "zeros", "side"):
            buf, out_ptr = _guarded(dev, count)
            if where == "side":
                side = torch.cuda.Stream()
                x = _filled_on(side, host)
                _check(call(ctypes.c_void_p(side.cuda_stream), x, out_ptr))
                side.synchronize()
            else:
                x = host.to(dev) if where == "default" else torch.zeros(host.shape, dtype=host.dtype, device=dev)
                _check(call(_stream(), x, out_ptr))
            torch.cuda.synchronize()
            assert _guards_intact(buf), name
            outs[where] = buf[GUARD:-GUARD].clone()
        assert torch.equal(outs["side"], outs["default"]), name
        assert not torch.equal(outs["zeros"], outs["default"]), name


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_call_split_into_chunks_equals_the_call_in_one(dev, precision):
    """CnnHipEncoder splits a call into steps of max_pixels // (H W) whole frames: 5 frames of 72 x 88 with room for 2 per step
    (steps of 2, 2, 1) give the bits of the one-step call, in both input forms"""
    from vsc_hip.cnn_encoder import CnnHipEncoder
    cfg = get_cnn_config("cnn_tiny")
    u8 = torch.from_numpy(synth.frames_u8(303, 5, 72, 88)).to(dev)
    want = _encoder("cnn_tiny", 41, precision)(u8)
    small = CnnHipEncoder(cfg, W.from_sscd_torchvision(_state("cnn_tiny", 41), cfg), precision=precision, max_pixels=2 * 72 * 88 + 100)
    assert torch.equal(small(u8), want)
    assert torch.equal(small(C.normalize_u8(u8.cpu(), IMAGENET_MEAN, IMAGENET_STD).to(dev)), want)
    with pytest.raises(ValueError, match="above max_pixels"):
        small(torch.zeros((1, 200, 200, 3), dtype=torch.uint8, device=dev))
    small.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_full_size_repeat_is_bit_identical(dev, precision):
    """64 frames of 320 x 320 on sscd_resnet50, three runs"""
    u8 = torch.from_numpy(synth.frames_u8(404, 64, 320, 320)).to(dev)
    enc = _encoder("sscd_resnet50", 53, precision)
    first = enc(u8)
    assert bool(torch.isfinite(first).all()) and float((first.norm(dim=1) - 1.0).abs().max()) < 1e-5
    for _ in range(2):
        assert torch.equal(enc(u8), first)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_refusals_write_nothing(dev, precision):
    from vsc_hip._lib import CnnEncoderConfigC, VscHipError
    from vsc_hip.cnn_config import cnn_weight_names
    lib = _lib_of(precision)
    enc = _encoder("cnn_tiny", 41, precision)
    u8 = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=dev)
    x = torch.zeros((2, 3, 8, 8), dtype=torch.float32, device=dev)
    desc = torch.full((2, 128), 7.0, device=dev)
    mean, std = (ctypes.c_float * 3)(*IMAGENET_MEAN), (ctypes.c_float * 3)(*IMAGENET_STD)
    with pytest.raises(VscHipError, match="null encoder"):
        _check(lib.vsc_cnn_encoder_forward(_stream(), None, x.data_ptr(), 2, 8, 8, desc.data_ptr()))
    with pytest.raises(VscHipError, match="above the workspace's max_pixels"):
        _check(lib.vsc_cnn_encoder_forward_u8(_stream(), enc._h, u8.data_ptr(), 2, 4000, 8, mean, std, desc.data_ptr()))
    for h, w in ((0, 8), (8, 0), (-1, 8)):
        with pytest.raises(VscHipError, match="must be >= 1"):
            _check(lib.vsc_cnn_encoder_forward(_stream(), enc._h, x.data_ptr(), 2, h, w, desc.data_ptr()))
    # forward before finalize: a handle that has its config and no weights
    cfg = get_cnn_config("cnn_tiny")
    i4 = lambda t: (ctypes.c_int32 * 4)(*t)
    c = CnnEncoderConfigC(stem_width=cfg.stem_width, widths=i4(cfg.widths), depths=i4(cfg.depths), head_in=cfg.widths[3], head_out=cfg.out_dim,
                          gem_p=cfg.gem_p, l2=1, max_pixels=1 << 16)
    handle = ctypes.c_void_p()
    _check(lib.vsc_cnn_encoder_create(ctypes.byref(c), ctypes.byref(handle)))
    try:
        with pytest.raises(VscHipError, match="forward before finalize"):
            _check(lib.vsc_cnn_encoder_forward(_stream(), handle, x.data_ptr(), 2, 8, 8, desc.data_ptr()))
        with pytest.raises(VscHipError, match="was never set"):
            _check(lib.vsc_cnn_encoder_finalize(handle))
        with pytest.raises(VscHipError, match="unknown tensor"):
            one = np.zeros(4, np.float32)
            _check(lib.vsc_cnn_encoder_set_weight(handle, b"fc.weight", one.ctypes.data, 4))
        assert "conv1.weight" in cnn_weight_names(cfg)
    finally:
        lib.vsc_cnn_encoder_destroy(handle)
    torch.cuda.synchronize()
    assert bool((desc == 7.0).all())
    # any H, W >= 1 is taken
    assert enc(torch.zeros((1, 1, 1, 3), dtype=torch.uint8, device=dev)).shape == (1, 128)


# ---------------------------------------------------------------------------------------------------------- the entry point
def _write_zip(root, vid, frames):
    from PIL import Image
    os.makedirs(os.path.join(root, vid[-2:]), exist_ok=True)
    with zipfile.ZipFile(os.path.join(root, vid[-2:], vid + ".zip"), "w") as z:
        for i, f in enumerate(frames):
            import io
            b = io.BytesIO()
            Image.fromarray(f).save(b, format="JPEG", quality=90)
            z.writestr(f"{i:05d}.jpg", b.getvalue())


def test_extract_ref_feats_with_a_cnn_arch(dev, tmp_path):
    """two videos, one landscape (96 x 160) and one portrait (150 x 100), through extract_ref_feats.py --arch cnn_tiny: the file equals
    CnnHipEncoder called directly on the transformed frames, and the contract within the fp16 tolerance"""
    import io
    from PIL import Image
    import extract_ref_feats
    from src.dataset import sscd_transform_u8
    from vsc.storage import load_features
    preset, wseed = "cnn_tiny", 41
    cfg = get_cnn_config(preset)
    videos = {"R000001": synth.frames_u8(501, 3, 96, 160), "R000002": synth.frames_u8(502, 2, 150, 100)}
    for vid, frames in videos.items():
        _write_zip(str(tmp_path / "zips"), vid, frames)
    (tmp_path / "vids.txt").write_text("\n".join(videos) + "\n")
    ckpt = tmp_path / "sscd.pt"
    torch.save({k: torch.from_numpy(v) for k, v in _state(preset, wseed).items()}, ckpt)
    args = extract_ref_feats.build_parser().parse_args([
        "--checkpoint_path", str(ckpt), "--arch", preset, "--weights_format", "sscd_torchvision", "--transforms", "resize_288",
        "--zip_prefix", str(tmp_path / "zips"), "--input_file", str(tmp_path / "vids.txt"), "--save_file", str(tmp_path / "refs"),
        "--workers", "0", "--precision", "fp16"])
    extract_ref_feats.main(args)
    feats = {f.video_id: f for f in load_features(str(tmp_path / "refs.npz"))}
    assert sorted(feats) == sorted(videos)
    from vsc_hip.cnn_encoder import CnnHipEncoder
    folded = W.from_sscd_torchvision(_state(preset, wseed), cfg)
    enc = CnnHipEncoder(cfg, folded, precision="fp16", max_pixels=288 * 512)
    tf = sscd_transform_u8("resize_288")
    for vid in videos:
        with zipfile.ZipFile(str(tmp_path / "zips" / vid[-2:] / (vid + ".zip"))) as z:
            frames = torch.stack([tf(Image.open(io.BytesIO(z.read(name)))) for name in sorted(z.namelist())])
        assert min(frames.shape[1:3]) == 288 and frames.shape[1:3] != (288, 288)
        direct = torch.cat([enc(frames[i:i + 1].to(dev)) for i in range(len(frames))]).cpu().numpy()
        assert np.array_equal(feats[vid].feature, direct)
        want = C.forward(folded, cfg, C.normalize_u8(frames, IMAGENET_MEAN, IMAGENET_STD))[1].numpy()
        assert float(np.abs(direct - want).max()) <= B.DESC_L2_ATOL
