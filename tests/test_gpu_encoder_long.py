"""The ViT encoder above 320 tokens (the streaming attention kernel, csrc/attention_stream.hip, behind vsc_encoder_*): the long
presets against golden vectors (transformers' ViTModel / CLIPVisionModel outputs, tests/golden/gen_vit_long_golden.py) and the fp32
oracle; the streaming kernel forced onto the short presets (VSC_ATTN_LONG=1) against their EXISTING golden vectors and mean bounds;
batching, uint8 input, 1 370 tokens, and extract_ref_feats.py with a long preset."""
import functools
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

import parity_bounds
from tools import synth
from vsc_hip.config import get_config

pytestmark = pytest.mark.gpu

DESC_L2_ATOL = 1e-3


@pytest.fixture(scope="module")
def dev():
    from vsc_hip import _lib
    _lib.require_device()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=4)
def _weights(cfg, seed):
    """synthetic weights of a configuration, made once (nobody writes to them)"""
    return synth.encoder_weights(seed, cfg)


def _encoder(cfg, seed, **kw):
    from vsc_hip.encoder import HipEncoder
    if isinstance(cfg, str):
        cfg = get_config(cfg)
    w = _weights(cfg, seed)
    return cfg, w, HipEncoder(cfg, w, **kw)


def _golden_assertions(preset, g, dev, case=None, enc_l2=None):
    """the assertions of test_gpu_encoder.py::test_encoder_matches_golden (token maxima, descriptor scale, DESC_L2_ATOL, unit norms)
    plus the cosine; the mean statistics are printed, and asserted only against an EXISTING entry of parity_bounds (`case`)"""
    cfg, _, enc = _encoder(preset, int(g["weights_seed"]), max_batch=4)
    x = torch.from_numpy(synth.frames(int(g["frames_seed"]), int(g["n_frames"]), cfg)).to(dev)
    desc, tok = enc(x, return_tokens=True)
    desc, tok = desc.cpu().numpy(), tok.cpu().numpy()
    assert np.abs(tok[:, :4] - g["tokens_head"]).max() < 0.08
    assert np.abs(tok[:, -2:] - g["tokens_tail"]).max() < 0.08
    assert np.abs(tok[:, :4] - g["tokens_head"]).mean() < 0.01
    assert np.abs(desc - g["desc"]).max() < 0.02 * np.abs(g["desc"]).max()
    d2 = (enc_l2 or _encoder(preset, int(g["weights_seed"]), max_batch=2, l2_normalize=True)[2])(x).cpu().numpy()
    mean_abs, bias = parity_bounds.stats(d2, g["desc_l2"])
    print(f"{preset}: max |d| {np.abs(d2 - g['desc_l2']).max():.3e}, mean |d| {mean_abs:.3e}, |mean d| {bias:.3e}")
    np.testing.assert_allclose(d2, g["desc_l2"], rtol=0, atol=DESC_L2_ATOL)
    assert ((d2 * g["desc_l2"]).sum(1) > 0.9999).all()
    np.testing.assert_allclose(np.linalg.norm(d2, axis=1), 1.0, atol=1e-5)
    if case:
        parity_bounds.check(case, d2, g["desc_l2"])
    return d2


@pytest.mark.parametrize("preset", ["tiny_long", "tiny_clip_long"])
def test_long_encoder_matches_golden(dev, preset, golden_dir):
    """577 tokens (HF ViTModel at image 384) and 401 tokens (CLIPVisionModel at image 320).  mean |d| and |mean d| are printed, not
    asserted: a bound for them would be a number measured on the kernel under test."""
    _golden_assertions(preset, np.load(os.path.join(golden_dir, f"vit_{preset}.npz")), dev)


@pytest.mark.parametrize("preset", ["tiny", "tiny_clip", "vit_b16_224"])
def test_streaming_kernel_meets_the_existing_bounds_of_the_short_presets(dev, preset, golden_dir):
    """VSC_ATTN_LONG=1: the encoder uses the streaming kernel at 17 / 197 tokens too, and must meet the golden vectors and the mean
    bounds that tests/parity_bounds.py holds for the register-row kernel (their 15 % is the allowance for rounding-order changes).
    With the switch off again the descriptors have the bits of a run before it was ever set."""
    from vsc_hip import _lib
    g = np.load(os.path.join(golden_dir, f"vit_{preset}.npz"))
    cfg, _, enc = _encoder(preset, int(g["weights_seed"]), max_batch=2, l2_normalize=True)
    x = torch.from_numpy(synth.frames(int(g["frames_seed"]), int(g["n_frames"]), cfg)).to(dev)
    assert _lib.get_option("VSC_ATTN_LONG") is None
    before = enc(x).clone()
    with _lib.option("VSC_ATTN_LONG", "1"):
        forced = enc(x).clone()
        d2 = _golden_assertions(preset, g, dev, case=f"vit/{preset}", enc_l2=enc)
        assert np.array_equal(d2, forced.cpu().numpy())
    # within ONE key block (the tiny presets: 17 tokens) the streaming form has the register-row kernel's arithmetic -- alpha = 0 on
    # zero accumulators, the same MFMA order -- and the same bits are the expected outcome; from two key blocks on they differ
    if cfg.tokens > _lib.ATTENTION_STREAM_KEY_BLOCK:
        assert not torch.equal(forced, before), "VSC_ATTN_LONG=1 changed nothing: the streaming kernel did not run"
    assert torch.equal(enc(x), before)


def _against_oracle(dev, cfg, n, seed=31, **kw):
    from oracle import vit_oracle
    cfg, w, enc = _encoder(cfg, seed, l2_normalize=True, **kw)
    x = torch.from_numpy(synth.frames(seed + 1, n, cfg))
    with torch.no_grad():
        ref = vit_oracle.descriptors({k: torch.from_numpy(v) for k, v in w.items()}, cfg, x).numpy()
    out = enc(x.to(dev)).cpu().numpy()
    mean_abs, bias = parity_bounds.stats(out, ref)
    print(f"{cfg.name} ({cfg.tokens} tokens): max |d| {np.abs(out - ref).max():.3e}, mean |d| {mean_abs:.3e}, |mean d| {bias:.3e}")
    assert out.shape == (n, cfg.desc_dim) and np.isfinite(out).all()
    np.testing.assert_allclose(out, ref, rtol=0, atol=DESC_L2_ATOL)
    assert ((out * ref).sum(1) > 0.9999).all()


def test_vit_b16_384_full_size_vs_oracle(dev):
    """the reference's VIT class at image 384: 577 tokens, 12 layers, GeM, 512-d"""
    _against_oracle(dev, "vit_b16_384", 2, max_batch=2)


def test_clip_vit_l14_336_four_layers_vs_oracle(dev):
    """VisionTransformer(336, 14, 1024, ., 16) cut to 4 layers: width 1024, 16 heads, patch 14 (K 588 -> 640), ln_pre, QuickGELU, CLS,
    577 tokens -- without a 24-layer oracle run on the CPU"""
    _against_oracle(dev, replace(get_config("clip_vit_l14_336"), layers=4), 2, max_batch=2)


def test_tiny_long_with_1370_tokens_creates_and_runs(dev):
    """image 592 = 37 x 37 patches + cls: 11 key blocks, 11 query blocks; workspace, pos / cls rows and the pooling at that size"""
    cfg = replace(get_config("tiny_long"), name="tiny_1370", image_size=592)
    assert cfg.tokens == 1370
    _against_oracle(dev, cfg, 2, seed=51, max_batch=1)


def test_long_encoder_batching_is_invisible(dev):
    cfg, w, enc1 = _encoder("tiny_long", 3, max_batch=1, l2_normalize=True, lanes=2)
    from vsc_hip.encoder import HipEncoder
    x = torch.from_numpy(synth.frames(5, 5, cfg)).to(dev)
    a = enc1(x)
    for mb in (2, 5):
        assert torch.equal(HipEncoder(cfg, w, max_batch=mb, l2_normalize=True)(x), a), f"max_batch {mb}"
    assert torch.equal(enc1(x[3:4]), a[3:4])


def test_long_encoder_uint8_frames_give_bit_identical_descriptors(dev):
    from vsc_hip.encoder import HipEncoder
    mean, std = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)
    cfg = get_config("tiny_long")
    enc = HipEncoder(cfg, synth.encoder_weights(3, cfg), max_batch=2, l2_normalize=True, u8_mean=mean, u8_std=std)
    u8 = torch.from_numpy((synth.uniform(17, (3, cfg.image_size, cfg.image_size, 3), 0.0, 256.0)).astype(np.uint8))
    x = u8.permute(0, 3, 1, 2).float() / 255.0
    x = (x - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1)
    assert np.array_equal(enc(u8.to(dev)).cpu().numpy(), enc(x.to(dev)).cpu().numpy())


def test_encoder_refuses_tokens_above_the_streaming_limit(dev):
    from vsc_hip import _lib, weights as W
    from vsc_hip.encoder import HipEncoder
    cfg = replace(get_config("tiny"), name="too_long", image_size=2064, patch_size=16)      # 129 x 129 + 1 = 16 642 tokens
    with pytest.raises(_lib.VscHipError, match=r"encoder: 16642 tokens > %d" % _lib.ATTENTION_STREAM_MAX_TOKENS):
        HipEncoder(cfg, {n: np.zeros(1, np.float32) for n in W.canonical_names(cfg)})     # refused at create: no weight is looked at


def test_extract_ref_feats_with_a_long_arch(dev, tmp_path):
    """a miniature zip set through extract_ref_feats.py --arch tiny_long (no new flag: the loader transform and --resize hip take the
    preset's image size): the host and the device resize write the same file, one 64-d row per frame"""
    import sys
    import extract_ref_feats as E
    from test_gpu_frame_inputs import _tiny_videos, assert_same_npz, _npz
    from test_gpu_view_preprocess import _write_zips
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import gen_vit_golden
    cfg = get_config("tiny_long")
    w = synth.encoder_weights(7, cfg)
    st = {"vit." + k: v for k, v in gen_vit_golden._to_hf_vit_state(w, cfg).items()}
    st["output_proj.weight"], st["output_proj.bias"] = torch.from_numpy(w["head.weight"]), torch.from_numpy(w["head.bias"])
    ckpt = str(tmp_path / "vit_long.pth")
    torch.save(st, ckpt)
    videos = _tiny_videos("R", 400001)
    zips, ids = str(tmp_path / "zips"), str(tmp_path / "ids.txt")
    _write_zips(zips, videos)
    with open(ids, "w") as f:
        f.write("\n".join(videos) + "\n")
    out = {}
    for mode in ("host", "hip"):
        out[mode] = str(tmp_path / f"long_{mode}")
        E.main(E.build_parser().parse_args(["--save_file", out[mode], "--zip_prefix", zips, "--input_file", ids, "--checkpoint_path", ckpt,
                                            "--arch", "tiny_long", "--weights_format", "hf_vit", "--batch_size", "2", "--workers", "0",
                                            "--resize", mode]))
    assert_same_npz(out["hip"] + ".npz", out["host"] + ".npz")
    feats = _npz(out["hip"] + ".npz")["features"]
    assert feats.shape == (sum(len(v) for v in videos.values()), 64) and np.isfinite(feats).all()
