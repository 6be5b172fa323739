"""Host side of the CNN descriptor backbone (no GPU): the contract against the fixtures, BatchNorm folding, the state-dict names, the
baseline's two transforms, and the refusals of the model zoo and the entry points."""
import argparse
import os

import numpy as np
import pytest
import torch

import sscd_resnet_contract as C
from tools import synth
from vsc_hip import weights as W
from vsc_hip.cnn_config import CNN_PRESETS, IMAGENET_MEAN, IMAGENET_STD, cnn_weight_names, get_cnn_config

ROUND_OFF = 2e-6
_cache = {}


def _state(preset, wseed):
    if (preset, wseed) not in _cache:
        _cache[(preset, wseed)] = synth.resnet_weights(wseed, get_cnn_config(preset))
    return _cache[(preset, wseed)]


@pytest.mark.parametrize("preset,cases", [("cnn_tiny", 2), ("sscd_resnet50", 3)])
def test_contract_reproduces_every_fixture(golden_dir, preset, cases):
    """to fp32 round-off: descriptors (raw relative, L2 absolute) and the stored slices of every stage; the stage RMS stays in [0.1, 10]"""
    fx = np.load(os.path.join(golden_dir, f"cnn_{preset}.npz"))
    cfg = get_cnn_config(preset)
    assert int(fx["n_cases"]) == cases
    for i in range(cases):
        n, h, w, wseed, fseed = (int(v) for v in fx[f"c{i}_meta"])
        x = C.normalize_u8(synth.frames_u8(fseed, n, h, w), IMAGENET_MEAN, IMAGENET_STD)
        raw, l2, stages = C.forward(W.from_sscd_torchvision(_state(preset, wseed), cfg), cfg, x, return_stages=True)
        assert float(np.abs(l2.numpy() - fx[f"c{i}_desc_l2"]).max()) <= ROUND_OFF
        assert float(np.abs(raw.numpy() - fx[f"c{i}_desc"]).max()) <= ROUND_OFF * float(np.abs(fx[f"c{i}_desc"]).max())
        for name, v in stages.items():
            ref = fx[f"c{i}_{name}"]
            assert float(np.abs(v[:, :8, :2, :3].numpy() - ref).max()) <= 1e-5 * max(1.0, float(np.abs(ref).max())), name
            assert 0.1 <= float(v.pow(2).mean().sqrt()) <= 10.0, name


def test_second_weight_seed_gives_other_descriptors(golden_dir):
    fx = np.load(os.path.join(golden_dir, "cnn_sscd_resnet50.npz"))
    assert tuple(fx["c0_meta"][:3]) == tuple(fx["c2_meta"][:3]) and fx["c0_meta"][3] != fx["c2_meta"][3]
    assert float(np.abs(fx["c0_desc_l2"] - fx["c2_desc_l2"]).max()) > 1e-2


def test_bn_folding_equals_the_unfolded_graph():
    cfg = get_cnn_config("cnn_tiny")
    state = _state("cnn_tiny", 41)
    x = C.normalize_u8(synth.frames_u8(5, 2, 40, 56), IMAGENET_MEAN, IMAGENET_STD)
    raw_f, l2_f = C.forward(W.from_sscd_torchvision(state, cfg), cfg, x)
    raw_u, l2_u = C.forward_unfolded(state, cfg, x)
    assert float((l2_f - l2_u).abs().max()) <= ROUND_OFF
    assert float((raw_f - raw_u).abs().max()) <= ROUND_OFF * float(raw_u.abs().max())


def test_both_name_forms_load_and_bad_names_are_listed():
    cfg = get_cnn_config("cnn_tiny")
    state = _state("cnn_tiny", 41)
    folded = W.from_sscd_torchvision(state, cfg)
    assert sorted(folded) == sorted(cnn_weight_names(cfg))
    assert folded["conv1.weight"].shape == (64, 3, 7, 7) and folded["layer2.0.downsample.weight"].shape == (256, 256, 1, 1)
    # an adapted file: project.* instead of embeddings.1.*; BatchNorm's batch counters and a module. prefix are fine
    adapted = {("module." + k).replace("embeddings.1.", "project."): v for k, v in state.items()}
    adapted["module.backbone.bn1.num_batches_tracked"] = np.zeros((), np.int64)
    again = W.from_sscd_torchvision(adapted, cfg)
    assert all(np.array_equal(again[k], folded[k]) for k in folded)
    missing = {k: v for k, v in state.items() if k != "backbone.layer1.1.bn2.running_var"}
    with pytest.raises(ValueError, match=r"missing \['backbone.layer1.1.bn2.running_var'\]"):
        W.from_sscd_torchvision(missing, cfg)
    stray = dict(state)
    stray["backbone.fc.weight"] = np.zeros((4, 4), np.float32)
    with pytest.raises(ValueError, match=r"unmatched \['backbone.fc.weight'\]"):
        W.from_sscd_torchvision(stray, cfg)
    with pytest.raises(ValueError, match="backbone.layer4.2.conv1.weight"):      # a ResNet-50 config on the tiny state: names it lacks
        W.from_sscd_torchvision(state, get_cnn_config("sscd_resnet50"))


def _pillow_restatement(img, mode):
    """torchvision's Resize(size) / CenterCrop(size) on a PIL image, written out directly"""
    from PIL import Image
    size = 288 if mode == "resize_288" else 320
    w, h = img.size
    short, long = (w, h) if w <= h else (h, w)
    if short != size:
        new_short, new_long = size, int(size * long / short)
        img = img.resize((new_short, new_long) if w <= h else (new_long, new_short), Image.BILINEAR)
    if mode == "resize_320_center":
        w, h = img.size
        top, left = int(round((h - size) / 2.0)), int(round((w - size) / 2.0))
        img = img.crop((left, top, left + size, top + size))
    return np.asarray(img, dtype=np.uint8)


@pytest.mark.parametrize("h,w,modes", [(360, 640, ("resize_288", "resize_320_center")), (640, 360, ("resize_288", "resize_320_center")),
                                       (301, 299, ("resize_288", "resize_320_center")), (288, 288, ("resize_288", "resize_320_center")),
                                       (321, 481, ("resize_320_center",))])
def test_transforms_equal_a_direct_pillow_restatement(h, w, modes):
    from PIL import Image
    from src.dataset import sscd_transform_u8
    img = Image.fromarray(synth.frames_u8(h * 1000 + w, 1, h, w)[0])
    for mode in modes:
        got = sscd_transform_u8(mode)(img).numpy()
        want = _pillow_restatement(img, mode)
        assert got.shape == want.shape and np.array_equal(got, want), (mode, got.shape, want.shape)
        if mode == "resize_320_center":
            assert got.shape == (320, 320, 3)
        else:
            assert min(got.shape[:2]) == 288 and max(got.shape[:2]) == int(288 * max(h, w) / min(h, w))
    if (h, w) == (321, 481):      # the crop offset rounds half to even: (479 - 320) / 2 = 79.5 -> 80
        resized = img.resize((479, 320), Image.BILINEAR)
        assert np.array_equal(sscd_transform_u8("resize_320_center")(img).numpy(), np.asarray(resized.crop((80, 0, 400, 320))))
    with pytest.raises(ValueError, match="transforms must be one of"):
        sscd_transform_u8("resize_512")


def test_model_zoo_and_entry_point_refusals(tmp_path):
    from src.model_zoo import WEIGHT_FORMATS, load_encoder
    import extract_query_feats
    import extract_ref_feats
    assert "sscd_torchvision" in WEIGHT_FORMATS and sorted(CNN_PRESETS) == ["cnn_tiny", "sscd_resnet50"]
    for arch in CNN_PRESETS:
        with pytest.raises(ValueError, match=f"{arch} is a CNN preset: weights_format must be sscd_torchvision, not hf_vit"):
            load_encoder(arch, "hf_vit", "nowhere.pth", 8)
    with pytest.raises(ValueError, match="weights_format sscd_torchvision belongs to the CNN presets"):
        load_encoder("vit_b16_224", "sscd_torchvision", "nowhere.pth", 8)
    with pytest.raises(ValueError, match="swinv2_base_256 is a Swin-V2 preset: weights_format must be swin_ref, not sscd_torchvision"):
        load_encoder("swinv2_base_256", "sscd_torchvision", "nowhere.pth", 8)
    # resnet50 alone is no preset: still today's message
    with pytest.raises(ValueError, match="unknown arch 'resnet50'"):
        load_encoder("resnet50", "hf_vit", "nowhere.pth", 8)
    with pytest.raises(ValueError, match="unknown arch 'resnet50'"):
        load_encoder("resnet50", "sscd_torchvision", "nowhere.pth", 8)
    ap = extract_ref_feats.build_parser()
    base = ["--checkpoint_path", "nowhere.pth", "--arch", "sscd_resnet50", "--weights_format", "sscd_torchvision"]
    assert ap.parse_args(base).transforms == "resize_288" and ap.parse_args(base).sscd_l2 == "on"
    with pytest.raises(ValueError, match="--resize hip with the CNN arch sscd_resnet50"):
        extract_ref_feats.check_cnn_args(ap.parse_args(base + ["--resize", "hip"]))
    with pytest.raises(ValueError, match="--decode hip with the CNN arch sscd_resnet50"):
        extract_ref_feats.check_cnn_args(ap.parse_args(base + ["--decode", "hip"]))
    with pytest.raises(ValueError, match="--resize hip with the CNN arch"):          # main() refuses before any device work
        extract_ref_feats.main(ap.parse_args(base + ["--resize", "hip", "--decode", "hip"]))
    assert extract_ref_feats.check_cnn_args(ap.parse_args(base + ["--transforms", "resize_320_center", "--sscd_l2", "off"]))
    assert not extract_ref_feats.check_cnn_args(ap.parse_args(["--checkpoint_path", "x", "--arch", "vit_b16_224"]))
    args = argparse.Namespace(models=["vit_b16_224:hf_vit:a.pth", "sscd_resnet50:sscd_torchvision:b.pt"])
    with pytest.raises(ValueError, match="sscd_resnet50 is a CNN arch; the query ensemble is square-input only"):
        extract_query_feats.check_models(args.models)


def test_layer_table_counts_resnet50():
    """the FLOP source of tools/cnn_encoder_bench.py: torchvision's ResNet-50 at 224 x 224 is 4.09 GMACs without fc"""
    cfg = get_cnn_config("sscd_resnet50")
    macs = cfg.flops_per_frame(224, 224) / 2 - 2048 * 512
    assert abs(macs / 4.09e9 - 1.0) < 0.01
    assert len(cnn_weight_names(cfg)) == 2 * (1 + 16 * 3 + 4 + 1)


def test_extraction_loop_groups_frames_by_size_inside_a_video_too(tmp_path):
    """a video whose frames differ in size (the transforms keep the aspect ratio) goes through: RaggedZipFrames hands lists on,
    extract_cnn_feat encodes per (H, W) and returns the rows in the loader's order.  The encoder here is a stand-in that maps a frame to
    (H, W, its mean): the loop is host logic."""
    import io
    import zipfile
    from PIL import Image
    from src.dataset import RaggedZipFrames, raw_collate, sscd_transform_u8
    from src.extractor import extract_cnn_feat
    videos = {"R000011": [(96, 160), (150, 100), (96, 160)], "R000012": [(120, 120)], "R000013": []}
    for vid, shapes in videos.items():
        os.makedirs(tmp_path / vid[-2:], exist_ok=True)
        with zipfile.ZipFile(tmp_path / vid[-2:] / (vid + ".zip"), "w") as z:
            for i, (h, w) in enumerate(shapes):
                b = io.BytesIO()
                Image.fromarray(synth.frames_u8(900 + i, 1, h, w)[0]).save(b, format="PNG")
                z.writestr(f"{i:05d}.png", b.getvalue())
    calls = []

    def fake(frames):
        calls.append(tuple(frames.shape))
        return torch.stack([torch.tensor([f.shape[0], f.shape[1], float(f.float().mean())]) for f in frames])

    data = RaggedZipFrames(list(videos), str(tmp_path), sscd_transform_u8("resize_288"))
    loader = torch.utils.data.DataLoader(data, batch_size=3, num_workers=0, collate_fn=raw_collate)
    ids, feats, stamps = extract_cnn_feat(fake, loader, "cpu")
    assert ids == ["R000011"] * 3 + ["R000012"] and stamps.tolist() == [0, 1, 2, 0]
    assert feats[:, :2].tolist() == [[288, 480], [432, 288], [288, 480], [288, 288]]
    assert sorted(calls) == [(1, 288, 288, 3), (1, 432, 288, 3), (2, 288, 480, 3)]
    tf = sscd_transform_u8("resize_288")
    want = float(tf(Image.fromarray(synth.frames_u8(901, 1, 150, 100)[0])).float().mean())
    assert abs(float(feats[1, 2]) - want) < 1e-3
