"""The state machine of the two model handles (vsc_encoder, vsc_swin) through ctypes, in both builds of the library: create,
set_weight, finalize-with-a-tensor-missing, forward-before-finalize and destroy make no HIP call, so none of this needs a GPU.
Pins the status codes and the exact error texts of the plumbing both handles share (csrc/model_host.h)."""
import ctypes
import os

import numpy as np
import pytest

VSC_ERR_INVALID, VSC_ERR_STATE = -1, -4


def _vit_config(**over):
    from vsc_hip._lib import EncoderConfigC
    from vsc_hip.config import get_config
    cfg = get_config("tiny")
    fields = dict(image_size=cfg.image_size, patch_size=cfg.patch_size, channels=cfg.channels, width=cfg.width, layers=cfg.layers,
                  heads=cfg.heads, mlp_dim=cfg.mlp_dim, out_dim=cfg.out_dim, ln_eps=cfg.ln_eps, act=0, pre_ln=0, patch_bias=1, pool=0,
                  gem_p=cfg.gem_p, max_batch=4, l2_normalize=1, head_conv_dim=0, lanes=2, fuse_ln=0)
    fields.update(over)
    return EncoderConfigC(**fields)


def _swin_config(**over):
    from vsc_hip._lib import SwinConfigC
    from vsc_hip.swin_config import get_swin_config
    cfg = get_swin_config("swinv2_base_256")
    four = lambda t: (ctypes.c_int32 * 4)(*t)
    fields = dict(image_size=cfg.image_size, patch_size=cfg.patch_size, channels=cfg.channels, embed_dim=cfg.embed_dim,
                  stages=cfg.stages, depths=four(cfg.depths), heads=four(cfg.heads), window_size=cfg.window_size,
                  pretrained_window_sizes=four(cfg.pretrained_window_sizes), mlp_ratio=cfg.mlp_ratio, out_dim=cfg.out_dim,
                  ln_eps=cfg.ln_eps, gem_p=cfg.gem_p, max_batch=8, l2_normalize=1)
    fields.update(over)
    return SwinConfigC(**fields)


# model -> (C prefix, prefix of its error texts, config, a tensor of the config and its element count, the lexicographically first
#           tensor of the config, an override that makes the config invalid)
MODELS = {
    "vit": ("vsc_encoder", "", _vit_config, "cls", 128, "blocks.0.fc1.bias", dict(width=100)),
    "swin": ("vsc_swin", "swin ", _swin_config, "norm.bias", 1024, "layers.0.blocks.0.attn.cpb_mlp.0.bias", dict(mlp_ratio=3)),
}


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def lib(request):
    from vsc_hip import _lib
    if not all(os.path.exists(p) for p in _lib.LIB_PATHS.values()):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load(request.param)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_handle_state_machine_and_error_texts(lib, model):
    prefix, say, config, tensor, count, first, _ = MODELS[model]
    fn = lambda name: getattr(lib, f"{prefix}_{name}")
    err = lambda: lib.vsc_last_error().decode()
    c = config()
    h = ctypes.c_void_p()
    assert fn("create")(ctypes.byref(c), ctypes.byref(h)) == 0 and h.value
    try:
        buf = np.zeros(count, dtype=np.float32)
        data = buf.ctypes.data_as(ctypes.c_void_p)
        assert fn("set_weight")(h, b"nope", data, count) == VSC_ERR_INVALID
        assert err() == f"{say}set_weight: unknown tensor 'nope' for this config"
        assert fn("set_weight")(h, tensor.encode(), data, 7) == VSC_ERR_INVALID
        assert err() == f"{say}set_weight: '{tensor}' has 7 elements, expected {count}"
        assert fn("set_weight")(h, tensor.encode(), data, count) == 0
        assert fn("set_weight")(None, tensor.encode(), data, count) == VSC_ERR_INVALID
        assert err() == f"{say}set_weight: null argument"
        # finalize names the first missing tensor in name order, whichever were set before it
        assert fn("finalize")(h) == VSC_ERR_STATE
        assert err() == f"{say}finalize: weight '{first}' was never set"
        # forward on a handle that was never finalized: refused before anything is read or launched
        frames = np.zeros(16, dtype=np.float32).ctypes.data_as(ctypes.c_void_p)
        desc = np.zeros(16, dtype=np.float32).ctypes.data_as(ctypes.c_void_p)
        assert fn("forward")(h, frames, 1, desc, None) == VSC_ERR_STATE
        assert err() == f"{say}forward before finalize"
        assert fn("forward_debug")(h, frames, 1, desc, None, None) == VSC_ERR_STATE
        assert fn("forward_u8")(h, frames, 1, frames, frames, desc, None) == VSC_ERR_STATE
        assert err() == f"{say}forward before finalize"
        assert fn("workspace_bytes")(h) == 0 and fn("workspace_bytes")(None) == 0
    finally:
        fn("destroy")(h)
    fn("destroy")(None)     # a no-op


@pytest.mark.parametrize("model", sorted(MODELS))
def test_create_refuses_an_invalid_config_and_leaves_out_untouched(lib, model):
    prefix, _, config, _, _, _, bad = MODELS[model]
    create = getattr(lib, f"{prefix}_create")
    c = config(**bad)
    h = ctypes.c_void_p(0x5a5a)
    assert create(ctypes.byref(c), ctypes.byref(h)) == VSC_ERR_INVALID
    assert h.value == 0x5a5a
    assert lib.vsc_last_error().decode().startswith(("encoder: width 100 with 2 heads", "swin: mlp_ratio 3"))
    assert create(None, ctypes.byref(h)) == VSC_ERR_INVALID and h.value == 0x5a5a
