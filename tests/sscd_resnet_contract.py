"""The CNN descriptor model as torch-functional fp32 on the CPU: what ``CnnHipEncoder`` has to compute.

``forward`` takes the FOLDED tensors (vsc_hip/weights.py: from_sscd_torchvision) -- F.conv2d with the folded BatchNorm as its
bias, max_pool2d, bottleneck blocks of torchvision's ResNet v1.5 (stride on the 3 x 3), GeM(p) as the reference's
GlobalGeMPool2d (clamp(min=1e-6).pow(p).mean.pow(1/p)), Linear, F.normalize.  ``forward_unfolded`` runs the same graph from a
torchvision-named state dict with F.batch_norm in eval mode: the two agree to fp32 round-off (tests/test_sscd_resnet_cpu.py), and
tests/golden/gen_sscd_resnet_golden.py shows that both equal HF's ResNetModel under the reference's own head classes."""
import numpy as np
import torch
import torch.nn.functional as F


def _t(v):
    return v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))


def normalize_u8(frames_u8, mean, std) -> torch.Tensor:
    """uint8 [n, H, W, 3] -> float32 [n, 3, H, W] in the reference's order: ToTensor (/ 255), then Normalize (- mean, / std)"""
    x = _t(np.asarray(frames_u8)).to(torch.float32) if not isinstance(frames_u8, torch.Tensor) else frames_u8.to(torch.float32)
    x = x.permute(0, 3, 1, 2) / 255.0
    m = torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).view(1, 3, 1, 1)
    return ((x - m) / s).contiguous()


def stem_rows(x: torch.Tensor, kpad: int = 192) -> torch.Tensor:
    """im2col rows of the 7 x 7 stride-2 pad-3 stem from normalised frames [n, 3, H, W]: [n * Ho * Wo, kpad], k = (r * 7 + s) * 3 + c"""
    n = x.shape[0]
    cols = F.unfold(x, kernel_size=7, padding=3, stride=2)                   # [n, 3 * 49, L], channel-major (c, r, s)
    cols = cols.view(n, 3, 49, -1).permute(0, 3, 2, 1).reshape(-1, 147)      # -> (r, s, c)
    return F.pad(cols, (0, kpad - 147))


def _tail(x, head_w, head_b, gem_p):
    n, c = x.shape[:2]
    pooled = x.reshape(n, c, -1).clamp(min=1e-6).pow(gem_p).mean(dim=2).pow(1.0 / gem_p)
    raw = F.linear(pooled, head_w, head_b)
    return raw, F.normalize(raw)


def forward(folded: dict, cfg, frames: torch.Tensor, return_stages: bool = False):
    """frames: float32 [n, 3, H, W], normalised -> (raw [n, out], l2 [n, out]) (and {name: NCHW map} of the stem, the pool and
    every stage)"""
    w = {k: _t(v) for k, v in folded.items()}
    conv = lambda x, name, stride=1, pad=0: F.conv2d(x, w[name + ".weight"], w[name + ".bias"], stride=stride, padding=pad)
    stages = {}
    with torch.no_grad():
        x = F.relu(conv(frames, "conv1", 2, 3))
        stages["stem"] = x
        x = F.max_pool2d(x, 3, 2, 1)
        stages["pool"] = x
        for s in range(4):
            for b in range(cfg.depths[s]):
                p = f"layer{s + 1}.{b}."
                stride = cfg.block_io(s, b)[3]
                t = F.relu(conv(x, p + "conv1"))
                t = F.relu(conv(t, p + "conv2", stride, 1))
                idn = conv(x, p + "downsample", stride) if b == 0 else x
                x = F.relu(conv(t, p + "conv3") + idn)
            stages[f"layer{s + 1}"] = x
        raw, l2 = _tail(x, w["head.weight"], w["head.bias"], cfg.gem_p)
    return (raw, l2, stages) if return_stages else (raw, l2)


def forward_unfolded(state: dict, cfg, frames: torch.Tensor):
    """The same model from a torchvision-named state dict (``backbone.*``, ``embeddings.1.*``) with eval-mode F.batch_norm"""
    w = {k: _t(v) for k, v in state.items()}

    def cbn(x, conv, bn, stride=1, pad=0):
        y = F.conv2d(x, w[conv + ".weight"], None, stride=stride, padding=pad)
        return F.batch_norm(y, w[bn + ".running_mean"], w[bn + ".running_var"], w[bn + ".weight"], w[bn + ".bias"], False, 0.0, cfg.bn_eps)

    with torch.no_grad():
        x = F.max_pool2d(F.relu(cbn(frames, "backbone.conv1", "backbone.bn1", 2, 3)), 3, 2, 1)
        for s in range(4):
            for b in range(cfg.depths[s]):
                p = f"backbone.layer{s + 1}.{b}."
                stride = cfg.block_io(s, b)[3]
                t = F.relu(cbn(x, p + "conv1", p + "bn1"))
                t = F.relu(cbn(t, p + "conv2", p + "bn2", stride, 1))
                idn = cbn(x, p + "downsample.0", p + "downsample.1", stride) if b == 0 else x
                x = F.relu(cbn(t, p + "conv3", p + "bn3") + idn)
        return _tail(x, w["embeddings.1.weight"], w["embeddings.1.bias"], cfg.gem_p)
