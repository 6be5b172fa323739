"""The streaming ViT attention kernel (csrc/attention_stream.hip) measured, recorded, not a gate:

    python tools/micro/attn_stream_bench.py [--out profiles/attention_stream_bench.txt] [--window 0.5] [--repeats 3] [--skip_model]

How: device events around a window of back-to-back launches, at least `--window` seconds long (the launch count comes from a
calibration run); every shape and contender is warmed up first; N(0, 1) operands, the SAME tensors for every contender; the
contenders of a shape alternate window by window; `--repeats` windows each, all of them on the page.

  (113, 577, 12), (64, 577, 16), (47, 1370, 12) as (frames, tokens, heads): the kernel against
      torch.nn.functional.scaled_dot_product_attention on strided q / k / v views of the same qkv tensor, same dtype, same box (its
      output stays [frames, heads, tokens, 64]: no transpose back is charged to it); us per launch, TF/s from 4 T^2 64 FLOP per
      (frame, head), the share of the 2.5 PF/s dense 16-bit peak, and the HBM floor of qkv in + context out at 8 TB/s.
  (332, 197, 12), (255, 257, 16): the streaming kernel against the register-row kernel (vsc_attention_bf16) it does NOT replace.
  vit_b16_384 at two chunks of its aligned batch (113 frames): frames/s of the HIP encoder next to PyTorch-ROCm running
      transformers.ViTModel + the reference's GeM / Linear head lines with the same weights in the same 16-bit type."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "vsc22-submission_amd"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

from vsc_hip import ops  # noqa: E402

PEAK_16BIT, HBM_BYTES_PER_S = 2.5e15, 8.0e12
LONG = ((113, 577, 12), (64, 577, 16), (47, 1370, 12))
SHORT = ((332, 197, 12), (255, 257, 16))


def window(fn, seconds, launches=None):
    """-> (us per launch, launches): one event pair around `launches` back-to-back calls (calibrated to `seconds` when not given)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if launches is None:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(10):
            fn()
        e1.record()
        torch.cuda.synchronize()
        launches = max(int(seconds / (e0.elapsed_time(e1) / 10 / 1e3)) + 1, 10)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches, launches


def contest(contenders, seconds, repeats):
    """contenders {name: fn} -> {name: [us per launch] * repeats}; warm-up and calibration of all first, then alternating windows"""
    counts = {name: window(fn, seconds)[1] for name, fn in contenders.items()}
    out = {name: [] for name in contenders}
    for _ in range(repeats):
        for name, fn in contenders.items():
            out[name].append(window(fn, seconds, counts[name])[0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_stream_bench.txt"))
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip_model", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"attention_stream_bench: {torch.cuda.get_device_name(0)}, windows >= {args.window} s, {args.repeats} repeats, N(0, 1) operands",
             "us per launch: every repeat; TF/s and shares from the median"]
    say = lambda s: (lines.append(s), print(s, flush=True))
    med = lambda v: sorted(v)[len(v) // 2]
    for precision in ("bf16", "fp16"):
        dtype = torch.bfloat16 if precision == "bf16" else torch.float16
        with ops.operands(precision):
            for shapes, other in ((LONG, "sdpa"), (SHORT, "register-row")):
                for frames, tokens, heads in shapes:
                    g = torch.Generator(device=dev).manual_seed(tokens)
                    qkv = torch.randn(frames * tokens, 3 * heads * 64, generator=g, device=dev).to(dtype)
                    q, k, v = qkv.view(frames, tokens, 3, heads, 64).permute(2, 0, 3, 1, 4)
                    contenders = {"stream": lambda: ops.attention_stream_bf16(qkv, frames, tokens, heads)}
                    if other == "sdpa":
                        contenders["sdpa"] = lambda: F.scaled_dot_product_attention(q, k, v)
                    else:
                        contenders["register-row"] = lambda: ops.attention_bf16(qkv, frames, tokens, heads)
                    res = contest(contenders, args.window, args.repeats)
                    flop = 4.0 * tokens * tokens * 64 * frames * heads
                    floor_us = frames * tokens * heads * 64 * 4 * 2 / HBM_BYTES_PER_S * 1e6
                    for name, us in res.items():
                        m = med(us)
                        say(f"{precision} ({frames}, {tokens}, {heads}) {name:>12}: us {' '.join(f'{u:8.1f}' for u in us)}   median {flop / m / 1e6:7.1f} TF/s "
                            f"= {100 * flop / m / 1e-6 / PEAK_16BIT:5.2f} % of 2.5 PF/s; HBM floor {floor_us:6.1f} us ({100 * floor_us / m:4.1f} % of the time)")
                    del qkv, q, k, v
    if not args.skip_model:
        from tools import synth
        from vsc_hip.config import aligned_batch, get_config
        from vsc_hip.encoder import HipEncoder
        cfg = get_config("vit_b16_384")
        w = synth.encoder_weights(7, cfg)
        batch = aligned_batch(cfg.tokens)
        x = torch.from_numpy(synth.frames(11, 2, cfg)).to(dev).repeat(batch, 1, 1, 1).contiguous()       # 2 x 113 frames: one chunk per lane
        for precision in ("bf16", "fp16"):
            enc = HipEncoder(cfg, w, max_batch=batch, l2_normalize=True, precision=precision)
            us = contest({"hip": lambda: enc(x)}, args.window, args.repeats)["hip"]
            say(f"vit_b16_384 {precision} HIP encoder, {len(x)} frames per call: frames/s {' '.join(f'{len(x) / (u * 1e-6):8.0f}' for u in us)}")
            enc.close()
            try:
                import gen_vit_golden
                from transformers import ViTConfig, ViTModel
                dtype = torch.bfloat16 if precision == "bf16" else torch.float16
                hf = ViTModel(ViTConfig(hidden_size=cfg.width, num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads,
                                        intermediate_size=cfg.mlp_dim, image_size=cfg.image_size, patch_size=cfg.patch_size,
                                        layer_norm_eps=cfg.ln_eps, hidden_act="gelu"), add_pooling_layer=False).eval()
                hf.load_state_dict(gen_vit_golden._to_hf_vit_state(w, cfg), strict=True)
                hf = hf.to(dev).to(dtype)
                hw, hb = torch.from_numpy(w["head.weight"]).to(dev).to(dtype), torch.from_numpy(w["head.bias"]).to(dev).to(dtype)
                xt = x.to(dtype)

                def torch_model():
                    with torch.no_grad():
                        tok = hf(xt).last_hidden_state
                        gem = tok.float().clamp(min=1e-6).pow(3).mean(dim=1).pow(1.0 / 3).to(dtype)
                        return F.normalize((gem @ hw.t() + hb).float())
                us = contest({"torch": torch_model}, args.window, args.repeats)["torch"]
                say(f"vit_b16_384 {precision} PyTorch-ROCm (transformers.ViTModel + head, same weights), {len(x)} frames per call: frames/s "
                    f"{' '.join(f'{len(x) / (u * 1e-6):8.0f}' for u in us)}")
                del hf
            except Exception as exc:  # noqa: BLE001 -- recorded: the yardstick did not run here
                say(f"vit_b16_384 {precision} PyTorch-ROCm: did not run ({type(exc).__name__}: {exc})")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
