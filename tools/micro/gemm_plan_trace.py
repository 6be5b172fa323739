"""Which GEMM kernels a build of the library launches, with what grid, workgroup and LDS (run on the GPU box).

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/micro/gemm_plan_trace.py
    python tools/micro/gemm_plan_trace.py --reduce OUT > trace.txt

The run sends, once each and on one stream: every GEMM of tests/gemm_plan_cases.py that the kernel-level wrappers reach
(ops.gemm_bf16, ops.gemm_resadd_ln_bf16 with VSC_GEMM_LN_TAIL unset and set, ops.gemm_ln_bf16), the shapes the kernel tests of
tests/test_gpu_kernels.py had before they asserted their plan, one ViT-B/16 forward of 332 frames with fuse_ln off and one with it
on (the LayerNorm-folding kinds are reachable no other way), and one Swin-V2-B forward of 256 frames.  --reduce prints the
dispatches in order as `kernel grid workgroup lds`, the first ones labelled with their case: two builds that choose the same
kernels give the same text.  Another build: VSC_HIP_LIB / VSC_HIP_LIB_F16, or PYTHONPATH to another tree's package."""
import csv
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path += [os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "vsc22-submission_amd")]   # (behind PYTHONPATH: another tree's package wins)
import gemm_plan_cases as C  # noqa: E402

# (name, epilogue, m, n, k, tokens): what tests/test_gpu_kernels.py called "the short-K tile choices" and its epilogue cases
OLD_TEST_SHAPES = [("store", "BF16", 1500, 384, 128, 0), ("store", "BF16", 2049, 512, 256, 0), ("store", "BF16", 1300, 128, 512, 0),
                   ("store", "BF16", 1025, 1032, 192, 0), ("store", "BF16", 5043, 2304, 768, 0), ("activation", "GELU_BF16", 1100, 3072, 768, 0),
                   ("activation", "QGELU_BF16", 1333, 512, 128, 0), ("residual", "RESADD_F32", 517, 768, 3072, 0),
                   ("residual", "RESADD_F32", 1300, 768, 768, 0), ("residual", "RESADD_F32", 1100, 512, 256, 0),
                   ("patch", "PATCH_F32", 48, 128, 768, 17)]


def kernel_cases():
    """(label, entry, arguments) in the order they are launched: one GEMM-class kernel each"""
    out = []
    for name, entry, args in C.model_gemms():
        if entry == "gemm" and args[3] <= C.EPI["F32"]:
            tokens = C.VIT[name.split("/")[0]][0] if args[3] == C.EPI["PATCH_F32"] else 0
            out.append((name, "gemm", (*args[:4], tokens)))
        elif entry == "resadd_ln":
            out += [(name, "resadd_ln", (*args, None)), (name + "+LN_TAIL", "resadd_ln", (*args, "1"))]
        elif entry == "gemm_ln" and args[3] == 0:
            out.append((name, "gemm_ln", args[:3]))
    return out + [(f"test_{t}/{m}x{n}x{k}", "gemm", (m, n, k, C.EPI[e], tokens)) for t, e, m, n, k, tokens in OLD_TEST_SHAPES]


def run():
    import torch
    from tools import synth
    from vsc_hip import _lib, ops
    from vsc_hip.config import get_config
    from vsc_hip.encoder import HipEncoder
    from vsc_hip.swin_config import get_swin_config
    from vsc_hip.swin_encoder import SwinHipEncoder
    dev = torch.device("cuda:0")
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
    for name, entry, args in kernel_cases():
        m, n, k = args[:3]
        a, w = z(m, k, dtype=torch.bfloat16), z(n, k, dtype=torch.bfloat16)
        if entry == "gemm":
            e, tokens = args[3:]
            aux = z(tokens, n) if tokens else z(m, n) if e == C.EPI["RESADD_F32"] else None
            ops.gemm_bf16(a, w, z(n), epilogue=e, aux=aux, tokens=tokens)
        elif entry == "resadd_ln":
            _lib.set_option("VSC_GEMM_LN_TAIL", args[3])
            ops.gemm_resadd_ln_bf16(a, w, z(n), z(m, n), z(n), z(n), 1e-6)
            _lib.set_option("VSC_GEMM_LN_TAIL", None)
        else:
            ops.gemm_ln_bf16(a, w, z(n), z(n), z(n), 1e-6, x_in=z(m, n))
        torch.cuda.synchronize()
        del a, w
    print(f"{len(kernel_cases())} kernel-level cases", flush=True)
    cfg = get_config("vit_b16_224")
    weights = synth.encoder_weights(7, cfg)
    frames = torch.from_numpy(synth.frames(1, 4, cfg)).to(dev).repeat(83, 1, 1, 1)
    for fuse_ln in (0, 1):
        enc = HipEncoder(cfg, weights, max_batch=332, l2_normalize=True, lanes=1, fuse_ln=fuse_ln)
        enc(frames)
        torch.cuda.synchronize()
        enc.close()
        print(f"ViT-B/16 forward, 332 frames, fuse_ln {fuse_ln}", flush=True)
    scfg = get_swin_config("swinv2_base_256")
    senc = SwinHipEncoder(scfg, synth.swin_weights(5, scfg), max_batch=256, l2_normalize=True)
    senc(torch.from_numpy(synth.swin_frames(1, 8, scfg)).to(dev).repeat(32, 1, 1, 1))
    torch.cuda.synchronize()
    print("Swin-V2-B forward, 256 frames", flush=True)


def reduce(folder):
    files = sorted(glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True))
    assert files, f"no *kernel_trace.csv under {folder}"
    rows = [r for f in files for r in csv.DictReader(open(f))]
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))
    labels = iter(name for name, _, _ in kernel_cases())
    short = lambda name: re.sub(r"\(anonymous namespace\)::|^void |\(.*$| \[clone .*$", "", name)
    for r in rows:
        name = short(r["Kernel_Name"])
        grid = "x".join(r[f"Grid_Size_{d}"] for d in "XYZ")
        wg = "x".join(r[f"Workgroup_Size_{d}"] for d in "XYZ")
        label = next(labels, "") if re.match(r"gemm_bf16|gemm_ln_kernel", name) else ""
        print(f"{name} grid {grid} workgroup {wg} lds {r['LDS_Block_Size']}" + (f"    # {label}" if label else ""))


if __name__ == "__main__":
    reduce(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "--reduce" else run()
