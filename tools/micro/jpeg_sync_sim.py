"""Self-synchronisation of JPEG sub-streams, simulated on the CPU (numpy only; DESIGN.md 4.19 quotes the output):
      python tools/micro/jpeg_sync_sim.py
For every frame and sub-stream size: how many sub-streams the segment is cut into (raw bytes), how many exit states are already
the true ones after the speculative round (sub-stream i started at bit 8 * i * sub_bytes, slot 0 of the MCU, "one bit on" at an
impossible code), and how many verification rounds it takes until a round changes no exit -- the number vsc_jpeg_decode_split's
``rounds`` has to reach for the frame to be decoded in parallel.  The rule is tests/jpeg_split_contract.py's, which the kernels of
csrc/jpeg_split.hip are tested against.  Frames: the benchmark's (tools/micro/jpeg_decode_bench.py) and the test cases'."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (os.path.join(ROOT, "vsc22-submission_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools", "micro"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def simulate(label, data, sub_bytes):
    import jpeg_split_contract as contract
    from vsc_hip import jpeg
    f = jpeg.parse(data)
    seg = data[f.seg_start:f.seg_end]
    n = -(-len(seg) // sub_bytes)
    exits, _, _ = contract.substreams(f, seg, sub_bytes, n)
    right = sum(a == b for a, b in zip(exits[0], exits[-1]))
    rounds = max([r for r in range(1, n + 1) if exits[r] != exits[r - 1]] + [0]) + 1
    print(f"| {label} ({len(seg) / 1e3:.1f} kB) | {sub_bytes} | {n} | {right} | {rounds} |")


def main():
    import jpeg_decode_bench as bench
    import jpeg_decode_cases as cases
    print("| frame | sub-stream bytes | sub-streams | right after the speculative round | rounds until a round changes nothing |")
    print("|---|---|---|---|---|")
    for name, h, w in bench.SHAPES:
        for q in bench.QUALITIES:
            files, _ = bench.jpg_files(h, w, q, n=2)
            for i, data in enumerate(files):
                for sub_bytes in (1024, 512) if h >= 720 else (1024, 512, 256, 128):
                    simulate(f"synth {name} q{q} [{i}]", data, sub_bytes)
    for sub_bytes in (1024, 256):
        simulate("360x640_420", cases.files("360x640_420")[0], sub_bytes)
    for name in ("37x53_420", "37x53_444", "37x53_422", "37x53_gray", "noise_q75"):
        simulate(name, cases.files(name)[0], 64)
    for sub_bytes in (32, 64):
        simulate("noise_q100[0]", cases.files("noise_q100")[0], sub_bytes)


if __name__ == "__main__":
    main()
