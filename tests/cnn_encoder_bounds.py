"""Error figures of the CNN encoder's end-to-end parity tests (tests/test_gpu_cnn_encoder.py), in the manner of parity_bounds.py.

All values are measured on the GPU against the FIXTURES (tests/golden/cnn_<preset>.npz: HF ResNetModel + the reference's head
classes in fp32), not against another run of the code under test; tools/cnn_encoder_stats.py prints them.
A case is "<operand type>/<preset>/<fixture case>".  Per case: (max |d|, mean |d|, |mean d|) over all frames and dimensions of the
L2-normalised descriptors, d = HIP - fixture.
    fp16 operands:  max |d| <= 1e-3 (DESC_L2_ATOL, the project's tolerance) -- promised
    bf16 operands:  max |d| <= max(1e-3, 1.5 x measured) -- measured, not promised (every measured maximum is below 1e-3)
    both:           mean |d| <= 1.15 x measured,  |mean d| <= max(2 x measured, 1e-5)
Block outputs and the residual are in the operand type: fp16 meets 1e-3 that way by a factor of 8.  (An fp32 stream, measured once
with the same tool and then taken out, gave fp16 maxima of 2.9e-5 - 8.8e-5 and bf16 maxima of 2.3e-4 - 6.3e-4.)
"""
import numpy as np

DESC_L2_ATOL = 1e-3
MEAN_SLACK, BIAS_SLACK, BIAS_FLOOR, BF16_MAX_SLACK = 1.15, 2.0, 1e-5, 1.5

# case -> (max |d|, mean |d|, |mean d|) measured
MEASURED = {
    "bf16/cnn_tiny/0": (7.270e-04, 2.036e-04, 4.779e-06), "bf16/cnn_tiny/1": (5.818e-04, 1.802e-04, 1.111e-05),
    "fp16/cnn_tiny/0": (1.263e-04, 2.672e-05, 1.023e-06), "fp16/cnn_tiny/1": (7.784e-05, 2.313e-05, 4.938e-07),
    "bf16/sscd_resnet50/0": (3.560e-04, 8.143e-05, 3.643e-06), "bf16/sscd_resnet50/1": (2.486e-04, 6.504e-05, 1.009e-06),
    "bf16/sscd_resnet50/2": (4.120e-04, 1.009e-04, 3.106e-06),
    "fp16/sscd_resnet50/0": (4.200e-05, 1.061e-05, 3.131e-07), "fp16/sscd_resnet50/1": (3.460e-05, 7.865e-06, 3.407e-07),
    "fp16/sscd_resnet50/2": (6.110e-05, 1.235e-05, 2.161e-07),
}
# backbone.layer3.2.conv2.weight x 1.01 on sscd_resnet50 case 0 (same tool): fp16 (1.013e-04, 1.891e-05, 5.095e-07) -- mean |d| 1.78 x the
# unperturbed value, outside the bound; bf16 (3.572e-04, 8.622e-05, 2.894e-06) -- mean |d| 1.06 x, INSIDE the 1.15 x bound: bf16's own
# rounding noise (8.1e-5) hides a shift of that size (about 1.6e-5), fp16's (1.1e-5) does not.


def stats(out, ref):
    d = np.asarray(out, np.float64) - np.asarray(ref, np.float64)
    return float(np.abs(d).max()), float(np.abs(d).mean()), float(abs(d.mean()))


def max_bound(case):
    return DESC_L2_ATOL if case.startswith("fp16/") else max(DESC_L2_ATOL, BF16_MAX_SLACK * MEASURED[case][0])


def mean_bounds(case):
    _, m, b = MEASURED[case]
    return MEAN_SLACK * m, max(BIAS_SLACK * b, BIAS_FLOOR)


def check(case, out, ref):
    mx, mean_abs, bias = stats(out, ref)
    print(f"{case}: max |d| {mx:.3e}, mean |d| {mean_abs:.3e}, |mean d| {bias:.3e}")
    assert mx <= max_bound(case), f"{case}: max |HIP - fixture| = {mx:.3e} > {max_bound(case):.3e}"
    mb, bb = mean_bounds(case)
    assert mean_abs <= mb, f"{case}: mean |HIP - fixture| = {mean_abs:.3e} > {mb:.3e} (measured {MEASURED[case][1]:.3e})"
    assert bias <= bb, f"{case}: |mean (HIP - fixture)| = {bias:.3e} > {bb:.3e} (measured {MEASURED[case][2]:.3e})"
