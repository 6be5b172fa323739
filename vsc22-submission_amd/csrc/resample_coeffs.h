// Pillow's 8-bit bicubic resample coefficients, shared by view_prep.hip (vsc_resize_bicubic_u8) and frame_inputs.hip
// (vsc_frame_inputs_u8): the host builder and the process-wide cache of device tables.  Host code only; it includes nothing of
// the library, so that tests/hip_emu/frame_inputs.h can build the same tables on the CPU.
//
// fp64 results must equal Pillow's bit for bit: every file that includes this one switches FMA contraction off first.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

constexpr int RESAMPLE_PRECISION_BITS = 32 - 8 - 2;

// Pillow's bicubic filter (a = -0.5)
inline double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// precompute_coeffs + normalize_coeffs_8bpc for a box (0, in) -> out, on the host
// -> table [out][2 + ksize] int32: first tap, tap count, then the fixed-point weights
inline std::vector<int32_t> resample_coeffs(int in, int out, int *ksize_out) {
    const double scale = (double)in / out;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    std::vector<int32_t> table((size_t)out * (2 + ksize), 0);
    std::vector<double> k(ksize);
    for (int xx = 0; xx < out; ++xx) {
        const double center = 0.0 + (xx + 0.5) * scale;
        const double ss = 1.0 / filterscale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        double ww = 0.0;
        int x = 0;
        for (; x < xmax; ++x) {
            const double wgt = bicubic_filter((x + xmin - center + 0.5) * ss);
            k[x] = wgt;
            ww += wgt;
        }
        for (x = 0; x < xmax; ++x)
            if (ww != 0.0) k[x] /= ww;
        int32_t *row = table.data() + (size_t)xx * (2 + ksize);
        row[0] = xmin;
        row[1] = xmax;
        for (x = 0; x < xmax; ++x)
            row[2 + x] = k[x] < 0 ? (int32_t)(-0.5 + k[x] * (1 << RESAMPLE_PRECISION_BITS)) : (int32_t)(0.5 + k[x] * (1 << RESAMPLE_PRECISION_BITS));
    }
    *ksize_out = ksize;
    return table;
}

// One table on the device and, for planning on the host, the same table in host memory (never freed either).
struct ResampleCoeffs {
    int32_t *dev = nullptr;
    const int32_t *host = nullptr;
    int ksize = 0;
};

// Device copies of the tables, per (device, in length, out length): built and uploaded once (a synchronous copy), then kept for
// the life of the process.  A table is never freed, so a pointer handed out stays valid for every kernel queued with it, on any
// thread or device.  The set is bounded by the distinct crop lengths: ~21 KiB per length at 1080p, and at most ~150 MiB per output
// size even if every length up to 4096 occurs.  Defined in view_prep.hip; `who` prefixes the error text.
int resample_coeffs_get(const char *who, int in, int out, ResampleCoeffs *res);
