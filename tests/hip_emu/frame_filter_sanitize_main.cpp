// A stand-alone program around the emulated csrc/frame_filter.hip for a host sanitizer run (it is no part of the test suite):
//   python tests/hip_emu_build.py frame_filter [-DFF_EMU_LDS_BYTES=2048]
// builds it with -fsanitize=address,undefined (frame_filter_emu.inc is the emulated source) and runs it.
// Seeded asymmetric matrices of 0 .. 300 rows in one flat buffer at odd offsets, exactly sized allocations (an access one element
// outside any operand is an error), then the refusals.  It checks only what needs no second implementation: counts in range, kept
// rows ascending, tails of -1, the visit order a permutation in descending mean.
#include "frame_filter_emu.inc"

static uint32_t g_seed = 12345u;
static float rnd() { g_seed = g_seed * 1664525u + 1013904223u; return (float)(g_seed >> 8) * (1.0f / 16777216.0f); }

int main() {
    const int rows[] = {0, 1, 2, 63, 64, 65, 130, 0, 257, 300, 5};
    const int n = sizeof rows / sizeof rows[0];
    std::vector<int64_t> items;
    size_t len = 0, total = 0;
    for (int k = 0; k < n; ++k) {
        len += 2 * (k % 5) + 3;
        items.push_back((int64_t)len), items.push_back(rows[k]);
        len += (size_t)rows[k] * rows[k];
        total += rows[k];
    }
    float *s = new float[len];
    for (size_t i = 0; i < len; ++i) s[i] = NAN;
    for (int k = 0; k < n; ++k) {
        float *m = s + items[2 * k];
        const int L = rows[k];
        for (int i = 0; i < L; ++i)
            for (int j = 0; j < L; ++j) m[(size_t)i * L + j] = i == j ? 1.0f : (rnd() < 0.02f ? 0.99f : rnd() * 1.1f - 0.2f);
    }
    int32_t *kept = new int32_t[total], *counts = new int32_t[n], *order = new int32_t[total];
    float *means = new float[total];
    vsc_frame_filter *h = nullptr;
    if (vsc_frame_filter_create(nullptr, &h) != 0) return 1;
    for (int pass = 0; pass < 2; ++pass) {
        memset(kept, 0x55, total * 4);
        if (vsc_frame_filter_f32(h, s, (int64_t)len, items.data(), n, 0.975f, kept, counts, pass ? nullptr : means, pass ? nullptr : order) != 0) return 2;
        size_t at = 0;
        for (int k = 0; k < n; ++k) {
            const int L = rows[k];
            if (counts[k] < (L ? 1 : 0) || counts[k] > L) return 3;
            for (int t = 0; t < L; ++t) {
                const int32_t v = kept[at + t];
                if (t < counts[k] ? (v < 0 || v >= L || (t && v <= kept[at + t - 1])) : v != -1) return 4;
            }
            if (!pass) {
                std::vector<char> seen(L, 0);
                for (int t = 0; t < L; ++t) {
                    const int32_t o = order[at + t];
                    if (o < 0 || o >= L || seen[o]) return 5;
                    seen[o] = 1;
                    if (t && means[at + o] > means[at + order[at + t - 1]]) return 6;
                }
            }
            at += L;
        }
    }
    const int64_t bad_rows[] = {0, 4097}, past[] = {(int64_t)len - 3, 2}, neg[] = {-1, 1};
    if (vsc_frame_filter_f32(h, s, (int64_t)len, bad_rows, 1, 0.975f, kept, counts, nullptr, nullptr) == 0) return 7;
    if (vsc_frame_filter_f32(h, s, (int64_t)len, past, 1, 0.975f, kept, counts, nullptr, nullptr) == 0) return 8;
    if (vsc_frame_filter_f32(h, s, (int64_t)len, neg, 1, 0.975f, kept, counts, nullptr, nullptr) == 0) return 9;
    if (vsc_frame_filter_f32(h, s, (int64_t)len, items.data(), n, NAN, kept, counts, nullptr, nullptr) == 0) return 10;
    if (vsc_frame_filter_f32(nullptr, s, (int64_t)len, items.data(), n, 0.975f, kept, counts, nullptr, nullptr) == 0) return 11;
    if (vsc_frame_filter_f32(h, nullptr, 0, nullptr, 0, 0.975f, nullptr, nullptr, nullptr, nullptr) != 0) return 12;
    vsc_frame_filter_destroy(h);
    delete[] s, delete[] kept, delete[] counts, delete[] order, delete[] means;
    printf("frame_filter emulated under the sanitizers: ok (%d items, %zu rows, LDS budget %d)\n", n, total, (int)VSC_FRAME_FILTER_LDS_BYTES);
    return 0;
}
