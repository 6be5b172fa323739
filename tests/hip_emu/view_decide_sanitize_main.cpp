// A stand-alone program around the emulated csrc/view_decide.hip for a host sanitizer run (it is no part of the test suite):
//   python tests/hip_emu_build.py view_decide
// builds it with -fsanitize=address,undefined (view_decide_emu.inc is the emulated source) and runs it.
// Seeded maps of 1 .. 300 pixels on a side -- plain, letterboxed, stacked, a 2 x 2 grid, thin ones around 8192 pixels -- in two flat
// buffers at odd offsets, exactly sized allocations (an access one element outside any operand is an error), then the refusals.  It
// checks only what needs no second implementation: status 0 or 1, counts in range, boxes inside the frame and non-empty, tails of -1.
#include "view_decide_emu.inc"

static uint32_t g_seed = 12345u;
static double rnd() { g_seed = g_seed * 1664525u + 1013904223u; return (double)(g_seed >> 8) * (1.0 / 16777216.0); }

struct Map { int h, w, m, n, kind; };   // kind 0 plain, 1 letterbox, 2 three stacked panels, 3 a 2 x 2 grid

static bool moving(const Map &p, int y, int x) {
    if (p.kind == 1) return y >= p.h / 8 && y < p.h - p.h / 8;
    if (p.kind == 2) return y % (p.h / 3) < p.h / 3 - 10;
    if (p.kind == 3) return y % (p.h / 2) >= 6 && y % (p.h / 2) < p.h / 2 - 6 && x % (p.w / 2) >= 6 && x % (p.w / 2) < p.w / 2 - 6;
    return true;
}

int main() {
    const Map maps[] = {{1, 1, 1, 8, 0}, {1, 9, 20, 8, 0}, {37, 1, 20, 8, 0}, {7, 41, 5, 8, 0}, {64, 128, 20, 8, 0}, {3, 2731, 7, 9, 0},
                        {150, 190, 20, 4, 1}, {150, 190, 20, 5, 1}, {300, 150, 20, 30, 2}, {300, 300, 13, 12, 3}, {129, 257, 255, 40, 1}};
    const int n = sizeof maps / sizeof maps[0], max_views = 5;
    std::vector<int64_t> items;
    size_t vlen = 0, clen = 0;
    for (int k = 0; k < n; ++k) {
        vlen += 2 * (k % 3) + 1, clen += 2 * (k % 2) + 3;
        const int64_t row[6] = {(int64_t)vlen, (int64_t)clen, maps[k].h, maps[k].w, maps[k].m, maps[k].n};
        items.insert(items.end(), row, row + 6);
        vlen += (size_t)maps[k].h * maps[k].w, clen += (size_t)maps[k].h * maps[k].w;
    }
    double *var = new double[vlen];
    uint16_t *count = new uint16_t[clen];
    for (size_t i = 0; i < vlen; ++i) var[i] = NAN;
    for (size_t i = 0; i < clen; ++i) count[i] = 0xFFFF;
    for (int k = 0; k < n; ++k) {
        const Map &p = maps[k];
        for (int y = 0; y < p.h; ++y)
            for (int x = 0; x < p.w; ++x) {
                const bool on = moving(p, y, x);
                const bool line = on && p.kind && (!moving(p, y - 1 < 0 ? 0 : y - 1, x) || !moving(p, y + 1 >= p.h ? p.h - 1 : y + 1, x));
                var[items[6 * k] + (size_t)y * p.w + x] = on ? 200.0 + 3800.0 * rnd() : 0.04 * rnd();
                count[items[6 * k + 1] + (size_t)y * p.w + x] = (uint16_t)(line ? p.m : on && rnd() < 0.03 ? 1 + (int)(rnd() * p.m) % p.m : 0);
            }
    }
    int32_t *boxes = new int32_t[(size_t)n * max_views * 4], *counts = new int32_t[n], *status = new int32_t[n];
    double *trace = new double[(size_t)n * 8];
    vsc_view_decide *h = nullptr;
    if (vsc_view_decide_create(nullptr, &h) != 0) return 1;
    int split = 0;
    for (int pass = 0; pass < 2; ++pass) {
        memset(boxes, 0x55, (size_t)n * max_views * 16);
        if (vsc_view_decide_f64(h, var, (int64_t)vlen, count, (int64_t)clen, items.data(), n, max_views, boxes, counts, status, pass ? nullptr : trace) != 0) return 2;
        for (int k = 0; k < n; ++k) {
            if (status[k] != 0 && status[k] != 1) return 3;
            if (status[k] ? counts[k] != 0 : (counts[k] < 1 || counts[k] > max_views)) return 4;
            split += counts[k] > 1;
            for (int v = 0; v < max_views; ++v) {
                const int32_t *b = boxes + ((size_t)k * max_views + v) * 4;
                if (v < counts[k] ? !(0 <= b[0] && b[0] < b[1] && b[1] <= maps[k].h && 0 <= b[2] && b[2] < b[3] && b[3] <= maps[k].w)
                                  : !(b[0] == -1 && b[1] == -1 && b[2] == -1 && b[3] == -1)) return 5;
            }
        }
    }
    if (!split) return 6;            // the stacked and the grid maps are there to walk the region stack
    const int64_t big[] = {0, 0, 4097, 1, 20, 8}, past[] = {(int64_t)vlen - 3, 0, 2, 2, 20, 8}, neg[] = {-1, 0, 1, 1, 20, 8}, m0[] = {0, 0, 1, 1, 0, 8};
    if (vsc_view_decide_f64(h, var, (int64_t)vlen, count, (int64_t)clen, big, 1, max_views, boxes, counts, status, nullptr) == 0) return 7;
    if (vsc_view_decide_f64(h, var, (int64_t)vlen, count, (int64_t)clen, past, 1, max_views, boxes, counts, status, nullptr) == 0) return 8;
    if (vsc_view_decide_f64(h, var, (int64_t)vlen, count, (int64_t)clen, neg, 1, max_views, boxes, counts, status, nullptr) == 0) return 9;
    if (vsc_view_decide_f64(h, var, (int64_t)vlen, count, (int64_t)clen, m0, 1, max_views, boxes, counts, status, nullptr) == 0) return 10;
    if (vsc_view_decide_f64(h, var, (int64_t)vlen, count, (int64_t)clen, items.data(), n, 65, boxes, counts, status, nullptr) == 0) return 11;
    if (vsc_view_decide_f64(nullptr, var, (int64_t)vlen, count, (int64_t)clen, items.data(), n, max_views, boxes, counts, status, nullptr) == 0) return 12;
    if (vsc_view_decide_f64(h, nullptr, 0, nullptr, 0, nullptr, 0, max_views, nullptr, nullptr, nullptr, nullptr) != 0) return 13;
    vsc_view_decide_destroy(h);
    delete[] var, delete[] count, delete[] boxes, delete[] counts, delete[] status, delete[] trace;
    printf("view_decide emulated under the sanitizers: ok (%d items, %d split)\n", n, split);
    return 0;
}
