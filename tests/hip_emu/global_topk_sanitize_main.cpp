// A stand-alone program around the emulated csrc/global_topk.hip for a host sanitizer run:
//   python tests/hip_emu_build.py global_topk
// builds it with -fsanitize=address,undefined (global_topk_emu.inc is the emulated source) and runs it;
// tests/test_global_topk_emulated.py starts it once as a child process.
// Every operand is a hipMalloc buffer of exactly the size the contract states (an access one element outside is an error):
// vsc_global_topk_f32 at n = 2049 (a tile + 1, every seventh entry padding) with want = 700, then vsc_pair_first_hits on 2049
// hits.  It checks only what needs no second implementation: the counts, scores descending with equal scores in input order,
// no padding selected, rows = position / stride, positions ascending and each the first of its pair.
#include "global_topk_emu.inc"

static uint32_t g_seed = 2049u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

template <class T> static T *dev(size_t count) { void *p = nullptr; hipMalloc(&p, count * sizeof(T)); return (T *)p; }

int main() {
    const int64_t n = 2049, want = 700, stride = 5;
    float *scores = dev<float>(n), *out_scores = dev<float>(want);
    int64_t *ids = dev<int64_t>(n), *out_rows = dev<int64_t>(want), *out_ids = dev<int64_t>(want), *count = dev<int64_t>(1);
    for (int64_t p = 0; p < n; ++p) {
        scores[p] = (float)(rnd() % 97) * 0.25f - 12.0f;          // 97 values: ties at the cut and in every digit pass
        ids[p] = p % 7 == 3 ? -1 : p;                             // the id is the position: the outputs can be traced back
    }
    if (vsc_global_topk_f32(scores, nullptr, ids, n, (int32_t)stride, want, out_rows, out_ids, out_scores, count, nullptr) != 0) return 1;
    if (*count != want) return 2;
    for (int64_t i = 0; i < want; ++i) {
        const int64_t p = out_ids[i];
        if (p < 0 || p >= n || p % 7 == 3 || out_rows[i] != p / stride || out_scores[i] != scores[p]) return 3;
        if (i && (out_scores[i - 1] < out_scores[i] || (out_scores[i - 1] == out_scores[i] && out_ids[i - 1] >= p))) return 4;
    }
    int64_t better = 0;                                            // valid entries that beat the last one selected: all of them are in
    for (int64_t p = 0; p < n; ++p) better += p % 7 != 3 && scores[p] > out_scores[want - 1];
    if (better >= want) return 5;

    const int32_t nqv = 9, nrv = 11;
    int64_t *rows = dev<int64_t>(n), *hits = dev<int64_t>(n), *pos = dev<int64_t>(n);
    int32_t *qv = dev<int32_t>(300), *rv = dev<int32_t>(500);
    for (int r = 0; r < 300; ++r) qv[r] = (int32_t)(rnd() % nqv);
    for (int r = 0; r < 500; ++r) rv[r] = (int32_t)(rnd() % nrv);
    for (int64_t p = 0; p < n; ++p) rows[p] = rnd() % 300, hits[p] = p % 11 == 5 ? -1 : (int64_t)(rnd() % 500);
    if (vsc_pair_first_hits(rows, hits, n, qv, rv, nrv, -1, pos, count, nullptr) != 0) return 6;
    if (*count < 1 || *count > nqv * nrv) return 7;
    std::vector<int64_t> first(nqv * nrv, -1);
    for (int64_t p = n - 1; p >= 0; --p)
        if (hits[p] >= 0) first[qv[rows[p]] * nrv + rv[hits[p]]] = p;
    int64_t pairs = 0;
    for (int64_t f : first) pairs += f >= 0;
    if (*count != pairs) return 8;
    for (int64_t i = 0; i < *count; ++i) {
        const int64_t p = pos[i];
        if (p < 0 || p >= n || hits[p] < 0 || first[qv[rows[p]] * nrv + rv[hits[p]]] != p || (i && pos[i - 1] >= p)) return 9;
    }
    const int64_t found = *count;
    int64_t *pos3 = dev<int64_t>(3);                               // a limit: the output holds min(n, limit) positions
    if (vsc_pair_first_hits(rows, hits, n, qv, rv, nrv, 3, pos3, count, nullptr) != 0 || *count != 3) return 10;
    if (pos3[0] != pos[0] || pos3[1] != pos[1] || pos3[2] != pos[2]) return 11;
    for (void *p : {(void *)scores, (void *)out_scores, (void *)ids, (void *)out_rows, (void *)out_ids, (void *)count, (void *)rows, (void *)hits,
                    (void *)pos, (void *)pos3, (void *)qv, (void *)rv})
        hipFree(p);
    printf("global_topk emulated under the sanitizers: ok (%lld of %lld entries, %lld pairs)\n", (long long)want, (long long)n, (long long)found);
    return 0;
}
