// Stand-alone program (tests/test_gemm_plan_cpu.py builds it with -fsanitize=address,undefined and starts it as a child process):
// the sweep of tests/gemm_plan_shim.cpp for 64, 256 and 304 CUs, and every plan entry at the extremes of its arguments, where a
// span or tile count could overflow.
#include <cstdio>
#include <initializer_list>

#include "gemm_plan_shim.cpp"

int main() {
    int failed = 0;
    for (int cus : {64, 256, 304}) {
        const long long tails = plan_tail_sweep(cus);
        std::printf("cus %d: %lld shapes take the tail form\n", cus, tails);
        failed += tails <= 0;
    }
    const int sw[12] = {};
    long long out[11];
    for (long long m : {1ll, 1023ll, 1ll << 20, (1ll << 31) - 1, 1ll << 37})
        for (int n : {4, 128, 512, 768, 1 << 20})
            for (int k : {64, 512, 3072, 1 << 20}) {
                for (int epi = 0; epi <= 9; ++epi) plan_gemm(m, n, k, epi, epi >= 6 && epi <= 8, k / 64, 256, sw, out);
                plan_resadd_ln(m, n, k, 256, sw, out);
                plan_gemm_ln(m, n, k, 0, 256, 1, sw, out);
            }
    std::printf(failed ? "FAILED\n" : "ok\n");
    return failed;
}
