// What csrc/segment_metric.hip needs beyond tests/hip_emu/common.h (which stays as it is), for tests/test_segment_metric_emulated.py
// only: the handle's device allocations.  Fresh "device" memory is filled with a NaN pattern, so a kernel that relied on what its
// scratch held would not reproduce the contract.
#pragma once
#include "common.h"
static inline int hipMalloc(void **p, size_t n) { *p = malloc(n ? n : 1); if (*p) memset(*p, 0xFF, n); return *p ? 0 : 1; }
static inline int hipFree(void *p) { free(p); return 0; }
