// What csrc/view_decide.hip needs beyond tests/hip_emu/common.h (which stays as it is), for tests/test_view_decide_emulated.py only:
// the header's constants, the kernel's dynamic LDS as a static buffer of the device's size, and the rounding functions of <cmath>
// under the names the device code uses.
#pragma once
#include "common.h"
#define VSC_VIEW_DECIDE_MAX_SIDE 4096
#define VSC_VIEW_DECIDE_MAX_SAMPLES 255
#define VSC_VIEW_DECIDE_MAX_VIEWS 64
#define VSC_VIEW_DECIDE_STACK 64
#define VSC_VIEW_DECIDE_CHUNK 64
alignas(16) static unsigned char vd_smem[163840];
using std::floor;
using std::rint;
