// csrc/view_decide.hip's own beside tests/hip_emu/common.h: the rounding functions of <cmath> under the names the device code uses.
#pragma once
#include "common.h"
using std::floor;
using std::rint;
