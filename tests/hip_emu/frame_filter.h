// csrc/frame_filter.hip's own beside tests/hip_emu/common.h: a test build may lower the budget by which the launcher chooses between
// adjacency bits in LDS and in the scratch (-DFF_EMU_LDS_BYTES), so that small matrices take the scratch path too.  The launches
// themselves may still ask for the device's LDS: rows on the scratch path keep their per-row state there.
#pragma once
#include "common.h"
#ifdef FF_EMU_LDS_BYTES
#undef VSC_FRAME_FILTER_LDS_BYTES
#define VSC_FRAME_FILTER_LDS_BYTES FF_EMU_LDS_BYTES
#endif
