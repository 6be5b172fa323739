// The slots of the grow-only device scratch (search_scratch_get in common.h).  It includes nothing, of HIP or of the library, so
// that tests/hip_emu/common.h hands the kernels compiled for the host the same slots.
#pragma once

// One owner per slot; two buffers that are live in one call never share one.  The numbers are part of nothing outside the library.
enum SearchScratchSlot {
    // knn.hip, exact fp32 sweeps
    SCRATCH_KNN_Q_F32 = 0, SCRATCH_KNN_R_F32 = 1,   // packed fp32 queries / references (every exact sweep, pair similarity)
    SCRATCH_KNN_LISTS = 2,                          // exact top-k: candidate lists per workgroup
    SCRATCH_KNN_PART = 3,                           // top-k, exact and pre-filter: sorted keys per (query, split)
    SCRATCH_RANGE_COUNTS = 4,                       // range search, exact and pre-filter: hits per (query, split)
    SCRATCH_PAIR_TILES = 5,                         // pair similarity: tile table
    SCRATCH_PAIRMAX_TABLE = 6, SCRATCH_PAIRMAX_COUNTS = 7,   // video-pair maxima: [q videos][r videos] table, entries per row
    // knn.hip, bf16 pre-filter (8-11: unused)
    SCRATCH_PF_QB = 12, SCRATCH_PF_RB = 13,         // packed bf16 queries / references
    SCRATCH_PF_QSTATS = 14, SCRATCH_PF_FLAGS = 15,  // per-query norms; max |r| bits + fallback flags + debug counters
    SCRATCH_PF_LISTS = 16, SCRATCH_PF_CAND = 17, SCRATCH_PF_NCAND = 18,   // sweep lists per workgroup; survivors per (query, split), their number
    SCRATCH_TN_TABLE = 19, SCRATCH_TN_NODES = 20,         // tn_align.hip
    SCRATCH_VIEW_CANNY = 21, SCRATCH_VIEW_RESIZE = 22,    // view_prep.hip; the resize slot also serves frame_inputs.hip's two-pass path
    SCRATCH_MS_TABLE = 23,                                // match_segments.hip
    // global_topk.hip
    SCRATCH_GTK_STATE = 24, SCRATCH_GTK_BLOCKS = 25,      // global top-k: select state; (above, equal) counts per tile
    SCRATCH_GTK_KEYS = 26, SCRATCH_GTK_PAY = 27, SCRATCH_GTK_HIST = 28,   // survivors' keys / positions (two buffers each); [digit][tile] counters
    SCRATCH_PFH_KEYS = 29, SCRATCH_PFH_POS = 30,          // pair first hits: table keys, least position per key
    SCRATCH_PFH_FLAGS = 31, SCRATCH_PFH_BLOCKS = 32,      // first-hit flag per entry; flags per tile
    // uap.hip; the two entries run one after the other and use the slots in turn
    SCRATCH_UAP_STATE = 33,                               // rank: the four status counters
    SCRATCH_UAP_KEYS = 34, SCRATCH_UAP_PAY = 35,          // rank: the sorts' two key buffers; two position buffers + the score keys.  curve: both term lists; (tps, last row) per tie group
    SCRATCH_UAP_HIST = 36, SCRATCH_UAP_TREE = 37,         // rank: [digit][tile] counters.  curve: counts per tile; the pairwise trees' slots
    SCRATCH_FRAME_FILTER_BITS = 38,                       // frame_filter.hip: adjacency bit matrices too large for LDS
    // l2_search.hip; live only inside its own entries, beside the slots of the inner-product sweep they call
    SCRATCH_L2_QAUG = 39, SCRATCH_L2_QNORM = 40,          // augmented queries; their |q|^2 (top-k) / the largest of them (range)
    SCRATCH_L2_RAUG = 41, SCRATCH_L2_RMAX = 42,           // a bank augmented for one call (no caller's copy); its largest |r|^2
    SCRATCH_L2_PROBE_S = 43, SCRATCH_L2_PROBE_I = 44,     // the probe's [nq, kk] scores / ids; range: the sweep's survivors
    SCRATCH_L2_FLAGS = 45, SCRATCH_L2_ROWS = 46,          // certificate per query row; the rows sent to the direct path
    SCRATCH_L2_DIST = 47,                                 // direct path: one materialised [rows, nr] chunk of distance bits
    SCRATCH_L2_COUNTS = 48, SCRATCH_L2_SLIMS = 49,        // range: hits per query row; the sweep's CSR offsets
    SCRATCH_L2_QAUG2 = 50,                                // the augmented queries of the wider probe
    SCRATCH_ALIGN_TABLE = 51, SCRATCH_ALIGN_ARENA = 52,   // vta_align.hip: pair table; the per-pair state of one launch
    SCRATCH_SLOTS
};
