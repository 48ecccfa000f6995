// intervals_rule.h — the amplicon table's record and its argument checks (--amplicon-table; include/tcmi.h, tcmi_interval_stats_dev),
// GPU-free: shared by the kernel (intervals.hip), by the library's host code and by host programs that check them
// (tests/amplicons_main.cpp).  It includes no HIP header and compiles with any C++ compiler.  All arithmetic is integer.
#pragma once
#include <stdint.h>

#include "../../include/tcmi.h"

#if defined(__HIP__)
#define TCMI_IV_HD __attribute__((host)) __attribute__((device))
#else
#define TCMI_IV_HD
#endif

static_assert(sizeof(tcmi_interval_stat) == 32, "tcmi_interval_stat is 32 bytes: two 16-byte stores");

constexpr int32_t TCMI_IV_MAX_N = 65536;                    // intervals of one call
constexpr int64_t TCMI_IV_MAX_END = (int64_t)1 << 29;       // an interval ends at or below this column
constexpr int TCMI_IV_STAGE = TCMI_INTERVAL_STAGE;          // columns of an interval the kernel stages in LDS; a longer one is selected from L2

// depths are compared as signed int32: with the sign bit flipped their order is the order of unsigned words (the radix selection)
TCMI_IV_HD inline uint32_t tcmi_iv_flip(int32_t depth) { return (uint32_t)depth ^ 0x80000000u; }
TCMI_IV_HD inline int32_t tcmi_iv_unflip(uint32_t word) { return (int32_t)(word ^ 0x80000000u); }

// (depth, position) as one 64-bit key: the smallest key is the smallest depth at its FIRST position (positions are below 2^31)
TCMI_IV_HD inline int64_t tcmi_iv_key(int32_t depth, int64_t pos) { return (int64_t)(((uint64_t)(uint32_t)depth << 32) | (uint64_t)(uint32_t)pos); }

// the checks of every entry point that takes intervals.  -> 0: fine; 1: n outside 0..65536; 2: min_depth < 0; 3: an interval with
// start < 0, end < start or end > 2^29 (*bad = its index); 4: n > 0 without both arrays
inline int tcmi_intervals_check(int64_t n, const int64_t *start, const int64_t *end, int32_t min_depth, int64_t *bad)
{
    if (bad) *bad = -1;
    if (n < 0 || n > TCMI_IV_MAX_N) return 1;
    if (min_depth < 0) return 2;
    if (n > 0 && (!start || !end)) return 4;
    for (int64_t i = 0; i < n; ++i)
        if (start[i] < 0 || end[i] < start[i] || end[i] > TCMI_IV_MAX_END) {
            if (bad) *bad = i;
            return 3;
        }
    return 0;
}
