// strand_rule.h — the strand verdict of --variant-strand (include/tcmi.h: tcmi_strand_verdict), GPU-free: it includes no HIP header and
// compiles with any C++ compiler, so the library's writer (variants_strand_text.cpp) and host programs that check it
// (tests/strand_main.cpp) share it.  All arithmetic is integer.
#pragma once
#include <cstdint>

#include "../../include/tcmi.h"

static_assert(sizeof(tcmi_strand_counts) == 64, "tcmi_strand_counts is sixteen int32");

enum { TCMI_STRAND_PASS = 0, TCMI_STRAND_BIAS = 1, TCMI_STRAND_LOW = 2 };

inline bool tcmi_strand_args_ok(int32_t min_strand_depth, int64_t num, int64_t den)
{
    return min_strand_depth >= 1 && den >= 1 && den <= 1000000 && num >= 0 && num <= den;
}

// LOW iff a strand's depth is below min_strand_depth; else BIAS iff the smaller of the two cross-multiplied strand frequencies lies below
// num / den of the larger.  alt * tot is below 2^62 and den below 2^20: the products of the comparison need more than 64 bits.
inline int tcmi_strand_rule(int32_t alt_fwd, int32_t alt_rev, int32_t tot_fwd, int32_t tot_rev, int32_t min_strand_depth, int64_t num, int64_t den)
{
    if (!tcmi_strand_args_ok(min_strand_depth, num, den) || alt_fwd < 0 || alt_rev < 0 || tot_fwd < 0 || tot_rev < 0) return TCMI_E_ARG;
    if (tot_fwd < min_strand_depth || tot_rev < min_strand_depth) return TCMI_STRAND_LOW;
    const uint64_t x = (uint64_t)alt_fwd * (uint64_t)tot_rev, y = (uint64_t)alt_rev * (uint64_t)tot_fwd;
    const unsigned __int128 lo = x < y ? x : y, hi = x < y ? y : x;
    return lo * (unsigned __int128)(uint64_t)den < hi * (unsigned __int128)(uint64_t)num ? TCMI_STRAND_BIAS : TCMI_STRAND_PASS;
}
