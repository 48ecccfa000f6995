// links_rule.h — the phase verdict of --variant-links (include/tcmi.h: tcmi_link_phase) and the sums of a pair's joint counts,
// GPU-free: it includes no HIP header and compiles with any C++ compiler, so the library's writer (variants_links_text.cpp) and host
// programs that check it (tests/links_main.cpp) share it.  All arithmetic is integer.
#pragma once
#include <cstdint>

#include "../../include/tcmi.h"

static_assert(sizeof(tcmi_link_counts) == 208, "tcmi_link_counts is fifty-two int32");

enum { TCMI_LINK_CIS = 0, TCMI_LINK_TRANS = 1, TCMI_LINK_MIXED = 2, TCMI_LINK_NONE = 3, TCMI_LINK_LOW = 4 };

// the ratio lies in (1/2, 1]: CIS and TRANS exclude each other
inline bool tcmi_link_args_ok(int32_t min_depth, int64_t num, int64_t den)
{
    return min_depth >= 1 && den >= 1 && den <= 1000000 && num <= den && 2 * num > den;
}

// LOW iff fewer than min_depth records span both columns; else with m the smaller of the two alleles' depths among them: NONE iff
// m = 0, CIS iff both >= num / den of m, TRANS iff both <= (1 - num / den) of m, else MIXED.  The counts are below 2^31 and num, den
// at or below 10^6 < 2^20: every product is below 2^52 and fits 64 bits.
inline int tcmi_link_rule(int32_t both, int32_t only_a, int32_t only_b, int32_t span, int32_t min_depth, int64_t num, int64_t den)
{
    if (!tcmi_link_args_ok(min_depth, num, den) || both < 0 || only_a < 0 || only_b < 0 || span < 0) return TCMI_E_ARG;
    if (span < min_depth) return TCMI_LINK_LOW;
    const int64_t da = (int64_t)both + only_a, db = (int64_t)both + only_b, m = da < db ? da : db;
    if (m == 0) return TCMI_LINK_NONE;
    if ((int64_t)both * den >= num * m) return TCMI_LINK_CIS;
    if ((int64_t)both * den <= (den - num) * m) return TCMI_LINK_TRANS;
    return TCMI_LINK_MIXED;
}

// sum_y j[x][y] (the records with class x at the pair's first column) and sum_x j[x][y] (class y at its second)
inline int64_t tcmi_link_row(const tcmi_link_counts &l, int x)
{
    int64_t s = 0;
    for (int y = 0; y < 7; ++y) s += l.j[x][y];
    return s;
}
inline int64_t tcmi_link_col(const tcmi_link_counts &l, int y)
{
    int64_t s = 0;
    for (int x = 0; x < 7; ++x) s += l.j[x][y];
    return s;
}
