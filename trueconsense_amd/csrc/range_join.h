// range_join.h — the joining rule of block ranges (include/tcmi.h, tcmi_split_step; distributed.check_range_anchors is the same rule
// in Python).  GPU-free: tests/range_join_main.cpp runs it against the Python twin under AddressSanitizer + UBSan.
#pragma once
#include <cstdint>

// Ranges in rank order, each {first_block, n_blocks, first, next}; a range in the middle of the file starts at the first offset its
// first block finds plausible for a record, and only the range in front can vouch for it: its last record ends there.  inflated: the
// length of the file's stream, where the last record must end (< 0: the ranges are sub-ranges of a rank's range, no end to check).
// -> nullptr, or what does not join, with the range (*who), its offset (*at) and the offset that was expected (*want)
static inline const char *tcmi_ranges_join(const int64_t (*rg)[4], int world, int64_t inflated, int *who, int64_t *at, int64_t *want)
{
    bool have = false, any_before = false;
    int64_t expect = -1;
    for (int r = 0; r < world; ++r) {
        const int64_t fb = rg[r][0], nb = rg[r][1], first = rg[r][2], nxt = rg[r][3];
        if (nb <= 0) continue;
        if (fb != 0 && first >= 0) {
            *who = r; *at = first; *want = expect;
            if (have && first != expect) return "starts a record where the range in front does not end its last one";
            if (!have && any_before) return "starts a record, but no range in front says where its last record ends";
        }
        any_before = true;
        if (nxt >= 0) { expect = nxt; have = true; }
    }
    if (have && inflated >= 0 && expect != inflated) { *who = world - 1; *at = expect; *want = inflated; return "the last alignment record does not end with the file's stream"; }
    return nullptr;
}
