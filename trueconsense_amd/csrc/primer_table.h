// primer_table.h — HOST, GPU-free: an amplicon scheme's primers compiled into the two segment lists the kernels search
// (tcmi_ctx_set_primers; include/tcmi.h has the rule).  No HIP header: tests/primer_table_main.cpp builds it with a plain compiler.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

// A read whose first column p lies in [a, b) of a HEAD segment has its tokens on columns < v masked (v = the largest `end` over the
// '+' primers with start - slack <= p < end); a read whose last column q lies in [a, b) of a TAIL segment has its tokens on columns
// >= v masked (v = the smallest `start` over the '-' primers with start <= q < end + slack).  Each list is sorted by a, its segments
// are disjoint, and neighbours of equal value are one segment.
struct tcmi_pseg {
    int32_t a, b, v;
};

constexpr int32_t TCMI_PRIMERS_MAX = 65536;     // primers of one table
constexpr int32_t TCMI_PRIMER_SLACK_MAX = 1000;
constexpr int64_t TCMI_PRIMER_POS_MAX = (int64_t)1 << 29;      // coordinates stay below it (the packed set's event words: TCMI_F_EVPOS)

// 0 and the two lists filled, or -1 and `msg` worded (the argument limits of tcmi_ctx_set_primers)
int tcmi_primers_build(int32_t n, const int64_t *start, const int64_t *end, const int32_t *reverse, int32_t slack, std::vector<tcmi_pseg> &head,
                       std::vector<tcmi_pseg> &tail, char *msg, size_t msg_cap);

// the lookup of the kernels (pack_device.hip: seg_find), on the host: the value of the segment that holds x, or `none`
int32_t tcmi_pseg_find(const tcmi_pseg *seg, int32_t n, int32_t x, int32_t none);
