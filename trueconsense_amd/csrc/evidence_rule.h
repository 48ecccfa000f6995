// evidence_rule.h — the evidence verdict of --variant-evidence (include/tcmi.h: tcmi_evidence_verdict) and the bound that decides whether
// evidence_counts.hip may count in 32-bit LDS counters, GPU-free: it includes no HIP header and compiles with any C++ compiler, so the
// kernel's host side (evidence_counts.hip), the library's writer (variants_evidence_text.cpp) and host programs that check them
// (tests/evidence_main.cpp) share it.  All arithmetic is integer.
#pragma once
#include <cstdint>

#include "../../include/tcmi.h"

static_assert(sizeof(tcmi_evidence_counts) == 200, "tcmi_evidence_counts is 21 int64 and 8 int32");

enum { TCMI_EVIDENCE_PASS = 0, TCMI_EVIDENCE_LOWQ = 1, TCMI_EVIDENCE_LOWMQ = 2, TCMI_EVIDENCE_END = 4 };

inline bool tcmi_evidence_args_ok(int32_t min_qual, int32_t min_mapq, int32_t min_dist)
{
    return min_qual >= 0 && min_qual <= 255 && min_mapq >= 0 && min_mapq <= 255 && min_dist >= 0 && min_dist <= 255;
}

// a bit per sum whose MEAN over the n tokens lies below its threshold: sum < threshold * n.  A threshold of 0 never fails (no sum is
// negative), n = 0 gives 0.  n is any int64: the products are formed in 128 bits.
inline int tcmi_evidence_rule(int64_t n, int64_t qual, int64_t mapq, int64_t dist, int32_t min_qual, int32_t min_mapq, int32_t min_dist)
{
    if (!tcmi_evidence_args_ok(min_qual, min_mapq, min_dist) || n < 0 || qual < 0 || mapq < 0 || dist < 0) return TCMI_E_ARG;
    const __int128 m = n;
    return (qual < min_qual * m ? TCMI_EVIDENCE_LOWQ : 0) | (mapq < min_mapq * m ? TCMI_EVIDENCE_LOWMQ : 0) | (dist < min_dist * m ? TCMI_EVIDENCE_END : 0);
}

// May a workgroup of evidence_counts.hip stage its counters in LDS as uint32?  Yes while the query has at most TCMI_EVIDENCE_LDS columns
// and no counter can pass 2^32 - 1: a record adds at most one token of at most 255 to a counter, and a workgroup of `block` lanes in a
// grid of `grid` workgroups visits at most ceil(ceil(n_records / block) / grid) * block records.
inline bool tcmi_evidence_lds_ok(int64_t n_cols, int64_t n_records, int64_t grid, int64_t block)
{
    if (n_cols < 1 || n_cols > TCMI_EVIDENCE_LDS || n_records < 0 || grid < 1 || block < 1) return false;
    const int64_t blocks = n_records / block + (n_records % block != 0), trips = blocks / grid + (blocks % grid != 0);
    return (__int128)255 * trips * block <= (__int128)UINT32_MAX;
}
