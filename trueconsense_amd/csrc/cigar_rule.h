// cigar_rule.h — which CIGAR a kept record may have, stated once for the kernels (pack_device.hip: classify_view; pack_device.h:
// kept_span), the host packer (host_pack.cpp: classify_slice, the body of tcmi_host_select; tcmi_host_piles_up and
// tcmi_reads_extent, which refuse nothing, do not ask it) and host programs that check them
// (tests/cigar_rule_main.cpp): it includes no HIP header and compiles with any C++ compiler.  All arithmetic is 64-bit integer.
//   the sums       span = the lengths of the ops that consume the reference (M 0, D 2, N 3, = 7, X 8), Yq = the lengths of the ops that
//                  consume the query (M 0, I 1, S 4, = 7, X 8).  Op codes 9-15 consume neither (htslib's bam_cigar_type agrees), an op
//                  of length 0 counts nothing; neither is refused.  At most 65 535 ops of 28 bits: both sums stay below 2^44.
//   the verdict    a record that would otherwise be kept — FLAG 0x4 clear, through the read filter, pos >= 0, on a reference that piles
//                  up, span > 0 — is MALFORMED when Yq >= TCMI_CIGAR_MAX_QUERY = 2^29 (the bound of the one axis, WALK_MAX_COL): the
//                  file or the upload is refused.  A record that is ignored anyway is not judged.  Below the bound nothing is asked of
//                  Yq against l_seq: a query index at or beyond l_seq reads as N with quality 0, bases behind Yq are ignored.
//   why            the kernels that walk a kept record keep its query index in 32 bits (DESIGN: "CIGARs no aligner writes") and guard
//                  every base and quality fetch with a signed `index < l_seq`: nine S ops of 2^28 - 1 make the index negative, seventeen
//                  make it positive again.  Under the rule the index of a kept record stays below 2^29.
#pragma once
#include <stdint.h>

#include "variants_rule.h"

#define TCMI_CIGAR_HD TCMI_VAR_HD

#define TCMI_CIGAR_MAX_QUERY ((int64_t)1 << 29)

struct tcmi_cigar_sums { int64_t span, yq; };

TCMI_CIGAR_HD inline bool tcmi_cigar_op_ref(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }
TCMI_CIGAR_HD inline bool tcmi_cigar_op_query(uint32_t op) { return op == 0 || op == 1 || op == 4 || op == 7 || op == 8; }

// one CIGAR word (len << 4 | op) into the sums: what a walk that looks at the words anyway (classify_view) calls per word
TCMI_CIGAR_HD inline void tcmi_cigar_add(tcmi_cigar_sums &s, uint32_t word)
{
    const uint32_t op = word & 0xFu;
    const int64_t len = word >> 4;
    if (tcmi_cigar_op_ref(op)) s.span += len;
    if (tcmi_cigar_op_query(op)) s.yq += len;
}

// ld(k): CIGAR word k — the device's unaligned loads and the host's aligned words share the walk
template <class Ld> TCMI_CIGAR_HD inline tcmi_cigar_sums tcmi_cigar_walk(Ld ld, uint32_t n)
{
    tcmi_cigar_sums s = {0, 0};
    for (uint32_t k = 0; k < n; ++k) tcmi_cigar_add(s, ld(k));
    return s;
}

// the verdict on a record that would otherwise be kept (the caller has decided that; span > 0 is asked here)
TCMI_CIGAR_HD inline bool tcmi_cigar_malformed(const tcmi_cigar_sums &s) { return s.span > 0 && s.yq >= TCMI_CIGAR_MAX_QUERY; }

// The verdict needs Yq only up to the bound.  A kernel at its register ceiling (pk_index; the counting kernels behind kept_span, two of
// which lose a wavefront per SIMD to one more scalar register) carries 32 bits beside the span it sums anyway:
//   yr = min(Yq - 2^29, 0), from TCMI_CIGAR_YR0 = -2^29: the room that is left below the bound, negative while there is some.
// A length is below 2^28, so yr + len cannot wrap; once yr is 0 it stays 0, however far the 64-bit sum goes (2^32 + 3 included).  Every
// constant of the step and of the verdict is 0 or fits an instruction's literal: none is kept in a scalar register across the walk.
#define TCMI_CIGAR_YR0 (-((int32_t)1 << 29))
TCMI_CIGAR_HD inline void tcmi_cigar_step(int64_t &span, int32_t &yr, uint32_t word)
{
    // bit `op` of 0x018D: consumes the reference (0, 2, 3, 7, 8); bit 16 + `op` of 0x0193 << 16: consumes the query (0, 1, 4, 7, 8)
    const uint32_t bits = 0x0193018Du >> (word & 0xFu), len = word >> 4;
    span += (int64_t)(len & (0u - (bits & 1u)));
    const int32_t y = yr + (int32_t)(len & (0u - ((bits >> 16) & 1u)));
    yr = y < 0 ? y : 0;
}
TCMI_CIGAR_HD inline bool tcmi_cigar_malformed(int64_t span, int32_t yr) { return span > 0 && yr >= 0; }
