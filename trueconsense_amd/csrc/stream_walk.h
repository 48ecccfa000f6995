// stream_walk.h — DEVICE side (.hip files only) of the kernels that ask a kept record for its token at given columns of the count matrix's
// axis, in ascending order: strand_counts.hip (the planes per strand), link_counts.hip (the token classes of a record at two columns
// together), codon_counts.hip (at the three columns of a codon; class_of is theirs) and indel_events.hip (the insertion behind and the deletion that starts on a column: after token_at, w.k is the op that
// holds the column).  One copy of the per-record incremental CIGAR walk and of the count matrix's token rule restated for one column, so both
// kernels count exactly what tally_stream_kernel (tally.hip) counts.  Which record is kept and where it lies (kept_span), the primer
// table's lookup (seg_find) and the leaves of the rule (base_plane, qual_at): pack_device.h.
#pragma once
#include "pack_device.h"

namespace {

// a kept record between its queried columns
struct Walk {
    ReadView v;
    int32_t x, y;                       // the first column and the query index of op k
    uint32_t k;
    int32_t q;                          // the last column
    int32_t keep0, keep1;               // tokens on columns outside [keep0, keep1) are masked
};

// record i, when it is kept -> its walk at the head of the CIGAR
__device__ inline bool open_walk(const PackSrc &src, const tcmi_primer_tab &pt, int64_t i, Walk &w)
{
    int64_t p, q;
    if (!kept_span(src, i, w.v, p, q)) return false;
    if (p >= WALK_MAX_COL) return false;                    // (beyond every column that can be asked for)
    w.x = (int32_t)p; w.y = 0; w.k = 0;
    w.q = (int32_t)(q < WALK_MAX_COL ? q : WALK_MAX_COL);
    w.keep0 = INT32_MIN; w.keep1 = INT32_MAX;
    if (pt.n_head + pt.n_tail != 0) {
        w.keep0 = seg_find(pt.seg, pt.n_head, w.x, w.x);
        w.keep1 = seg_find(pt.seg + 3 * pt.n_head, pt.n_tail, w.q, w.q + 1);
    }
    if (pt.clip) w.keep0 = max(w.keep0, w.x + (int32_t)pt.clip[i]);        // (the mate join: the record's first clip columns are its mate's)
    return true;
}

// the planes the record's token on column c adds to (bit TCMI_COV..TCMI_I), c in [w.x, w.q] and not below an earlier call's
__device__ inline uint32_t token_at(Walk &w, int32_t c, uint32_t Q)
{
    const ReadView &v = w.v;
    uint32_t op = 0;
    int32_t len = 0;
    for (;; ++w.k) {                                        // on to the op that holds column c
        if (w.k >= v.n_cigar) return 0u;
        const uint32_t cw = ld_u32(v.cigar + 4 * (size_t)w.k);
        op = cw & 0xFu;
        len = (int32_t)(cw >> 4);
        if (consumes_ref(op)) {
            if (c - w.x < len) break;
            w.x += len;
        }
        if (consumes_query(op)) w.y += len;
    }
    if (c < w.keep0 || c >= w.keep1) return 0u;             // masked: nothing, the I mark included
    const int32_t j = c - w.x;
    const int32_t qi = is_match(op) ? w.y + j : w.y;       // a D / N token is tested with the query index at which its op starts
    if (Q != 0u && qual_at(v, qi) < Q) return 0u;          // below the floor (Q = 0: nothing is, and QUAL is not read)
    const bool ins = j == len - 1 && ins_after(v.cigar, v.n_cigar, w.k);
    uint32_t bits = 1u << TCMI_COV;                         // M, =, X, D and N all count coverage
    if (is_match(op)) {
        const uint32_t nib = qi < v.l_seq ? nib_at(v.seq, qi) : 15u;           // past SEQ -> 'N'
        if (__popc(nib) == 1) bits |= 1u << base_plane(nib);
    } else if (op == 2 && !ins) bits |= 1u << TCMI_X;       // "*+.." does not count X
    if (ins) bits |= 1u << TCMI_I;
    return bits;
}

// the planes a token adds to (token_at) -> its class: 0 nothing, 1..4 plane A, T, C, G, 5 a deleted column that counts X, 6 coverage only
// (link_counts.hip, codon_counts.hip)
__device__ inline uint32_t class_of(uint32_t bits)
{
    if (bits == 0u) return 0u;
    const uint32_t m = bits & ((1u << TCMI_A) | (1u << TCMI_T) | (1u << TCMI_C) | (1u << TCMI_G) | (1u << TCMI_X));
    return m ? (uint32_t)__builtin_ctz(m) : 6u;             // (TCMI_A..TCMI_X are 1..5; a token adds to at most one of them)
}

__device__ inline int32_t first_at_or_above(const int32_t *cols, int32_t n, int32_t p)
{
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (cols[mid] < p) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

} // namespace
