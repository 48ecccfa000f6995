// cigar_host.h — HOST: the CIGAR rules of the host packer (host_pack.cpp) and the host insert sweep (insert_tokens.cpp), over aligned
// CIGAR words (len << 4 | op).  Plain C++, no HIP header.  The kernels keep __device__ twins that read unaligned bytes (pack_device.h).
#pragma once
#include <cstdint>

#include "cigar_rule.h"
#include "indel_rule.h"

namespace tcmi_cigar {

// CIGAR operations (SAM spec §1.4: M 0, I 1, D 2, N 3, S 4, H 5, P 6, = 7, X 8)
inline bool consumes_ref(unsigned op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }
inline bool is_match(unsigned op) { return op == 0 || op == 7 || op == 8; }
inline bool consumes_query(unsigned op) { return op == 0 || op == 1 || op == 4 || op == 7 || op == 8; }

inline int64_t ref_span(const uint32_t *cg, int64_t n)
{
    int64_t s = 0;
    for (int64_t k = 0; k < n; ++k)
        if (consumes_ref(cg[k] & 0xF)) s += cg[k] >> 4;
    return s;
}

// p->indel of htslib's resolve_cigar2 at the last base of op k: > 0 an insertion of that many bases, < 0 a deletion
inline int64_t indel_after(const uint32_t *cg, int64_t n, int64_t k)
{
    if (k + 1 >= n) return 0;
    const unsigned op = cg[k] & 0xF, op2 = cg[k + 1] & 0xF;
    int64_t tot = 0;
    if (op2 == 2 && op != 2) {
        tot = -(int64_t)(cg[k + 1] >> 4);
        for (int64_t j = k + 2; j < n && (cg[j] & 0xF) == 2; ++j) tot -= cg[j] >> 4;
    } else if (op2 == 1) {
        tot = cg[k + 1] >> 4;
        for (int64_t j = k + 2; j < n; ++j) {
            const unsigned o = cg[j] & 0xF;
            if (o == 1) tot += cg[j] >> 4;
            else if (o != 6) break;
        }
    } else if (op2 == 6 && k + 2 < n) {
        for (int64_t j = k + 2; j < n; ++j) {
            const unsigned o = cg[j] & 0xF;
            if (o == 1) tot += cg[j] >> 4;
            else if (consumes_ref(o)) break;
        }
    }
    return tot;
}

// ... its peek at the last reference base of op k: is an insertion reported there?
inline bool ins_after(const uint32_t *cg, int64_t n, int64_t k) { return indel_after(cg, n, k) > 0; }

// the insertion ins_after reports behind op k, base by base: f(query index) for every base of exactly the I ops indel_after adds up, in
// CIGAR order (y: the query index behind op k) -> their number.  The host twin of the kernels' walk (indel_events.hip), over the one
// iterator of indel_rule.h.
template <class F> inline int64_t ins_bases(const uint32_t *cg, int64_t n, int64_t k, int64_t y, F f)
{
    tcmi_ins_iter it([cg](uint32_t j) { return cg[j]; }, (uint32_t)n, (uint32_t)k, y);
    int64_t len = 0;
    for (int64_t qi; (qi = it.next()) >= 0; ++len) f(qi);
    return len;
}

// [H]*[S]* (M|=|X)+ [S]*[H]*  ->  query offset of the first aligned base, aligned length (at most max_span)
inline bool aligned_shape(const uint32_t *cg, int64_t n, int64_t max_span, int64_t *y0, int64_t *len)
{
    int64_t k = 0, clip = 0, m = 0;
    while (k < n && (cg[k] & 0xF) == 5) ++k;
    while (k < n && (cg[k] & 0xF) == 4) { clip += cg[k] >> 4; ++k; }
    if (k == n || !is_match(cg[k] & 0xF)) return false;
    while (k < n && is_match(cg[k] & 0xF)) { m += cg[k] >> 4; ++k; }
    while (k < n && (cg[k] & 0xF) == 4) ++k;
    while (k < n && (cg[k] & 0xF) == 5) ++k;
    if (k != n || m <= 0 || m > max_span) return false;
    *y0 = clip;
    *len = m;
    return true;
}

} // namespace tcmi_cigar
