// variants_rule.h — the rule of the variant table (--variant-table; include/tcmi.h, tcmi_variants_dev), GPU-free: which alleles of
// one position give a record.  One function, shared by the kernels (variants.hip) and by host programs that check them
// (tests/variants_main.cpp): it includes no HIP header and compiles with any C++ compiler.  All arithmetic is integer.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define TCMI_VAR_HD __attribute__((host)) __attribute__((device))
#else
#define TCMI_VAR_HD
#endif

// min_af = num / den (0 <= num <= den, 1 <= den <= 10^6), min_alt_depth >= 1, min_depth >= 0
struct tcmi_var_rule {
    int64_t num, den;
    int32_t min_alt_depth, min_depth;
};

// the matrix plane (TCMI_A..TCMI_G = 1..4) of a reference byte, 0 when it is not one of ACGTacgt (N, IUPAC codes, a guard's zero)
TCMI_VAR_HD inline int tcmi_var_ref_plane(int ref_byte)
{
    const int u = ref_byte & ~0x20;                 // ('a' and 'A' are the only bytes that give 'A')
    return u == 'A' ? 1 : u == 'T' ? 2 : u == 'C' ? 3 : u == 'G' ? 4 : 0;
}

// c[0..7): the position's counters in plane order (coverage, A, T, C, G, X, I); ref_byte: the reference on this position, or 0
// where it has none (p >= n_ref).  -> bit (a - 1) set for every plane a in 1..6 that gives a record: a is not the reference's
// plane, c[a] >= min_alt_depth and c[a] * den >= num * cov (an exact tie is in).  No record at all where the reference byte is
// not one of ACGTacgt or cov < max(min_depth, 1).  The products are below 2^31 * 10^6 < 2^51.
TCMI_VAR_HD inline unsigned tcmi_variant_mask(const int32_t c[7], int ref_byte, const tcmi_var_rule &r)
{
    const int rp = tcmi_var_ref_plane(ref_byte);
    const int64_t cov = c[0];
    if (rp == 0 || cov < (r.min_depth > 1 ? r.min_depth : 1)) return 0u;
    const int64_t bar = r.num * cov;
    unsigned m = 0;
    for (int a = 1; a <= 6; ++a)
        if (a != rp && c[a] >= r.min_alt_depth && (int64_t)c[a] * r.den >= bar) m |= 1u << (a - 1);
    return m;
}
