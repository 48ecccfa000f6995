// codon_rule.h — the host rule of --codon-table (include/tcmi.h: tcmi_cds, tcmi_codon_aa, tcmi_codon_select, tcmi_codons_text), GPU-free:
// it includes no HIP header and compiles with any C++ compiler, so the library's writer (codons_text.cpp) and host programs that
// check it (tests/codons_main.cpp) share it.  The reading frames of a CDS row, the standard genetic code over the count matrix's
// planes, and the sums of a codon's joint counts.  All arithmetic is integer.
#pragma once
#include <cstdint>

#include "../../include/tcmi.h"

static_assert(sizeof(tcmi_codon_counts) == 346 * 4, "tcmi_codon_counts is 346 int32");
static_assert(sizeof(tcmi_cds) == 16, "tcmi_cds is four int32");
static_assert(TCMI_A == 1 && TCMI_T == 2 && TCMI_C == 3 && TCMI_G == 4 && TCMI_X == 5, "the classes 1..5 are the planes A, T, C, G, X");

inline bool tcmi_cds_ok(const tcmi_cds &f)
{
    return f.start >= 0 && f.end >= f.start && (f.strand == 1 || f.strand == -1) && f.phase >= 0 && f.phase <= 2;
}

// The frame's codon that holds column p -> its first (lowest) column, or -1 when p lies in none (outside the row, in front of the
// phase, in the incomplete last triplet); *number (may be NULL): the codon's 1-based number in coding direction.
// + strand: the triplets from start + phase upward; - strand: from end - 1 - phase downward.
inline int64_t tcmi_cds_codon_of(const tcmi_cds &f, int64_t p, int64_t *number)
{
    int64_t m, c0;
    if (f.strand > 0) {
        const int64_t first = (int64_t)f.start + f.phase;
        if (p < first) return -1;
        m = (p - first) / 3;
        c0 = first + 3 * m;
        if (c0 + 3 > f.end) return -1;
    } else {
        const int64_t top = (int64_t)f.end - 1 - f.phase;
        if (p > top) return -1;
        m = (top - p) / 3;
        c0 = top - 3 * m - 2;
        if (c0 < f.start) return -1;
    }
    if (number) *number = m + 1;
    return c0;
}

// is c0 the first column of one of the frame's codons?  (*number as above)
inline bool tcmi_cds_has_codon(const tcmi_cds &f, int64_t c0, int64_t *number)
{
    return tcmi_cds_codon_of(f, c0, number) == c0;          // (a codon's lowest column lies in that codon and in no other)
}

// the plane of the complementary base (0 stays 0)
inline int tcmi_plane_complement(int p)
{
    return p == TCMI_A ? TCMI_T : p == TCMI_T ? TCMI_A : p == TCMI_C ? TCMI_G : p == TCMI_G ? TCMI_C : 0;
}

// The standard genetic code by the codon's first two bases, the third in plane order A, T, C, G.  Rows: the first base in plane order,
// within it the second.
inline int tcmi_codon_aa_rule(int b0, int b1, int b2)
{
    static const char *const box[16] = {
        /* AA */ "KNNK", /* AT */ "IIIM", /* AC */ "TTTT", /* AG */ "RSSR",
        /* TA */ "*YY*", /* TT */ "LFFL", /* TC */ "SSSS", /* TG */ "*CCW",
        /* CA */ "QHHQ", /* CT */ "LLLL", /* CC */ "PPPP", /* CG */ "RRRR",
        /* GA */ "EDDE", /* GT */ "VVVV", /* GC */ "AAAA", /* GG */ "GGGG"};
    if (b0 < TCMI_A || b0 > TCMI_G || b1 < TCMI_A || b1 > TCMI_G || b2 < TCMI_A || b2 > TCMI_G) return 'X';
    return box[(b0 - 1) * 4 + (b1 - 1)][b2 - 1];
}

// the sums of a codon's joint counts
struct tcmi_codon_sums {
    int64_t total;                      // every counted record
    int64_t span;                       // ... with a class >= 1 at all three columns
    int64_t complete;                   // ... with a complete triplet: three bases, or three deleted columns
    int64_t slot[3][7];                 // [k][x]: ... with class x at column c0 + k
};

inline bool tcmi_codon_complete(int t0, int t1, int t2)
{
    return (t0 >= 1 && t0 <= 4 && t1 >= 1 && t1 <= 4 && t2 >= 1 && t2 <= 4) || (t0 == 5 && t1 == 5 && t2 == 5);
}

// false: a negative counter, or j[0][0][0] != 0
inline bool tcmi_codon_sum(const tcmi_codon_counts &c, tcmi_codon_sums &s)
{
    s = tcmi_codon_sums();
    if (c.j[0][0][0] != 0 || c.ins_inside < 0) return false;
    for (int x = 0; x < 7; ++x)
        for (int y = 0; y < 7; ++y)
            for (int z = 0; z < 7; ++z) {
                const int64_t v = c.j[x][y][z];
                if (v < 0) return false;
                s.total += v;
                s.slot[0][x] += v; s.slot[1][y] += v; s.slot[2][z] += v;
                if (x && y && z) s.span += v;
                if (tcmi_codon_complete(x, y, z)) s.complete += v;
            }
    return true;
}
