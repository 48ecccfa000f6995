// amplicon_reads_rule.h — the rule of --amplicon-reads (include/tcmi.h, tcmi_readset_amplicon_reads), GPU-free: the compiled table and
// the lookup that says which amplicon of a scheme CONTAINS a read's columns [p, q].  The one copy that the kernel
// (amplicon_reads.hip), the library's host code (amplicon_reads_table.cpp) and host programs that check them
// (tests/amplicon_reads_main.cpp) share: it includes no HIP header and compiles with any C++ compiler.  All arithmetic is integer.
//
// Amplicon i is (fs, le, rs, fe) on the count matrix's axis: fs the smallest LEFT start, le the largest LEFT end, rs the smallest RIGHT
// start, fe the largest RIGHT end; with slack s its widened extent is [a, b) = [fs - s, fe + s).  A read is contained in i iff
// a <= p and q < b.  Contained in exactly one: that amplicon's read — and a FULL-LENGTH one iff also p < le and q >= rs —; in two or
// more: ambiguous; in none: unassigned.
//
// The table, int32 [6 * n], six dense arrays one behind the other:
//   a[k]     the widened starts, ascending (ties in the order given)                        k-th in sorted order
//   bmax[k]  the largest b among the first k + 1 sorted amplicons
//   idx[k]   the index, in the order GIVEN, of the first of them that has it
//   b2[k]    the second largest b among them, counted with multiplicity (two equal b are two); TCMI_AR_NONE for k = 0
//   le[i], rs[i]   of amplicon i in the order GIVEN
// Lookup (p, q): k = the number of a <= p (binary search).  The amplicons with a <= p are the first k; those of them that contain the
// read have b > q.  None iff k == 0 or bmax[k - 1] <= q; two or more iff b2[k - 1] > q; else exactly one, and it is the one with the
// largest b: idx[k - 1].  Exact for arbitrary interval sets — overlapping, nested, identical — in O(log n).
#pragma once
#include <stdint.h>

#include "../../include/tcmi.h"

#if defined(__HIP__)
#define TCMI_AR_HD __attribute__((host)) __attribute__((device))
#else
#define TCMI_AR_HD
#endif

static_assert(sizeof(tcmi_amplicon_reads) == 16, "tcmi_amplicon_reads is two int64");

constexpr int32_t TCMI_AR_MAX_N = 65536;                    // amplicons of one call
constexpr int64_t TCMI_AR_MAX_POS = (int64_t)1 << 29;       // a coordinate lies in [0, 2^29]
constexpr int32_t TCMI_AR_MAX_SLACK = 1000;
constexpr int32_t TCMI_AR_NONE = INT32_MIN;                 // "no second amplicon": below every q
constexpr int32_t TCMI_AR_WORDS = 6;                        // table words per amplicon
// the lookup's verdicts that are not an amplicon's index
constexpr int32_t TCMI_AR_UNASSIGNED = -1, TCMI_AR_AMBIGUOUS = -2;

// the checks of every entry point that takes a scheme.  -> 0: fine; 1: n outside 1..65536; 2: slack outside 0..1000; 3: a null array;
// 4: amplicon *bad has a coordinate outside [0, 2^29]; 5: amplicon *bad does not satisfy fs < le, rs < fe, fs < fe
inline int tcmi_amplicon_reads_check(int64_t n, const int64_t *fs, const int64_t *le, const int64_t *rs, const int64_t *fe, int32_t slack, int64_t *bad)
{
    if (bad) *bad = -1;
    if (n < 1 || n > TCMI_AR_MAX_N) return 1;
    if (slack < 0 || slack > TCMI_AR_MAX_SLACK) return 2;
    if (!fs || !le || !rs || !fe) return 3;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t v[4] = {fs[i], le[i], rs[i], fe[i]};
        for (int64_t x : v)
            if (x < 0 || x > TCMI_AR_MAX_POS) {
                if (bad) *bad = i;
                return 4;
            }
        if (!(fs[i] < le[i] && rs[i] < fe[i] && fs[i] < fe[i])) {
            if (bad) *bad = i;
            return 5;
        }
    }
    return 0;
}

// the table over its six arrays (t: int32 [6 * n], wherever it lies: device memory, LDS, the host)
struct tcmi_ar_table {
    const int32_t *a, *bmax, *idx, *b2, *le, *rs;
    int32_t n;
};
TCMI_AR_HD inline tcmi_ar_table tcmi_ar_view(const int32_t *t, int32_t n)
{
    return tcmi_ar_table{t, t + n, t + 2 * (int64_t)n, t + 3 * (int64_t)n, t + 4 * (int64_t)n, t + 5 * (int64_t)n, n};
}

// (p, q), q >= p: the first and last column of a kept read -> the index of the one amplicon that contains it (*full: does it start in
// the left primer zone and end in the right one), TCMI_AR_AMBIGUOUS or TCMI_AR_UNASSIGNED (*full false)
TCMI_AR_HD inline int32_t tcmi_ar_lookup(const tcmi_ar_table &t, int32_t p, int32_t q, bool *full)
{
    *full = false;
    int32_t lo = 0, hi = t.n;                               // a[lo - 1] <= p < a[hi]
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (t.a[mid] <= p) lo = mid + 1;
        else hi = mid;
    }
    if (lo == 0 || t.bmax[lo - 1] <= q) return TCMI_AR_UNASSIGNED;
    if (lo >= 2 && t.b2[lo - 1] > q) return TCMI_AR_AMBIGUOUS;
    const int32_t i = t.idx[lo - 1];
    *full = p < t.le[i] && q >= t.rs[i];
    return i;
}

// HOST (amplicon_reads_table.cpp): checks the scheme and compiles it into table[6 * n].  -> 0, or -1 with the reason in msg (may be null)
int tcmi_amplicon_reads_build(int64_t n, const int64_t *fs, const int64_t *le, const int64_t *rs, const int64_t *fe, int32_t slack, int32_t *table,
                              char *msg, size_t msg_cap);
