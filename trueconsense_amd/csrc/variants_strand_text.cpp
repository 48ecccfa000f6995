// variants_strand_text.cpp — the writer of --variant-strand's rows and the strand verdict behind the C ABI (include/tcmi.h:
// tcmi_variants_strand_text, tcmi_strand_verdict; the rule: strand_rule.h).  HOST only, re-entrant, no HIP header: the command line
// calls it through the C ABI and tests/strand_main.cpp links it into a program of its own.
#include <cstdio>
#include <cstring>

#include "strand_rule.h"

extern "C" int tcmi_strand_verdict(int32_t alt_fwd, int32_t alt_rev, int32_t tot_fwd, int32_t tot_rev, int32_t min_strand_depth, int64_t num, int64_t den)
{
    return tcmi_strand_rule(alt_fwd, alt_rev, tot_fwd, tot_rev, min_strand_depth, num, den);
}

extern "C" int tcmi_variants_strand_text(const tcmi_variant *records, int64_t n, const tcmi_strand_counts *strand, int64_t n_cols, int32_t min_strand_depth,
                                         int64_t num, int64_t den, const char *region, int64_t pos_offset, const uint8_t *ref, int64_t n_ref,
                                         char *text, int64_t cap, int64_t *len)
{
    if (len) *len = 0;
    if (n < 0 || cap < 0 || n_ref < 0 || pos_offset < 0 || n_cols < 0 || !region || !len || (n > 0 && (!records || !ref)) || (n_cols > 0 && !strand) ||
        (cap > 0 && !text) || !tcmi_strand_args_ok(min_strand_depth, num, den))
        return TCMI_E_ARG;
    static const char alt_of[TCMI_NCOL] = {0, 'A', 'T', 'C', 'G', '*', '+'};
    static const char *const word_of[3] = {"PASS", "BIAS", "LOW"};
    const size_t n_region = std::strlen(region);
    int64_t used = 0, j = -1;                       // j: the index of the current record's position among the distinct ones
    bool fits = true;
    for (int64_t i = 0; i < n; ++i) {
        const tcmi_variant &v = records[i];
        if (v.pos < pos_offset || v.pos >= n_ref || v.allele < TCMI_A || v.allele > TCMI_I || v.cov <= 0) return TCMI_E_ARG;
        if (i == 0 || v.pos != records[i - 1].pos) ++j;
        if (j >= n_cols || strand[j].pos != v.pos) return TCMI_E_ARG;
        const tcmi_strand_counts &s = strand[j];
        const int32_t af = s.fwd[v.allele], ar = s.rev[v.allele], tf = s.fwd[TCMI_COV], tr = s.rev[TCMI_COV];
        // the stream kernel and the matrix's kernels disagree: no table
        if ((int64_t)af + ar != v.count || (int64_t)tf + tr != v.cov) return TCMI_E_ARG;
        const char r = (char)(ref[v.pos] & ~0x20);
        const int rp = r == 'A' ? TCMI_A : r == 'T' ? TCMI_T : r == 'C' ? TCMI_C : r == 'G' ? TCMI_G : -1;
        const int verdict = tcmi_strand_rule(af, ar, tf, tr, min_strand_depth, num, den);
        if (verdict < 0) return TCMI_E_ARG;
        char row[192];              // (everything behind the region: nine numbers of at most 11 characters, a frequency, a word, thirteen separators)
        const int m = std::snprintf(row, sizeof row, "\t%lld\t%c\t%c\t%d\t%d\t%.6f\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n", (long long)(v.pos - pos_offset + 1), r,
                                    alt_of[v.allele], (int)v.count, (int)v.cov, (double)v.count / (double)v.cov, rp < 0 ? 0 : (int)s.fwd[rp],
                                    rp < 0 ? 0 : (int)s.rev[rp], (int)af, (int)ar, (int)tf, (int)tr, word_of[verdict]);
        if (m < 0 || m >= (int)sizeof row) return TCMI_E_ARG;
        const int64_t need = (int64_t)n_region + m;
        if (fits && used + need <= cap) {
            std::memcpy(text + used, region, n_region);
            std::memcpy(text + used + n_region, row, (size_t)m);
        } else fits = false;
        used += need;
    }
    if (j + 1 != n_cols) return TCMI_E_ARG;         // (counts of a position no record has)
    *len = used;
    return fits || !text ? TCMI_OK : TCMI_E_ARG;    // (text == NULL with cap = 0 is the sizing call: *len, and no refusal)
}
