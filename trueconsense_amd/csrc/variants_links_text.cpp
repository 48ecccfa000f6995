// variants_links_text.cpp — the writer of --variant-links' rows and the phase verdict behind the C ABI (include/tcmi.h:
// tcmi_variants_links_text, tcmi_link_phase; the rule: links_rule.h).  HOST only, re-entrant, no HIP header: the command line calls it
// through the C ABI and tests/links_main.cpp links it into a program of its own.
#include <cstdio>
#include <cstring>
#include <vector>

#include "links_rule.h"

extern "C" int tcmi_link_phase(int32_t both, int32_t only_a, int32_t only_b, int32_t span, int32_t min_depth, int64_t num, int64_t den)
{
    return tcmi_link_rule(both, only_a, only_b, span, min_depth, num, den);
}

namespace {

// do the joint counts of a pair with b >= 0 add up to the record of its first (side 0) or second (side 1) column?
bool adds_up(const tcmi_link_counts &l, int side, const tcmi_variant &v)
{
    int64_t cov = 0;
    for (int x = 1; x < 7; ++x) cov += side ? tcmi_link_col(l, x) : tcmi_link_row(l, x);
    if (cov != v.cov) return false;
    if (v.allele > TCMI_X) return true;                     // (the I mark is no class: only the coverage can be checked)
    return (side ? tcmi_link_col(l, v.allele) : tcmi_link_row(l, v.allele)) == v.count;
}

} // namespace

extern "C" int tcmi_variants_links_text(const tcmi_variant *records, int64_t n, const tcmi_link_counts *links, int64_t n_cols, int32_t k, int32_t min_depth,
                                        int64_t num, int64_t den, const char *region, int64_t pos_offset, const uint8_t *ref, int64_t n_ref,
                                        char *text, int64_t cap, int64_t *len)
{
    if (len) *len = 0;
    if (n < 0 || cap < 0 || n_ref < 0 || pos_offset < 0 || n_cols < 0 || n_cols > n || k < 1 || k > 7 || !region || !len ||
        (n > 0 && (!records || !ref)) || (n_cols > 0 && !links) || (cap > 0 && !text) || !tcmi_link_args_ok(min_depth, num, den))
        return TCMI_E_ARG;
    static const char alt_of[TCMI_NCOL] = {0, 'A', 'T', 'C', 'G', '*', '+'};
    static const char *const word_of[5] = {"CIS", "TRANS", "MIXED", "NONE", "LOW"};
    const size_t n_region = std::strlen(region);
    // the records fit; first[jx]: the first record of the jx-th distinct position
    std::vector<int64_t> first;
    try {
        first.assign((size_t)n_cols + 1, n);
    } catch (...) {                                         // (no exception may cross the C ABI)
        return TCMI_E_NOMEM;
    }
    int64_t n_pos = 0;
    for (int64_t i = 0; i < n; ++i) {
        const tcmi_variant &v = records[i];
        if (v.pos < pos_offset || v.pos >= n_ref || v.allele < TCMI_A || v.allele > TCMI_I || v.cov <= 0 || v.count < 0) return TCMI_E_ARG;
        if (i && v.pos < records[i - 1].pos) return TCMI_E_ARG;
        if (i == 0 || v.pos != records[i - 1].pos) {
            if (n_pos >= n_cols) return TCMI_E_ARG;
            first[(size_t)n_pos++] = i;
        }
    }
    if (n_pos != n_cols) return TCMI_E_ARG;                 // (counts of a position no record has)
    const auto pos_of = [&](int64_t jx) { return records[first[(size_t)jx]].pos; };
    // the links belong to the distinct positions in order, and their sums are the records' depths
    for (int64_t jx = 0; jx < n_cols; ++jx) {
        for (int d = 1; d <= k; ++d) {
            const tcmi_link_counts &l = links[jx * k + d - 1];
            if (l.a != pos_of(jx)) return TCMI_E_ARG;
            const bool inside = jx + d < n_cols;
            // behind the last position: no pair, or a column beyond it (the next region's)
            if (inside ? l.b != pos_of(jx + d) : (l.b != -1 && l.b <= pos_of(n_cols - 1))) return TCMI_E_ARG;
            for (int x = 0; x < 7; ++x)
                for (int y = 0; y < 7; ++y)
                    if (l.j[x][y] < 0) return TCMI_E_ARG;
            if (l.b < 0) continue;
            // the stream kernel and the matrix's kernels disagree: no table
            for (int64_t i = first[(size_t)jx]; i < first[(size_t)jx + 1]; ++i)
                if (!adds_up(l, 0, records[i])) return TCMI_E_ARG;
            if (!inside) continue;
            for (int64_t i = first[(size_t)(jx + d)]; i < first[(size_t)(jx + d) + 1]; ++i)
                if (!adds_up(l, 1, records[i])) return TCMI_E_ARG;
        }
    }
    int64_t used = 0;
    bool fits = true;
    for (int64_t jx = 0; jx < n_cols; ++jx) {
        for (int64_t i1 = first[(size_t)jx]; i1 < first[(size_t)jx + 1]; ++i1) {
            const tcmi_variant &va = records[i1];
            if (va.allele > TCMI_X) continue;               // '+' rows are not linked
            for (int d = 1; d <= k && jx + d < n_cols; ++d) {
                const tcmi_link_counts &l = links[jx * k + d - 1];
                for (int64_t i2 = first[(size_t)(jx + d)]; i2 < first[(size_t)(jx + d) + 1]; ++i2) {
                    const tcmi_variant &vb = records[i2];
                    if (vb.allele > TCMI_X) continue;
                    const int A = va.allele, B = vb.allele;
                    int64_t span = 0, only_a = 0, only_b = 0;
                    for (int x = 1; x < 7; ++x)
                        for (int y = 1; y < 7; ++y) span += l.j[x][y];
                    for (int y = 1; y < 7; ++y)
                        if (y != B) only_a += l.j[A][y];
                    for (int x = 1; x < 7; ++x)
                        if (x != A) only_b += l.j[x][B];
                    const int64_t both = l.j[A][B];
                    // (span is at most a record's cov, checked above: everything fits int32)
                    const int phase = tcmi_link_rule((int32_t)both, (int32_t)only_a, (int32_t)only_b, (int32_t)span, min_depth, num, den);
                    if (phase < 0) return TCMI_E_ARG;
                    char row[192];  // (everything behind the region: seven numbers of at most 11 characters, four letters, a word, twelve separators)
                    const int m = std::snprintf(row, sizeof row, "\t%lld\t%c\t%c\t%lld\t%c\t%c\t%lld\t%lld\t%lld\t%lld\t%lld\t%s\n",
                                                (long long)(va.pos - pos_offset + 1), (char)(ref[va.pos] & ~0x20), alt_of[A],
                                                (long long)(vb.pos - pos_offset + 1), (char)(ref[vb.pos] & ~0x20), alt_of[B], (long long)span,
                                                (long long)both, (long long)only_a, (long long)only_b, (long long)(span - both - only_a - only_b),
                                                word_of[phase]);
                    if (m < 0 || m >= (int)sizeof row) return TCMI_E_ARG;
                    const int64_t need = (int64_t)n_region + m;
                    if (fits && used + need <= cap) {
                        std::memcpy(text + used, region, n_region);
                        std::memcpy(text + used + n_region, row, (size_t)m);
                    } else fits = false;
                    used += need;
                }
            }
        }
    }
    *len = used;
    return fits || !text ? TCMI_OK : TCMI_E_ARG;            // (text == NULL with cap = 0 is the sizing call: *len, and no refusal)
}
