// codons_text.cpp — the host side of --codon-table behind the C ABI (include/tcmi.h: tcmi_codon_aa, tcmi_codon_select,
// tcmi_codons_text; the rule: codon_rule.h).  HOST only, re-entrant, no HIP header: the command line calls it through the C ABI and
// tests/codons_main.cpp links it into a program of its own.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "codon_rule.h"
#include "variants_rule.h"

extern "C" int tcmi_codon_aa(int b0, int b1, int b2) { return tcmi_codon_aa_rule(b0, b1, b2); }

extern "C" int tcmi_codon_select(const tcmi_variant *records, int64_t n, const tcmi_cds *cds, int64_t n_cds, int64_t *c0, int64_t cap, int64_t *n_found)
{
    if (n_found) *n_found = 0;
    if (n < 0 || n_cds < 0 || cap < 0 || !n_found || (n > 0 && !records) || (n_cds > 0 && !cds) || (cap > 0 && !c0)) return TCMI_E_ARG;
    for (int64_t f = 0; f < n_cds; ++f)
        if (!tcmi_cds_ok(cds[f])) return TCMI_E_ARG;
    std::vector<int64_t> found;
    try {
        for (int64_t i = 0; i < n; ++i) {
            const tcmi_variant &v = records[i];
            if (v.pos < 0 || v.allele < TCMI_A || v.allele > TCMI_I) return TCMI_E_ARG;
            if (v.allele > TCMI_X) continue;                // '+' rows do not select
            for (int64_t f = 0; f < n_cds; ++f) {
                const int64_t c = tcmi_cds_codon_of(cds[f], v.pos, nullptr);
                if (c >= 0) found.push_back(c);
            }
        }
        std::sort(found.begin(), found.end());
    } catch (...) {                                         // (no exception may cross the C ABI)
        return TCMI_E_NOMEM;
    }
    found.erase(std::unique(found.begin(), found.end()), found.end());
    *n_found = (int64_t)found.size();
    if (!c0 && cap == 0) return TCMI_OK;                    // the sizing call
    if (*n_found > cap) return TCMI_E_ARG;
    std::copy(found.begin(), found.end(), c0);
    return TCMI_OK;
}

namespace {

struct Triplet { int32_t count, code; };

} // namespace

extern "C" int tcmi_codons_text(const tcmi_codon_counts *counts, int64_t n, const tcmi_cds *cds, int64_t n_cds, const char *const *names,
                                const int32_t *matrix, int64_t L, int64_t ld, int64_t num, int64_t den, int32_t min_alt_depth, int32_t min_depth,
                                const char *region, int64_t pos_offset, const uint8_t *ref, int64_t n_ref, char *text, int64_t cap, int64_t *len)
{
    if (len) *len = 0;
    if (n < 0 || n_cds < 0 || cap < 0 || n_ref < 0 || pos_offset < 0 || L < 0 || ld < L || !region || !len || (n > 0 && !counts) ||
        (n_cds > 0 && (!cds || !names)) || (L > 0 && !matrix) || (n_ref > 0 && !ref) || (cap > 0 && !text) || den < 1 || den > 1000000 || num < 0 ||
        num > den || min_alt_depth < 1 || min_depth < 0)
        return TCMI_E_ARG;
    for (int64_t f = 0; f < n_cds; ++f)
        if (!tcmi_cds_ok(cds[f]) || !names[f]) return TCMI_E_ARG;
    // the counts are ascending, and add up to the count matrix at each of their three columns
    std::vector<tcmi_codon_sums> sums;
    try {
        sums.resize((size_t)n);
    } catch (...) {                                         // (no exception may cross the C ABI)
        return TCMI_E_NOMEM;
    }
    for (int64_t e = 0; e < n; ++e) {
        const tcmi_codon_counts &c = counts[e];
        if (c.pos < 0 || (e && c.pos <= counts[e - 1].pos) || !tcmi_codon_sum(c, sums[(size_t)e])) return TCMI_E_ARG;
        for (int k = 0; k < 3; ++k) {
            const int64_t col = (int64_t)c.pos + k;
            int64_t planes = 0;
            for (int x = TCMI_A; x <= TCMI_X; ++x) {
                const int64_t d = col < L ? matrix[x * ld + col] : 0;
                // the stream kernel and the matrix's kernels disagree: no table
                if (sums[(size_t)e].slot[k][x] != d) return TCMI_E_ARG;
                planes += d;
            }
            if (sums[(size_t)e].slot[k][6] != (col < L ? matrix[TCMI_COV * ld + col] : 0) - planes) return TCMI_E_ARG;
        }
    }
    static const char letter_of[6] = {'N', 'A', 'T', 'C', 'G', '-'};
    const size_t n_region = std::strlen(region);
    int64_t used = 0;
    bool fits = true;
    for (int64_t e = 0; e < n; ++e) {
        const tcmi_codon_counts &c = counts[e];
        const tcmi_codon_sums &s = sums[(size_t)e];
        int r[3];                                           // the reference's planes on the axis; 0: none of A, C, G, T, or beyond it
        for (int k = 0; k < 3; ++k) r[k] = (int64_t)c.pos + k < n_ref ? tcmi_var_ref_plane(ref[c.pos + k]) : 0;
        for (int64_t f = 0; f < n_cds; ++f) {
            int64_t number = 0;
            if (!tcmi_cds_has_codon(cds[f], c.pos, &number)) continue;
            const bool minus = cds[f].strand < 0;
            // axis order -> coding order
            const auto coding = [&](const int t[3], int out[3]) {
                for (int k = 0; k < 3; ++k) out[k] = minus ? (t[2 - k] == TCMI_X ? TCMI_X : tcmi_plane_complement(t[2 - k])) : t[k];
            };
            int rc[3];
            coding(r, rc);
            const int ref_aa = tcmi_codon_aa_rule(rc[0], rc[1], rc[2]);
            Triplet rows[4 * 4 * 4 + 1];
            int n_rows = 0;
            for (int code = 0; code < 343; ++code) {
                const int t0 = code / 49, t1 = code / 7 % 7, t2 = code % 7;
                if (!tcmi_codon_complete(t0, t1, t2) || (t0 == r[0] && t1 == r[1] && t2 == r[2])) continue;
                const int64_t count = c.j[t0][t1][t2];
                if (count >= min_alt_depth && count * den >= num * s.span && s.span >= min_depth) rows[n_rows++] = {(int32_t)count, code};
            }
            std::sort(rows, rows + n_rows, [](const Triplet &a, const Triplet &b) { return a.count != b.count ? a.count > b.count : a.code < b.code; });
            const size_t n_name = std::strlen(names[f]);
            for (int i = 0; i < n_rows; ++i) {
                const int t[3] = {rows[i].code / 49, rows[i].code / 7 % 7, rows[i].code % 7};
                int tc[3];
                coding(t, tc);
                const bool del = t[0] == TCMI_X;
                const int alt_aa = del ? '-' : tcmi_codon_aa_rule(tc[0], tc[1], tc[2]);
                int subs = 0;
                for (int k = 0; k < 3 && !del; ++k) subs += t[k] != r[k];
                const char *effect = del ? "DEL" : ref_aa == 'X' ? "UNKNOWN" : alt_aa == ref_aa ? "SYN" : alt_aa == '*' ? "STOP_GAINED" :
                                     ref_aa == '*' ? "STOP_LOST" : "MIS";
                char row[256];  // (everything behind the feature: eight numbers of at most 20 characters, eight letters, two words, sixteen separators)
                const int m = std::snprintf(row, sizeof row, "\t%c\t%lld\t%lld\t%c%c%c\t%c\t%c%c%c\t%c\t%s\t%d\t%lld\t%lld\t%.6f\t%lld\t%lld\t%lld\n",
                                            minus ? '-' : '+', (long long)number, (long long)(c.pos - pos_offset + 1), letter_of[rc[0]],
                                            letter_of[rc[1]], letter_of[rc[2]], (char)ref_aa, letter_of[tc[0]], letter_of[tc[1]], letter_of[tc[2]],
                                            (char)alt_aa, effect, subs, (long long)rows[i].count, (long long)s.span,
                                            (double)rows[i].count / (double)s.span, (long long)(s.total - s.span), (long long)(s.span - s.complete),
                                            (long long)c.ins_inside);
                if (m < 0 || m >= (int)sizeof row) return TCMI_E_ARG;
                const int64_t need = (int64_t)n_region + 1 + (int64_t)n_name + m;
                if (fits && used + need <= cap) {
                    char *at = text + used;
                    std::memcpy(at, region, n_region);
                    at[n_region] = '\t';
                    std::memcpy(at + n_region + 1, names[f], n_name);
                    std::memcpy(at + n_region + 1 + n_name, row, (size_t)m);
                } else fits = false;
                used += need;
            }
        }
    }
    *len = used;
    return fits || !text ? TCMI_OK : TCMI_E_ARG;            // (text == NULL with cap = 0 is the sizing call: *len, and no refusal)
}
