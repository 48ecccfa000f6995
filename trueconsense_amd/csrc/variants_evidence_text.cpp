// variants_evidence_text.cpp — the writer of --variant-evidence's rows and the evidence verdict behind the C ABI (include/tcmi.h:
// tcmi_variants_evidence_text, tcmi_evidence_verdict; the rule: evidence_rule.h).  HOST only, re-entrant, no HIP header: the command
// line calls it through the C ABI and tests/evidence_main.cpp links it into a program of its own.
#include <cstdio>
#include <cstring>

#include "evidence_rule.h"

extern "C" int tcmi_evidence_verdict(int64_t n, int64_t qual, int64_t mapq, int64_t dist, int32_t min_qual, int32_t min_mapq, int32_t min_dist)
{
    return tcmi_evidence_rule(n, qual, mapq, dist, min_qual, min_mapq, min_dist);
}

namespace {

// sum / n cut to one decimal: the tenths (0 when n = 0)
inline long long tenths(int64_t sum, int64_t n) { return n > 0 ? (long long)(((__int128)10 * sum) / n) : 0; }

} // namespace

extern "C" int tcmi_variants_evidence_text(const tcmi_variant *records, int64_t n, const tcmi_evidence_counts *ev, int64_t n_cols, int32_t min_qual,
                                           int32_t min_mapq, int32_t min_dist, const char *region, int64_t pos_offset, const uint8_t *ref, int64_t n_ref,
                                           char *text, int64_t cap, int64_t *len)
{
    if (len) *len = 0;
    if (n < 0 || cap < 0 || n_ref < 0 || pos_offset < 0 || n_cols < 0 || !region || !len || (n > 0 && (!records || !ref)) || (n_cols > 0 && !ev) ||
        (cap > 0 && !text) || !tcmi_evidence_args_ok(min_qual, min_mapq, min_dist))
        return TCMI_E_ARG;
    static const char alt_of[TCMI_NCOL] = {0, 'A', 'T', 'C', 'G', '*', '+'};
    static const char *const word_of[8] = {"PASS", "LOWQ", "LOWMQ", "LOWQ,LOWMQ", "END", "LOWQ,END", "LOWMQ,END", "LOWQ,LOWMQ,END"};
    const size_t n_region = std::strlen(region);
    // pass 0 checks every record against its counts and sizes the text; pass 1 writes: a refusal leaves the buffer as it was
    int64_t used = 0;
    for (int pass = 0; pass < 2; ++pass) {
        int64_t j = -1;                             // the index of the current record's position among the distinct ones
        used = 0;
        for (int64_t i = 0; i < n; ++i) {
            const tcmi_variant &v = records[i];
            if (i == 0 || v.pos != records[i - 1].pos) ++j;
            if (pass == 0) {
                if (v.pos < pos_offset || v.pos >= n_ref || v.allele < TCMI_A || v.allele > TCMI_I || v.cov <= 0) return TCMI_E_ARG;
                if (j >= n_cols || ev[j].pos != v.pos) return TCMI_E_ARG;
                for (int k = 0; k < TCMI_NCOL; ++k) {           // (a token adds at most 255 to a sum)
                    const int64_t top = 255 * (int64_t)ev[j].n[k];
                    if (ev[j].n[k] < 0 || ev[j].qual[k] < 0 || ev[j].mapq[k] < 0 || ev[j].dist[k] < 0 || ev[j].qual[k] > top || ev[j].mapq[k] > top ||
                        ev[j].dist[k] > top)
                        return TCMI_E_ARG;
                }
                // the stream kernel and the matrix's kernels disagree: no table
                if (ev[j].n[v.allele] != v.count || ev[j].n[TCMI_COV] != v.cov) return TCMI_E_ARG;
            }
            const tcmi_evidence_counts &e = ev[j];
            const char r = (char)(ref[v.pos] & ~0x20);
            const int rp = r == 'A' ? TCMI_A : r == 'T' ? TCMI_T : r == 'C' ? TCMI_C : r == 'G' ? TCMI_G : -1;
            const int al = v.allele;
            const int verdict = tcmi_evidence_rule(e.n[al], e.qual[al], e.mapq[al], e.dist[al], min_qual, min_mapq, min_dist);
            if (verdict < 0) return TCMI_E_ARG;
            const long long rq = rp < 0 ? 0 : tenths(e.qual[rp], e.n[rp]), rm = rp < 0 ? 0 : tenths(e.mapq[rp], e.n[rp]),
                            rd = rp < 0 ? 0 : tenths(e.dist[rp], e.n[rp]);
            const long long aq = tenths(e.qual[al], e.n[al]), am = tenths(e.mapq[al], e.n[al]), ad = tenths(e.dist[al], e.n[al]);
            char row[256];              // (everything behind the region: three numbers of at most 11 characters, a frequency, six means of at most 22, a word of at most 14)
            const int m = std::snprintf(row, sizeof row, "\t%lld\t%c\t%c\t%d\t%d\t%.6f\t%lld.%lld\t%lld.%lld\t%lld.%lld\t%lld.%lld\t%lld.%lld\t%lld.%lld\t%s\n",
                                        (long long)(v.pos - pos_offset + 1), r, alt_of[al], (int)v.count, (int)v.cov, (double)v.count / (double)v.cov,
                                        rq / 10, rq % 10, aq / 10, aq % 10, rm / 10, rm % 10, am / 10, am % 10, rd / 10, rd % 10, ad / 10, ad % 10,
                                        word_of[verdict]);
            if (m < 0 || m >= (int)sizeof row) return TCMI_E_ARG;
            if (pass == 1) {
                std::memcpy(text + used, region, n_region);
                std::memcpy(text + used + n_region, row, (size_t)m);
            }
            used += (int64_t)n_region + m;
        }
        if (pass == 0 && j + 1 != n_cols) return TCMI_E_ARG;    // (counts of a position no record has)
        if (pass == 0 && (!text || used > cap)) break;          // the sizing call, or a short buffer: *len, nothing written
    }
    *len = used;
    return !text || used <= cap ? TCMI_OK : TCMI_E_ARG;         // (text == NULL with cap = 0 is the sizing call: *len, and no refusal)
}
