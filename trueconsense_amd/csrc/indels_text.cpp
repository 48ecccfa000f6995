// indels_text.cpp — the host side of --indel-table behind the C ABI (include/tcmi.h: tcmi_indels_text, tcmi_indel_passes,
// tcmi_indel_hash; the rule: indel_rule.h) and the merge of event lists (tcmi_indel_merge: THE order, the sum over the parts of a read
// set of sub-ranges).  HOST only, re-entrant, no HIP header: the command line calls it through the C ABI and tests/indel_main.cpp links
// it into a program of its own.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "indel_rule.h"

extern "C" uint64_t tcmi_indel_hash(uint32_t seed, int32_t len, const uint8_t *nibbles, int32_t bits)
{
    uint64_t h = tcmi_indel_hash_begin(seed);
    for (int32_t i = 0; i < len; ++i) h = tcmi_indel_hash_step(h, nibbles ? nibbles[i] : 15u);
    return tcmi_indel_hash_end(h, len < 0 ? 0 : len, bits);
}

extern "C" int tcmi_indel_passes(int32_t count, int32_t cov, int64_t num, int64_t den, int32_t min_alt_depth, int32_t min_depth)
{
    const tcmi_var_rule r = {num, den, min_alt_depth, min_depth};
    if (!tcmi_indel_rule_ok(r) || count < 0 || cov < 0) return TCMI_E_ARG;
    return tcmi_indel_rule_passes(count, cov, r) ? 1 : 0;
}

namespace {

struct Ref {                            // an event of part p
    const tcmi_indel_event *e;
    const char *bases;                  // len letters (INS), nullptr (DEL)
};

// THE order: (pos, kind, len, bases)
int cmp(const Ref &a, const Ref &b)
{
    if (a.e->pos != b.e->pos) return a.e->pos < b.e->pos ? -1 : 1;
    if (a.e->kind != b.e->kind) return a.e->kind < b.e->kind ? -1 : 1;
    if (a.e->len != b.e->len) return a.e->len < b.e->len ? -1 : 1;
    if (!a.bases || !b.bases) return 0;
    const int c = std::memcmp(a.bases, b.bases, (size_t)a.e->len);
    return c < 0 ? -1 : c > 0 ? 1 : 0;
}

} // namespace

bool tcmi_indel_merge(const std::vector<tcmi_indel_list> &parts, const tcmi_var_rule *rule, tcmi_indel_list &out)
{
    std::vector<Ref> refs;
    for (const tcmi_indel_list &p : parts) {
        for (const tcmi_indel_event &e : p.ev) {
            const bool ins = e.kind == TCMI_INDEL_INS;
            if ((!ins && e.kind != TCMI_INDEL_DEL) || e.len < 0 || e.count < 0) return false;
            if (ins && (e.text_off < 0 || (uint64_t)e.text_off + (uint64_t)e.len > p.text.size())) return false;
            refs.push_back({&e, ins ? p.text.data() + e.text_off : nullptr});
        }
    }
    std::sort(refs.begin(), refs.end(), [](const Ref &a, const Ref &b) { return cmp(a, b) < 0; });
    out.ev.clear();
    out.text.clear();
    for (size_t i = 0; i < refs.size();) {
        size_t j = i + 1;
        int64_t count = refs[i].e->count;
        for (; j < refs.size() && cmp(refs[i], refs[j]) == 0; ++j) {
            if (refs[j].e->cov != refs[i].e->cov) return false;
            count += refs[j].e->count;
        }
        if (count > INT32_MAX) return false;
        tcmi_indel_event e = *refs[i].e;
        e.count = (int32_t)count;
        e.reserved = 0;
        if (!rule || tcmi_indel_rule_passes(e.count, e.cov, *rule)) {
            e.text_off = -1;
            if (refs[i].bases) {
                e.text_off = (int64_t)out.text.size();
                out.text.append(refs[i].bases, (size_t)e.len);
            }
            out.ev.push_back(e);
        }
        i = j;
    }
    return true;
}

namespace {

// text written into a buffer of `cap`, counted beyond it
struct Sink {
    char *text;
    int64_t cap, used;
    bool fits;
    void put(const char *p, size_t m)
    {
        if (fits && used + (int64_t)m <= cap) std::memcpy(text + used, p, m);
        else fits = false;
        used += (int64_t)m;
    }
};

} // namespace

extern "C" int tcmi_indels_text(const tcmi_indel_event *events, int64_t n, const char *text, int64_t text_len, const tcmi_indel_totals *totals, int64_t n_cols,
                                const tcmi_variant *records, int64_t n_records, const char *region, int64_t pos_offset, const uint8_t *ref, int64_t n_ref,
                                char *out, int64_t cap, int64_t *len)
{
    if (len) *len = 0;
    if (n < 0 || text_len < 0 || n_cols < 0 || n_records < 0 || cap < 0 || n_ref < 0 || pos_offset < 0 || !region || !len || (n > 0 && !events) ||
        (text_len > 0 && !text) || (n_cols > 0 && !totals) || (n_records > 0 && !records) || (n_ref > 0 && !ref) || (cap > 0 && !out))
        return TCMI_E_ARG;
    // the totals belong to the distinct positions of the '*' and '+' records, in order; cov_of[j]: the records' coverage there
    std::vector<int32_t> cov_of;
    try {
        cov_of.assign((size_t)n_cols, 0);
    } catch (...) {                                         // (no exception may cross the C ABI)
        return TCMI_E_NOMEM;
    }
    int64_t n_pos = 0;
    for (int64_t i = 0; i < n_records; ++i) {
        const tcmi_variant &v = records[i];
        if (v.pos < pos_offset || v.pos >= n_ref || v.allele < TCMI_A || v.allele > TCMI_I || v.cov <= 0 || v.count < 0) return TCMI_E_ARG;
        if (i && v.pos < records[i - 1].pos) return TCMI_E_ARG;
        if (v.allele != TCMI_X && v.allele != TCMI_I) continue;
        if (n_pos == 0 || totals[n_pos - 1].pos != v.pos) {
            if (n_pos >= n_cols || totals[n_pos].pos != v.pos) return TCMI_E_ARG;
            const tcmi_indel_totals &t = totals[n_pos];
            if (t.ins_total < 0 || t.del_total < 0 || t.del_total > v.cov) return TCMI_E_ARG;
            cov_of[(size_t)n_pos++] = v.cov;
        }
        const tcmi_indel_totals &t = totals[n_pos - 1];
        if (v.cov != cov_of[(size_t)n_pos - 1]) return TCMI_E_ARG;
        // THE invariant: the stream kernels and the matrix's kernels agree on the I plane
        if (v.allele == TCMI_I && t.ins_total != v.count) return TCMI_E_ARG;
    }
    if (n_pos != n_cols) return TCMI_E_ARG;                 // (totals of a position no record has)
    // the events: in THE order, each on a queried position, within its kind's total, its letters inside text
    int64_t jx = 0;
    for (int64_t i = 0; i < n; ++i) {
        const tcmi_indel_event &e = events[i];
        const bool ins = e.kind == TCMI_INDEL_INS;
        if ((!ins && e.kind != TCMI_INDEL_DEL) || e.len < 1 || e.count < 0) return TCMI_E_ARG;
        if (ins) {
            if (e.text_off < 0 || e.text_off > text_len || (int64_t)e.len > text_len - e.text_off) return TCMI_E_ARG;
            for (int32_t k = 0; k < e.len; ++k)
                if (!std::memchr("=ACMGRSVTWYHKDBN", text[e.text_off + k], 16)) return TCMI_E_ARG;
        }
        if (i) {
            const Ref a = {&events[i - 1], events[i - 1].kind == TCMI_INDEL_INS ? text + events[i - 1].text_off : nullptr}, b = {&e, ins ? text + e.text_off : nullptr};
            if (cmp(a, b) >= 0) return TCMI_E_ARG;
        }
        while (jx < n_cols && totals[jx].pos < e.pos) ++jx;
        if (jx >= n_cols || totals[jx].pos != e.pos) return TCMI_E_ARG;
        if (e.cov != cov_of[(size_t)jx] || e.count > (ins ? totals[jx].ins_total : totals[jx].del_total)) return TCMI_E_ARG;
    }
    const size_t n_region = std::strlen(region);
    Sink sink = {out, cap, 0, true};
    std::string seq;
    for (int64_t i = 0; i < n; ++i) {
        const tcmi_indel_event &e = events[i];
        const bool ins = e.kind == TCMI_INDEL_INS;
        char head[64], tail[64];    // (two numbers of at most 11 characters, a word, four separators; three numbers)
        const int m1 = std::snprintf(head, sizeof head, "\t%lld\t%s\t%d\t", (long long)(e.pos - pos_offset + 1), ins ? "INS" : "DEL", e.len);
        const int m2 = std::snprintf(tail, sizeof tail, "\t%d\t%d\t%.6f\n", e.count, e.cov, (double)e.count / (double)e.cov);
        if (m1 < 0 || m1 >= (int)sizeof head || m2 < 0 || m2 >= (int)sizeof tail) return TCMI_E_ARG;
        sink.put(region, n_region);
        sink.put(head, (size_t)m1);
        if (ins) sink.put(text + e.text_off, (size_t)e.len);
        else {
            // the deleted reference bases in pieces (a deletion may be as long as a CIGAR op: 2^28)
            char piece[256];
            for (int64_t p = e.pos, end = (int64_t)e.pos + e.len; p < end;) {
                size_t m = 0;
                for (; m < sizeof piece && p < end; ++m, ++p) {
                    const int u = p < n_ref ? ref[p] & ~0x20 : 'N';
                    piece[m] = (char)((u >= 'A' && u <= 'Z') ? u : 'N');
                }
                sink.put(piece, m);
            }
        }
        sink.put(tail, (size_t)m2);
    }
    *len = sink.used;
    return sink.fits || !out ? TCMI_OK : TCMI_E_ARG;        // (out == NULL with cap = 0 is the sizing call: *len, and no refusal)
}
