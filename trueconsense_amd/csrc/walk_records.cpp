// walk_records.cpp — HOST: call records of one BAM -> consensus: insert candidates -> modal tokens -> accepted inserts
// (Events.py:5-82), then the sequential walk of Sequences.BuildConsensus (Sequences.py:179-322, consensus_walk.cpp); and what both
// native runners share around it (walk_records.h).
#include "walk_records.h"

#include <cctype>

int tcmi_orfs_assign(tcmi_orfs *o, int32_t n_orf, const int64_t *start, const int64_t *end, const uint8_t *is_plus)
{
    if (!o || n_orf < 0 || (n_orf > 0 && (!start || !end || !is_plus))) return tcmi_fail(nullptr, TCMI_E_ARG, "bad argument");
    o->start.assign(start, start + n_orf);
    o->end.assign(end, end + n_orf);
    o->plus.assign(is_plus, is_plus + n_orf);
    return TCMI_OK;
}

void tcmi_insert_candidates(const uint8_t *flags, int64_t L, std::vector<int64_t> &cand)
{
    cand.clear();
    for (int64_t i = 0; i < L; ++i)
        if (flags[i] & TCMI_F_INSCAND) cand.push_back(i + 1);
}

int tcmi_host_reads::load(const char *path, int threads, const tcmi_read_filter &flt)
{
    int rc = tcmi_bam_load(path, threads, &bam);
    if (!rc) rc = tcmi_bam_filter(bam, (int32_t)flt.min_mapq, flt.require, flt.exclude, nullptr);
    if (!rc) tcmi_bam_reads(bam, &reads);
    return rc;
}

namespace {

// Events.py:75-80 on the modal token: re.search("(\d)([a-zA-Z]+)")
bool parse_token(const char *t, int64_t n, int *size_digit, const char **bases, int64_t *n_bases)
{
    for (int64_t i = 0; i + 1 < n; ++i)
        if (std::isdigit((unsigned char)t[i]) && std::isalpha((unsigned char)t[i + 1])) {
            int64_t j = i + 1;
            while (j < n && std::isalpha((unsigned char)t[j])) ++j;
            *size_digit = t[i] - '0';
            *bases = t + i + 1;
            *n_bases = j - i - 1;
            return true;
        }
    return false;
}

// insert candidates -> accepted inserts (positions, bases) and the digit of each one's token
int accept_inserts(const std::vector<int64_t> &cand, const tcmi_reads *reads, const tcmi_tokens *pre, long long item, tcmi_inserts &ins,
                   std::vector<int32_t> &shift)
{
    ins.off.assign(1, 0);
    if (cand.empty()) return TCMI_OK;
    tcmi_tokens own;
    if (!(pre && pre->valid)) {
        if (!reads)
            return tcmi_fail(nullptr, TCMI_E_UNSUPPORTED,
                             "item %lld has %zu insert candidates but no host reads were given to resolve their tokens", item, cand.size());
        int32_t tok_status = 0;
        // pysam's defaults for AlignmentFile.pileup() (Events.py:66 passes none): SURVEY §8-Q8
        const int rc = tcmi_tokens_grow(nullptr, cand.size(), own, [&](char *text, int64_t cap) {
            return tcmi_modal_tokens(reads, (int32_t)cand.size(), cand.data(), 13, 0x4 | 0x100 | 0x200 | 0x400, 1, 8000, 1, text, cap,
                                     own.off.data(), own.cnt.data(), &tok_status);
        });
        if (rc) return rc;
        if (tok_status & TCMI_TOKENS_OVERLAP_UNKNOWN)
            return tcmi_fail(nullptr, TCMI_E_UNSUPPORTED,
                             "item %lld: overlapping mates with a deletion on an insert-candidate column: pysam's overlap quality tweak there is not modelled", item);
        pre = &own;
    }
    for (size_t k = 0; k < cand.size(); ++k) {
        if (pre->cnt[k] == 0) continue;
        int digit;
        const char *b;
        int64_t nb;
        if (!parse_token(pre->toks.data() + pre->off[k], pre->off[k + 1] - pre->off[k], &digit, &b, &nb)) continue;
        ins.pos.push_back(cand[k]);
        shift.push_back(digit);
        ins.seq.append(b, (size_t)nb);
        ins.off.push_back((int64_t)ins.seq.size());
    }
    return TCMI_OK;
}

} // namespace

int tcmi_walk_records(const uint8_t *plain, const uint8_t *alt, const uint8_t *flags, int64_t L, const std::vector<int64_t> &cand,
                      const tcmi_reads *reads, const tcmi_tokens *pre, const tcmi_orfs &orfs, char *out, int64_t cap, int64_t *out_len,
                      long long item, tcmi_walk_extra *extra)
{
    tcmi_inserts own_ins;
    tcmi_inserts &ins = extra ? extra->ins : own_ins;
    std::vector<int32_t> shift;
    int rc = accept_inserts(cand, reads, pre, item, ins, shift);
    if (rc) return rc;
    const int32_t n_orf = (int32_t)orfs.size();
    std::vector<int64_t> ns((size_t)n_orf), ne((size_t)n_orf);
    int64_t err_pos = 0;
    auto walk = [&](int include_ins, char *dst, int64_t room, int64_t *len, int64_t *new_start, int64_t *new_end) {
        return tcmi_consensus_walk(plain, alt, flags, L, n_orf, orfs.start.data(), orfs.end.data(), orfs.plus.data(), (int32_t)ins.pos.size(),
                                   ins.pos.data(), shift.data(), ins.seq.c_str(), ins.off.data(), include_ins, dst, room, len, new_start,
                                   new_end, &err_pos);
    };
    rc = walk(1, out, cap, out_len, ns.data(), ne.data());
    if (rc || !extra) return rc;
    // the insert-free consensus the VCF is made from: a second walk (Outputs.py:98), whose ORF corrections are discarded
    extra->cons_noinsert.resize((size_t)L + 1);
    int64_t len2 = 0;
    std::vector<int64_t> ns2((size_t)n_orf), ne2((size_t)n_orf);
    rc = walk(0, &extra->cons_noinsert[0], (int64_t)extra->cons_noinsert.size(), &len2, ns2.data(), ne2.data());
    if (rc) return rc;
    extra->cons_noinsert.resize((size_t)len2);
    extra->new_start = ns; extra->new_end = ne;
    return TCMI_OK;
}
