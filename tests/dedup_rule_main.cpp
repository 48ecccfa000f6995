// dedup_rule_main.cpp — csrc/dedup_rule.h as a program of its own (tests/test_dedup_rule.py builds it plain and under AddressSanitizer +
// UBSan): the rule of --dedup on records given as text, without a GPU.
//   dedup_rule_main IN OUT
// IN:  "N M", then N lines, one per record of the file: kept flag tid pos mate n_cigar word... qual-in-hex ("-": l_seq == 0) — kept:
//      the device packer keeps the record; mate: the record index + 1 of its mate when the mate join made a pair of them, else 0;
//      the CIGAR words as BAM stores them (len << 4 | op).  Then M lines "a b": the leaders of two templates.
// OUT: one line per record: examined u5 rev score key hash — key: the twelve key bytes in hex and hash: its FNV-1a, for a template's
//      leader, "-" for every other record.  Then one line per "a b": 1 when template a is the better of the two, else 0.  "ok N" on stdout.
// Ends, scores, keys, the hash and the order of two templates are the header's; who leads what is decided here as the kernels do.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../trueconsense_amd/csrc/dedup_rule.h"

struct Rec {
    int kept;
    unsigned flag;
    int tid, pos;
    unsigned mate;
    std::vector<uint32_t> cigar;
    std::vector<uint8_t> qual;
    bool examined = false;
    tcmi_dup_end end = {0, 0u, 0u, 0u};
};

static int fail(const char *what, size_t i)
{
    std::fprintf(stderr, "%s on record %zu\n", what, i);
    return 1;
}

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: dedup_rule_main IN OUT\n"); return 2; }
    FILE *in = std::fopen(argv[1], "r");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    size_t n = 0, m = 0;
    if (std::fscanf(in, "%zu %zu", &n, &m) != 2) return 2;
    std::vector<Rec> recs(n);
    std::vector<char> hex(1 << 20);
    for (size_t i = 0; i < n; ++i) {
        Rec &r = recs[i];
        unsigned n_cigar = 0;
        if (std::fscanf(in, "%d %u %d %d %u %u", &r.kept, &r.flag, &r.tid, &r.pos, &r.mate, &n_cigar) != 6) return fail("short line", i);
        r.cigar.resize(n_cigar);
        for (uint32_t &c : r.cigar)
            if (std::fscanf(in, "%u", &c) != 1) return fail("short CIGAR", i);
        if (std::fscanf(in, "%1048575s", hex.data()) != 1) return fail("no QUAL", i);
        const std::string h = hex.data();
        if (h != "-")
            for (size_t k = 0; k + 1 < h.size(); k += 2) r.qual.push_back((uint8_t)std::strtol(h.substr(k, 2).c_str(), nullptr, 16));
        r.examined = r.kept && tcmi_dup_examined(r.flag);
        if (!r.examined) continue;
        const bool rev = (r.flag & 0x10u) != 0u;
        const std::vector<uint32_t> &cg = r.cigar;
        const int64_t u5 = tcmi_dup_u5(r.pos, rev, n_cigar, [&cg](uint32_t k) { return cg[k]; });
        const uint32_t score = tcmi_dup_score(r.qual.data(), (int64_t)r.qual.size());
        // the word-wise form the kernels use gives the same score: whole words, then the tail as the last four bytes shifted down
        uint32_t sw = 0;
        size_t k = 0;
        auto word = [&](size_t at, size_t nb) { uint32_t w = 0; for (size_t b = 0; b < nb; ++b) w |= (uint32_t)r.qual[at + b] << (8 * b); return w; };
        for (; k + 4 <= r.qual.size(); k += 4) sw = tcmi_dup_score_add(sw, tcmi_dup_score_word(word(k, 4)));
        const size_t rest = r.qual.size() - k;
        if (rest && r.qual.size() >= 4) sw = tcmi_dup_score_add(sw, tcmi_dup_score_word(word(r.qual.size() - 4, 4) >> (8 * (4 - rest)), (int)rest));
        else if (rest) sw = tcmi_dup_score_add(sw, tcmi_dup_score_word(word(k, rest) | 0x29000000u, (int)rest));    // (bytes behind QUAL do not count)
        if (sw != score) return fail("word-wise score differs", i);
        r.end = tcmi_dup_end_make(r.tid, u5, rev, score, 1u);
        if (!tcmi_dup_end_examined(r.end) || tcmi_dup_end_rev(r.end) != (rev ? 1u : 0u) || (int)tcmi_dup_end_tid(r.end) != r.tid || r.end.u5 != u5)
            return fail("ends[] does not give back what went in", i);
    }
    // the template a record leads: its key and its score; false: it leads none
    auto leads = [&](size_t i, tcmi_dup_key &key, uint32_t &score) {
        const Rec &r = recs[i];
        if (!r.examined || (r.mate && (size_t)r.mate - 1 < i)) return false;
        if (!r.mate) { key = tcmi_dup_key_fragment(r.end); score = r.end.score; return true; }
        const Rec &o = recs[r.mate - 1];
        key = tcmi_dup_key_pair(r.end, o.end);
        const tcmi_dup_key other = tcmi_dup_key_pair(o.end, r.end);
        if (!tcmi_dup_key_same(key, other)) { std::fprintf(stderr, "the pair key depends on the order of its ends\n"); std::exit(1); }
        score = tcmi_dup_score_add(r.end.score, o.end.score);
        return true;
    };
    FILE *out = std::fopen(argv[2], "w");
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    for (size_t i = 0; i < n; ++i) {
        const Rec &r = recs[i];
        tcmi_dup_key key;
        uint32_t score = 0;
        std::fprintf(out, "%d %d %u %u ", r.examined ? 1 : 0, r.end.u5, tcmi_dup_end_rev(r.end), r.end.score);
        if (leads(i, key, score)) {
            for (int w = 0; w < 3; ++w)
                for (int b = 0; b < 4; ++b) std::fprintf(out, "%02x", (key.w[w] >> (8 * b)) & 0xFFu);
            std::fprintf(out, " %016llx\n", (unsigned long long)tcmi_dup_hash(key));
        } else std::fprintf(out, "- -\n");
    }
    for (size_t j = 0; j < m; ++j) {
        size_t a = 0, b = 0;
        if (std::fscanf(in, "%zu %zu", &a, &b) != 2 || a >= n || b >= n) return fail("bad template pair", j);
        tcmi_dup_key ka, kb;
        uint32_t sa = 0, sb = 0;
        if (!leads(a, ka, sa) || !leads(b, kb, sb)) return fail("not a leader in template pair", j);
        const bool better = tcmi_dup_better(sa, (uint32_t)a, sb, (uint32_t)b);
        if (a != b && better == tcmi_dup_better(sb, (uint32_t)b, sa, (uint32_t)a)) return fail("two templates without exactly one better", j);
        if (tcmi_dup_rank_leader(tcmi_dup_rank(sa, (uint32_t)a)) != (uint32_t)a) return fail("the rank does not give back its leader", j);
        std::fprintf(out, "%d\n", better ? 1 : 0);
    }
    std::fclose(in);
    std::fclose(out);
    std::printf("ok %zu\n", n);
    return 0;
}
