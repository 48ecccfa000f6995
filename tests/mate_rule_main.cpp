// mate_rule_main.cpp — csrc/mate_rule.h as a program of its own (tests/test_mate_rule.py builds it plain and under AddressSanitizer +
// UBSan): the rule of --mate-overlap on records given as text, without a GPU.
//   mate_rule_main IN OUT
//   mate_rule_main --names      tcmi_mate_same_name on every name length 1 .. 12 x every byte position, prints "names ok <compares>"
// IN:  one line per kept record: flag tid pos next_tid next_pos p q name-in-hex ("-" for an empty name)
// OUT: one line per record: eligible hash(hex) members pair loses clip — members: the eligible records of its key (itself included),
//      pair: its group is a pair, loses: it is the pair's loser, clip: its clip.  Then "ok <records>" on stdout.
// The grouping here is a std::map over the key; whether two keys are equal, the pair test, the loser and the clip are the header's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../trueconsense_amd/csrc/mate_rule.h"

struct Rec {
    tcmi_mate_fields f;
    long long p, q;
    std::string name;
    bool eligible;
    unsigned long long hash;
};

// a name as it lies in a record: its bytes, then `junk` where the NUL, the CIGAR and SEQ follow — a dword load at the name's last
// whole-dword boundary ends inside them
static std::vector<uint8_t> lying(const std::vector<uint8_t> &name, uint8_t junk)
{
    std::vector<uint8_t> v = name;
    for (int k = 0; k < 4; ++k) v.push_back((uint8_t)(junk + 17 * k));
    return v;
}
static bool same_name(const std::vector<uint8_t> &a, uint8_t junk_a, const std::vector<uint8_t> &b, uint8_t junk_b)
{
    const std::vector<uint8_t> la = lying(a, junk_a), lb = lying(b, junk_b);
    auto word = [](const std::vector<uint8_t> &v) { return [&v](uint32_t k) { uint32_t w; std::memcpy(&w, v.data() + k, 4); return w; }; };   // (little-endian hosts)
    return tcmi_mate_same_name((uint32_t)a.size(), (uint32_t)b.size(), word(la), word(lb));
}
// every length 1 .. 12, every byte position, three ways to differ there; equal names over different bytes behind them; a name and the
// same name one byte longer or shorter.  -> compares made, -1: a wrong answer (said on stderr)
static long check_names()
{
    long n_cmp = 0;
    for (size_t n = 1; n <= 12; ++n) {
        std::vector<uint8_t> a(n);
        for (size_t k = 0; k < n; ++k) a[k] = (uint8_t)(33 + (7 * k + 3 * n) % 94);
        for (uint8_t junk_b : {(uint8_t)0x00, (uint8_t)0x5A, (uint8_t)0xFF}) {
            ++n_cmp;
            if (!same_name(a, 0x5A, a, junk_b)) { std::fprintf(stderr, "equal names of %zu bytes compare different\n", n); return -1; }
            for (size_t p = 0; p < n; ++p)
                for (uint8_t flip : {(uint8_t)0x01, (uint8_t)0x80, (uint8_t)0xFF}) {
                    std::vector<uint8_t> b = a;
                    b[p] ^= flip;
                    n_cmp += 2;
                    if (same_name(a, 0x5A, b, junk_b) || same_name(b, junk_b, a, 0x5A)) {
                        std::fprintf(stderr, "names of %zu bytes that differ in byte %zu (^ %02x) compare equal\n", n, p, flip);
                        return -1;
                    }
                }
            // (the longer name continues with the very byte that lies behind the shorter one)
            std::vector<uint8_t> longer = a;
            longer.push_back(junk_b);
            n_cmp += 2;
            if (same_name(a, junk_b, longer, 0x5A) || same_name(longer, 0x5A, a, junk_b)) { std::fprintf(stderr, "names of %zu and %zu bytes compare equal\n", n, n + 1); return -1; }
        }
    }
    return n_cmp;
}

int main(int argc, char **argv)
{
    if (argc == 2 && std::string(argv[1]) == "--names") {
        const long n_cmp = check_names();
        if (n_cmp < 0) return 1;
        std::printf("names ok %ld\n", n_cmp);
        return 0;
    }
    if (argc != 3) { std::fprintf(stderr, "usage: mate_rule_main IN OUT\n"); return 2; }
    FILE *in = std::fopen(argv[1], "r");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<Rec> recs;
    char hex[1024];
    unsigned flag;
    int tid, pos, ntid, npos;
    long long p, q;
    while (std::fscanf(in, "%u %d %d %d %d %lld %lld %1023s", &flag, &tid, &pos, &ntid, &npos, &p, &q, hex) == 8) {
        Rec r;
        r.f.flag = flag; r.f.tid = tid; r.f.pos = pos; r.f.next_tid = ntid; r.f.next_pos = npos;
        r.p = p; r.q = q;
        const std::string h = hex;
        if (h != "-")
            for (size_t k = 0; k + 1 < h.size(); k += 2) r.name.push_back((char)std::strtol(h.substr(k, 2).c_str(), nullptr, 16));
        r.eligible = tcmi_mate_eligible(r.f);
        r.hash = tcmi_mate_hash(reinterpret_cast<const uint8_t *>(r.name.data()), (int)r.name.size(), r.f);
        // the word-wise form the kernels use gives the same hash
        uint64_t hw = TCMI_MATE_FNV_BASIS;
        size_t k = 0;
        auto word = [&](size_t at, size_t n) { uint32_t w = 0; for (size_t b = 0; b < n; ++b) w |= (uint32_t)(uint8_t)r.name[at + b] << (8 * b); return w; };
        for (; k + 4 <= r.name.size(); k += 4) hw = tcmi_mate_hash_word(hw, word(k, 4));
        if (k < r.name.size()) hw = tcmi_mate_hash_word(hw, word(k, r.name.size() - k) | 0xAB000000u, (int)(r.name.size() - k));   // (bytes behind the name do not count)
        if (tcmi_mate_hash_finish(hw, r.f) != r.hash) { std::fprintf(stderr, "word-wise hash differs on record %zu\n", recs.size()); return 1; }
        recs.push_back(r);
    }
    std::fclose(in);
    std::map<std::tuple<std::string, int, int, int>, std::vector<size_t>> groups;
    for (size_t i = 0; i < recs.size(); ++i)
        if (recs[i].eligible) groups[std::make_tuple(recs[i].name, recs[i].f.tid, tcmi_mate_lo(recs[i].f), tcmi_mate_hi(recs[i].f))].push_back(i);
    std::vector<int> members(recs.size(), 0), pair(recs.size(), 0), loses(recs.size(), 0);
    std::vector<unsigned> clip(recs.size(), 0u);
    for (const auto &g : groups) {
        const std::vector<size_t> &m = g.second;
        for (size_t i : m) {
            members[i] = (int)m.size();
            if (!tcmi_mate_same_ints(recs[i].f, recs[m[0]].f)) { std::fprintf(stderr, "same_ints disagrees with the key\n"); return 1; }
        }
        if (m.size() != 2) continue;
        const Rec &a = recs[m[0]], &b = recs[m[1]];
        if (tcmi_mate_pair(a.f, b.f) != tcmi_mate_pair(b.f, a.f)) { std::fprintf(stderr, "the pair test is not symmetric\n"); return 1; }
        if (!tcmi_mate_pair(a.f, b.f)) continue;
        if (tcmi_mate_loses(a.f, b.f) == tcmi_mate_loses(b.f, a.f)) { std::fprintf(stderr, "a pair without exactly one loser\n"); return 1; }
        const size_t lo = tcmi_mate_loses(a.f, b.f) ? m[0] : m[1], wi = lo == m[0] ? m[1] : m[0];
        pair[lo] = pair[wi] = 1;
        loses[lo] = 1;
        clip[lo] = tcmi_mate_clip(recs[lo].p, recs[lo].q, recs[wi].q);
    }
    FILE *out = std::fopen(argv[2], "w");
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    for (size_t i = 0; i < recs.size(); ++i)
        std::fprintf(out, "%d %016llx %d %d %d %u\n", recs[i].eligible ? 1 : 0, recs[i].hash, members[i], pair[i], loses[i], clip[i]);
    std::fclose(out);
    std::printf("ok %zu\n", recs.size());
    return 0;
}
