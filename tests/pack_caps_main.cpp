// pack_caps_main.cpp — csrc/pack_caps.h as a program of its own (tests/test_pack_caps.py builds it plain and under AddressSanitizer +
// UBSan): the device packer's decline flags, the one-sync packer's capacities and both packers' arena scratch, without a GPU.
//   pack_caps_main flags                                         one line "NAME value" per PKF_* flag
//   pack_caps_main caps INFLATED HINT SAFE LEN_BOUND SLOTS BALANCE
//                                                                "rec_cap word_cap chunk_cap event_cap n_wg" of pk_one_sync_caps
//   pack_caps_main fits REC WORD CHUNK EVENT  N_REC N_WORDS N_CHUNKS N_EVENTS
//                                                                the flags of pk_beyond_caps for totals against capacities
//   pack_caps_main pin N_BLOCKS                                  "alg end stat mate bytes" of ReportPin
//   pack_caps_main rest N_REC N_BLOCKS MATE PREFIX_OPTION        "several one_sync": what each packer's list sums to from an empty arena
//   pack_caps_main scratch START                                 both lists over a grid of settings, the summing pass against the taking
//                                                                pass on a counting stand-in for the arena that already holds START bytes:
//                                                                one line "packer settings.. : summed taken" each, then "ok <lines>"
// The stand-in hands out addresses and counts; nothing is ever stored there.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../trueconsense_amd/csrc/pack_caps.h"

namespace {

struct CountingArena {              // api.cpp's tcmi_arena_take, restated: a piece starts on 256 bytes
    size_t used;
    void *take(size_t bytes)
    {
        const size_t at = (used + 255) / 256 * 256;
        used = at + bytes;
        return reinterpret_cast<void *>(at + 4096);         // (never null, never followed)
    }
};

// arrays [from, to) of a list: summed, then taken; the pieces must be there exactly where bytes were asked for, aligned, in order, apart
template <int N> bool pass(PkScratch<N> &s, CountingArena &a, int from, int to, size_t *summed)
{
    *summed = s.end(*summed, from, to);
    size_t floor = a.used;
    s.take([&a](size_t b) { return a.take(b); }, from, to);
    for (int i = from; i < to; ++i) {
        if ((s.p[i] != nullptr) != (s.bytes[i] != 0)) return false;
        if (!s.p[i]) continue;
        const size_t at = reinterpret_cast<size_t>(s.p[i]) - 4096;
        if (at % 256 || at < floor) return false;
        floor = at + s.bytes[i];
    }
    return floor == a.used || from == to || a.used == *summed;
}

long long num(const char *s) { return std::strtoll(s, nullptr, 0); }

int scratch_grid(size_t start)
{
    const long long records[] = {0, 1, 255, 256, 257, 65537}, blocks[] = {1, 16383, 16384};
    int lines = 0;
    for (long long n : records)
        for (int mode = 0; mode < 2; ++mode)
            for (int mate = 0; mate < 2; ++mate)
                for (long long nf : {n, n / 2, 0ll}) {
                    // the several-kernel packer takes in four goes: the record index (a stream's), what classifies, the mate join's, and
                    // — once the kept reads are counted — their compacted arrays
                    PkScratch<SK_N> s = pk_several_scratch(n, mode, mate != 0);
                    const size_t reserved = s.end(start);                   // (every record kept)
                    CountingArena a = {start};
                    size_t summed = start;
                    bool ok = pass(s, a, SK_REC_OFF, SK_INFO, &summed) && pass(s, a, SK_INFO, SK_MATE_TABLE, &summed) && pass(s, a, SK_MATE_TABLE, SK_C_IDX, &summed);
                    pk_several_kept(s, nf);
                    ok = ok && pass(s, a, SK_C_IDX, SK_N, &summed) && a.used <= reserved && (nf != n || a.used == reserved);
                    std::printf("several %lld %d %d %lld : %zu %zu\n", n, mode, mate, nf, summed, a.used);
                    if (!ok) { std::printf("FAILED\n"); return 1; }
                    ++lines;
                }
    for (long long n : records)
        for (long long nb : blocks)
            for (int mate = 0; mate < 2; ++mate)
                for (int prefix = 0; prefix < 2; ++prefix) {
                    PkScratch<OS_N> s = pk_one_sync_scratch(n, nb, mate != 0, prefix != 0);
                    CountingArena a = {start};
                    size_t summed = start;
                    const bool ok = pass(s, a, 0, OS_N, &summed);
                    std::printf("one_sync %lld %lld %d %d : %zu %zu\n", n, nb, mate, prefix, summed, a.used);
                    if (!ok) { std::printf("FAILED\n"); return 1; }
                    ++lines;
                }
    std::printf("ok %d\n", lines);
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    const char *cmd = argc > 1 ? argv[1] : "";
    if (!std::strcmp(cmd, "flags") && argc == 2) {
        const struct { const char *name; unsigned v; } f[] = {
            {"PKF_LONG", PKF_LONG}, {"PKF_FARPOS", PKF_FARPOS}, {"PKF_BADREAD", PKF_BADREAD}, {"PKF_EVENT_OVF", PKF_EVENT_OVF}, {"PKF_CHUNK_OVF", PKF_CHUNK_OVF},
            {"PKF_HEADER_OVF", PKF_HEADER_OVF}, {"PKF_WORD_OVF", PKF_WORD_OVF}, {"PKF_MULTIREF", PKF_MULTIREF}, {"PKF_CHAIN", PKF_CHAIN}, {"PKF_STAT", PKF_STAT},
            {"PKF_REC_OVF", PKF_REC_OVF}, {"PKF_SLOT_OVF", PKF_SLOT_OVF}};
        for (const auto &e : f) std::printf("%s %u\n", e.name, e.v);
        return 0;
    }
    if (!std::strcmp(cmd, "caps") && argc == 8) {
        const PkCaps c = pk_one_sync_caps((uint64_t)num(argv[2]), (uint32_t)num(argv[3]), num(argv[4]) != 0, num(argv[5]), num(argv[6]), num(argv[7]) != 0);
        std::printf("%lld %llu %u %u %lld\n", (long long)c.rec_cap, (unsigned long long)c.word_cap, c.chunk_cap, c.event_cap, (long long)c.n_wg);
        return 0;
    }
    if (!std::strcmp(cmd, "fits") && argc == 10) {
        PkCaps c = {};
        c.rec_cap = num(argv[2]); c.word_cap = (uint64_t)num(argv[3]); c.chunk_cap = (uint32_t)num(argv[4]); c.event_cap = (uint32_t)num(argv[5]);
        std::printf("%u\n", pk_beyond_caps(c, (uint64_t)num(argv[6]), (uint64_t)num(argv[7]), (uint32_t)num(argv[8]), (uint32_t)num(argv[9])));
        return 0;
    }
    if (!std::strcmp(cmd, "pin") && argc == 3) {
        const ReportPin p(num(argv[2]));
        std::printf("%zu %zu %zu %zu %zu\n", p.alg, p.end, p.stat, p.mate, p.bytes);
        return 0;
    }
    if (!std::strcmp(cmd, "rest") && argc == 6) {
        const long long n = num(argv[2]), nb = num(argv[3]);
        const bool mate = num(argv[4]) != 0;
        std::printf("%zu %zu\n", pk_several_scratch(n, 1, mate).end(0), pk_one_sync_scratch(n, nb, mate, pk_prefix_on((int)num(argv[5]), nb)).end(0));
        return 0;
    }
    if (!std::strcmp(cmd, "scratch") && argc == 3) return scratch_grid((size_t)num(argv[2]));
    std::fprintf(stderr, "usage: pack_caps_main flags | caps .. | fits .. | pin N | rest .. | scratch START (see the head of tests/pack_caps_main.cpp)\n");
    return 2;
}
