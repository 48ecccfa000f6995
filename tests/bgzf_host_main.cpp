// bgzf_host_main.cpp — a program of its own around trueconsense_amd/csrc/bgzf_host.{h,cpp}, built by tests/test_bgzf_host.py with
// AddressSanitizer + UBSan and run as a child process (no GPU, no HIP, nothing of it loaded into python).
//
//   bgzf_host_main table FILE...     what the host parses of each file, for the test to hold against its own restatement:
//                                        file <path>
//                                        refused <code> <byte offset>                              — or —
//                                        parsed <blocks> <inflated> <first record> <refs> <rec_bytes_hint> <tok_total> <pay_dwords>
//                                        block <cin> <clen> <ulen> <uout> <crc> <entry> <1: inflates and its CRC-32 holds>   (per block)
//                                        text <hex>
//                                        ref <length> <name in hex>                                                        (per reference)
//                                        whole <first record>      (every block inflated: the header once more, from the whole stream, as tcmi_bam_load has it)
//   bgzf_host_main damaged FILE...   the same, and a last line "damaged: <n> files, <refused> refused, <parsed> parsed"
//   bgzf_host_main chain             the record-chain rule on a table of hand-made cases; a line per case, exit status 1 if one fails
//   bgzf_host_main chainfile TABLE   the record-chain rule over windows of a block table read from TABLE (chainfile() says how it is
//                                    written); a line per window: <code> <block> <range_first> <range_next> <what>
#include <cstdio>
#include <fstream>
#include <memory>

#include "../trueconsense_amd/csrc/bgzf_host.h"

static void hex(const std::string &s)
{
    for (unsigned char c : s) std::printf("%02x", c);
}

static bool table(const char *path)
{
    std::ifstream in(path, std::ios::binary | std::ios::ate);
    const size_t n = in ? (size_t)in.tellg() : 0;
    const std::unique_ptr<uint8_t[]> file(new uint8_t[n]);      // (an allocation of exactly the file's size: a read past its end is the sanitizer's to report)
    in.seekg(0);
    in.read(reinterpret_cast<char *>(file.get()), (std::streamsize)n);
    std::printf("file %s\n", path);
    tcmi_bam_front f;
    tcmi_parse_error e = tcmi_bam_front_blocks(file.get(), n, &f);
    if (!e.code) e = tcmi_bam_front_header(file.get(), &f);
    if (e.code) {
        std::printf("refused %d %zu\n", e.code, e.at);
        return false;
    }
    std::printf("parsed %zu %zu %zu %zu %u %zu %u\n", f.blocks.size(), f.inflated, f.first_record, f.ref_name.size(), f.rec_bytes_hint, f.tok_total, f.pay_dwords);
    // the members once more, as tcmi_bam_load walks them: the table must be the same one; every block inflated, with its CRC-32
    std::vector<tcmi_bgzf_member> members;
    size_t total = 0;
    const tcmi_parse_error e2 = tcmi_bgzf_walk(file.get(), n, &total, [&members](const tcmi_bgzf_member &m) { members.push_back(m); });
    if (e2.code || total != f.inflated || members.size() != f.blocks.size()) { std::printf("the two walks differ\n"); std::exit(1); }
    std::vector<uint8_t> raw(total);
    bool all = true;
    for (size_t b = 0; b < members.size(); ++b) {
        const tcmi_bgzf_member &m = members[b];
        const BlockDesc &d = f.blocks[b];
        if (m.cin != d.cin || m.clen != d.clen || m.ulen != d.ulen || m.uout != d.uout) { std::printf("the two walks differ\n"); std::exit(1); }
        const bool ok = tcmi_bgzf_inflate(file.get() + m.cin, m.clen, raw.data() + m.uout, m.ulen, &m.crc);
        all = all && ok;
        std::printf("block %zu %zu %zu %zu %u %d %d\n", m.cin, m.clen, m.ulen, m.uout, m.crc, d.entry, ok ? 1 : 0);
    }
    std::printf("text ");
    hex(f.text);
    std::printf("\n");
    for (size_t r = 0; r < f.ref_name.size(); ++r) {
        std::printf("ref %lld ", (long long)f.ref_len[r]);
        hex(f.ref_name[r]);
        std::printf("\n");
    }
    if (all) {
        tcmi_stream_front whole = {raw.data(), raw.size(), nullptr};
        tcmi_bam_head h;
        const tcmi_parse_error e3 = tcmi_bam_header_parse(&whole, &h);
        if (e3.code || h.text != f.text || h.ref_name != f.ref_name || h.ref_len != f.ref_len) { std::printf("the header from the whole stream differs\n"); std::exit(1); }
        std::printf("whole %zu\n", h.first_record);
    }
    return true;
}

// ---- the record chain: hand-made cases ------------------------------------------------------------------------------------
static const uint32_t NONE = 0xFFFFFFFFu;
struct Blk { int32_t entry; uint32_t ulen, stat, first; int32_t over; };
struct Case {
    const char *name;
    bool ranged;
    size_t nb_own;
    std::vector<Blk> b;
    int code;
    size_t block;                       // (code != TCMI_OK)
    int64_t range_first, range_next;    // (code == TCMI_OK)
};

static int chain()
{
    const std::vector<Case> cases = {
        // a header-only block, the block of the first record (the header says where: 50), blocks cut on record boundaries
        {"a chain that closes", false, 4, {{-1, 100, ST_OK, NONE, 0}, {50, 200, ST_OK, 50, 0}, {-2, 200, ST_OK, 0, 0}, {-2, 0, ST_OK, NONE, 0}}, TCMI_OK, 0, -1, 500},
        {"a record straddling two blocks", false, 2, {{12, 200, ST_OK, 12, 30}, {-2, 100, ST_OK, 30, 0}}, TCMI_OK, 0, -1, 300},
        {"a block wholly inside a record", false, 3, {{0, 200, ST_OK, 0, 300}, {-2, 200, ST_OK, NONE, 0}, {-2, 200, ST_OK, 100, 0}}, TCMI_OK, 0, -1, 600},
        {"a start that is not where the predecessor ended", false, 2, {{12, 200, ST_OK, 12, 30}, {-2, 100, ST_OK, 31, 0}}, TCMI_E_UNSUPPORTED, 1, 0, 0},
        {"the header's first record is not where the block found one", false, 1, {{12, 200, ST_OK, 13, 0}}, TCMI_E_UNSUPPORTED, 0, 0, 0},
        {"no start in a block that a record ends in", false, 2, {{0, 200, ST_OK, 0, 50}, {-2, 100, ST_OK, NONE, 0}}, TCMI_E_UNSUPPORTED, 1, 0, 0},
        {"a last record whose size could not be read", false, 2, {{0, 200, ST_OK, 0, -1}, {-2, 100, ST_OK, 0, 0}}, TCMI_E_UNSUPPORTED, 0, 0, 0},
        {"ST_BAD_RECORD", false, 2, {{0, 200, ST_OK, 0, 0}, {-2, 100, ST_BAD_RECORD, 0, 0}}, TCMI_E_FORMAT, 1, 0, 0},
        {"ST_BAD_RECORD in a header-only block does not count", false, 2, {{-1, 200, ST_BAD_RECORD, NONE, 0}, {0, 100, ST_OK, 0, 0}}, TCMI_OK, 0, -1, 300},
        {"ST_BAD_STREAM", false, 3, {{0, 200, ST_OK, 0, 0}, {-2, 100, ST_OK, 0, 0}, {-2, 100, ST_BAD_STREAM, NONE, 0}}, TCMI_E_FORMAT, 2, 0, 0},
        {"ST_BAD_LENGTH", false, 2, {{0, 200, ST_BAD_LENGTH, 0, 0}, {-2, 100, ST_OK, 0, 0}}, TCMI_E_FORMAT, 0, 0, 0},
        {"ST_BAD_CRC", false, 3, {{0, 200, ST_OK, 0, 0}, {-2, 100, ST_BAD_CRC, 0, 0}, {-2, 100, ST_OK, 0, 0}}, TCMI_E_FORMAT, 1, 0, 0},
        {"a damaged stream is named before a CRC in front of it", false, 3, {{0, 200, ST_OK, 0, 0}, {-2, 100, ST_BAD_CRC, 0, 0}, {-2, 100, ST_BAD_STREAM, 0, 0}}, TCMI_E_FORMAT, 2, 0, 0},
        {"ST_BAD_CRC in a range's extra block", true, 1, {{-2, 200, ST_OK, 0, 0}, {-2, 100, ST_BAD_CRC, 0, 0}}, TCMI_E_FORMAT, 1, 0, 0},
        // a range: its first block lies inside a record (no start), the second finds one at 17; one block more is taken along
        {"a range with its extra block", true, 3, {{-2, 100, ST_OK, NONE, 0}, {-2, 200, ST_OK, 17, 40}, {-2, 200, ST_OK, 40, 25}, {-2, 200, ST_OK, 25, 7}}, TCMI_OK, 0, 117, 525},
        {"a range that starts with the file: the header says where", true, 1, {{33, 200, ST_OK, 33, 9}, {-2, 200, ST_OK, 9, 0}}, TCMI_OK, 0, -1, 209},
        {"a range whose last record is longer than the extra block", true, 2, {{-2, 200, ST_OK, 17, 40}, {-2, 200, ST_OK, 40, 300}, {-2, 200, ST_OK, NONE, 0}}, TCMI_E_UNSUPPORTED, 2, 0, 0},
        {"a range whose last record just fits the extra block", true, 2, {{-2, 200, ST_OK, 17, 40}, {-2, 200, ST_OK, 40, 200}, {-2, 200, ST_OK, NONE, 0}}, TCMI_OK, 0, 17, 600},
        {"a range of header blocks only", true, 2, {{-1, 200, ST_OK, NONE, 0}, {-1, 200, ST_OK, NONE, 0}, {5, 200, ST_OK, 5, 0}}, TCMI_OK, 0, -1, -1},
        {"a range in which no block found a start", true, 2, {{-2, 200, ST_OK, NONE, 0}, {-2, 200, ST_OK, NONE, 0}, {-2, 200, ST_OK, 5, 0}}, TCMI_OK, 0, -1, -1},
        {"a last record past the end of the file", false, 2, {{0, 200, ST_OK, 0, 0}, {-2, 100, ST_OK, 0, 12}}, TCMI_E_UNSUPPORTED, 1, 0, 0},
        {"a range that ends with the file, its last record past the end", true, 2, {{-2, 200, ST_OK, 4, 0}, {-2, 100, ST_OK, 0, 12}}, TCMI_E_UNSUPPORTED, 1, 0, 0},
    };
    int bad = 0;
    for (const Case &c : cases) {
        const size_t nb = c.b.size();
        std::vector<BlockDesc> blocks(nb);
        std::vector<uint32_t> stat(nb), first(nb);
        std::vector<int32_t> over(nb);
        uint64_t uout = 0;
        for (size_t b = 0; b < nb; ++b) {
            blocks[b] = BlockDesc{0, uout, 0, c.b[b].ulen, c.b[b].entry, 0, 0};
            uout += c.b[b].ulen;
            stat[b] = c.b[b].stat; first[b] = c.b[b].first; over[b] = c.b[b].over;
        }
        const tcmi_chain_verdict v = tcmi_bam_chain_check(blocks.data(), nb, c.nb_own, c.ranged, stat.data(), first.data(), over.data());
        const bool ok = v.code == c.code && (c.code ? v.block == c.block && !v.what.empty() : v.range_first == c.range_first && v.range_next == c.range_next);
        std::printf("%s  %s: code %d, block %zu, anchors %lld %lld%s%s\n", ok ? "ok  " : "FAIL", c.name, v.code, v.block, (long long)v.range_first, (long long)v.range_next,
                    v.what.empty() ? "" : " — ", v.what.c_str());
        bad += !ok;
    }
    std::printf("chain: %zu cases, %d failed\n", cases.size(), bad);
    return bad ? 1 : 0;
}

// ---- the record chain over a block table from a file, window by window -----------------------------------------------------------------
// TABLE: the number of blocks, then per block "entry ulen first over stat"; the number of windows, then per window "first_block nb_own nb
// ranged".  A window is decoded as a file of its own (bam_device.hip: decode_enqueue): its blocks' places in the stream start at 0, and
// so do the anchors printed for it.
static int chainfile(const char *path)
{
    std::ifstream in(path);
    size_t n = 0, n_win = 0;
    if (!(in >> n)) { std::fprintf(stderr, "%s: no block count\n", path); return 2; }
    std::vector<Blk> all(n);
    for (Blk &b : all) {
        long long entry, ulen, first, over, stat;
        if (!(in >> entry >> ulen >> first >> over >> stat)) { std::fprintf(stderr, "%s: the block table ends early\n", path); return 2; }
        b = Blk{(int32_t)entry, (uint32_t)ulen, (uint32_t)stat, (uint32_t)first, (int32_t)over};
    }
    if (!(in >> n_win)) { std::fprintf(stderr, "%s: no window count\n", path); return 2; }
    std::vector<BlockDesc> blocks;
    std::vector<uint32_t> stat, first;
    std::vector<int32_t> over;
    for (size_t w = 0; w < n_win; ++w) {
        long long fb, nb_own, nb, ranged;
        if (!(in >> fb >> nb_own >> nb >> ranged) || fb < 0 || nb_own < 0 || nb < nb_own || (size_t)(fb + nb) > n) {
            std::fprintf(stderr, "%s: window %zu does not lie in the table\n", path, w);
            return 2;
        }
        blocks.assign((size_t)nb, BlockDesc{});
        stat.assign((size_t)nb, 0); first.assign((size_t)nb, 0); over.assign((size_t)nb, 0);
        uint64_t uout = 0;
        for (size_t b = 0; b < (size_t)nb; ++b) {
            const Blk &s = all[(size_t)fb + b];
            blocks[b] = BlockDesc{0, uout, 0, s.ulen, s.entry, 0, 0};
            uout += s.ulen;
            stat[b] = s.stat; first[b] = s.first; over[b] = s.over;
        }
        const tcmi_chain_verdict v = tcmi_bam_chain_check(blocks.data(), (size_t)nb, (size_t)nb_own, ranged != 0, stat.data(), first.data(), over.data());
        std::printf("%d %zu %lld %lld %s\n", v.code, v.block, (long long)v.range_first, (long long)v.range_next, v.what.c_str());
    }
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "chain") return chain();
    if (mode == "chainfile" && argc == 3) return chainfile(argv[2]);
    if (mode != "table" && mode != "damaged") {
        std::fprintf(stderr, "usage: %s table FILE... | damaged FILE... | chain | chainfile TABLE\n", argv[0]);
        return 2;
    }
    int parsed = 0;
    for (int i = 2; i < argc; ++i) parsed += table(argv[i]) ? 1 : 0;
    if (mode == "damaged") std::printf("damaged: %d files, %d refused, %d parsed\n", argc - 2, argc - 2 - parsed, parsed);
    return 0;
}
