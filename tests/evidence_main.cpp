// evidence_main.cpp — a program of its own over csrc/evidence_rule.h and csrc/variants_evidence_text.cpp and nothing else (no HIP, no
// GPU): tests/test_evidence_rule.py builds it plain and with AddressSanitizer + UBSan and runs it as a program.
//   evidence_main verdict IN OUT   IN: int64 n, then n x {n, qual, mapq, dist, min_qual, min_mapq, min_dist} (int64)
//                                  OUT: n int32, tcmi_evidence_verdict's answers
//   evidence_main lds IN OUT       IN: int64 n, then n x {n_cols, n_records, grid, block} (int64)
//                                  OUT: n int32, tcmi_evidence_lds_ok's answers
//   evidence_main text IN OUT      IN: int64 {n, n_cols, min_qual, min_mapq, min_dist, pos_offset, n_region, n_ref}, the region's bytes, the
//                                  reference's, n tcmi_variant, n_cols tcmi_evidence_counts.  OUT: "rc len\n" of the call with a buffer of
//                                  exactly the sizing call's length, then the text.  The sizing call, a buffer one byte short (TCMI_E_ARG,
//                                  the same *len, nothing written), a buffer with room to spare whose tail must stay untouched, and a
//                                  refusal that writes nothing are checked here.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../trueconsense_amd/csrc/evidence_rule.h"

static bool read_all(const char *path, std::vector<char> &buf)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    char tmp[65536];
    size_t m;
    while ((m = std::fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + m);
    std::fclose(f);
    return true;
}

static int fail(const char *what)
{
    std::printf("FAILED: %s\n", what);
    return 1;
}

static bool all_are(const std::vector<char> &v, char c)
{
    for (char x : v)
        if (x != c) return false;
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 4) return fail("usage: evidence_main verdict|lds|text IN OUT");
    std::vector<char> in;
    if (!read_all(argv[2], in) || in.size() < 8) return fail("cannot read IN");
    FILE *out = std::fopen(argv[3], "wb");
    if (!out) return fail("cannot open OUT");
    int64_t n;
    std::memcpy(&n, in.data(), 8);
    if (!std::strcmp(argv[1], "verdict")) {
        if (n < 0 || in.size() != 8 + (size_t)n * 56) return fail("verdict: IN has the wrong size");
        std::vector<int32_t> got((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            int64_t v[7];
            std::memcpy(v, in.data() + 8 + (size_t)i * 56, 56);
            got[(size_t)i] = tcmi_evidence_verdict(v[0], v[1], v[2], v[3], (int32_t)v[4], (int32_t)v[5], (int32_t)v[6]);
            if (got[(size_t)i] != tcmi_evidence_rule(v[0], v[1], v[2], v[3], (int32_t)v[4], (int32_t)v[5], (int32_t)v[6]))
                return fail("the ABI's verdict is not the header's");
        }
        std::fwrite(got.data(), 4, got.size(), out);
        std::fclose(out);
        std::printf("ok %lld verdicts\n", (long long)n);
        return 0;
    }
    if (!std::strcmp(argv[1], "lds")) {
        if (n < 0 || in.size() != 8 + (size_t)n * 32) return fail("lds: IN has the wrong size");
        std::vector<int32_t> got((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            int64_t v[4];
            std::memcpy(v, in.data() + 8 + (size_t)i * 32, 32);
            got[(size_t)i] = tcmi_evidence_lds_ok(v[0], v[1], v[2], v[3]) ? 1 : 0;
        }
        std::fwrite(got.data(), 4, got.size(), out);
        std::fclose(out);
        std::printf("ok %lld bounds\n", (long long)n);
        return 0;
    }
    if (std::strcmp(argv[1], "text")) return fail("verdict, lds or text");
    int64_t h[8];
    if (in.size() < 64) return fail("text: IN has no header");
    std::memcpy(h, in.data(), 64);
    const int64_t n_cols = h[1], n_region = h[6], n_ref = h[7];
    if (n < 0 || n_cols < 0 || n_region < 0 || n_ref < 0 || in.size() != 64 + (size_t)n_region + (size_t)n_ref + (size_t)n * 16 + (size_t)n_cols * 200)
        return fail("text: IN has the wrong size");
    const char *p = in.data() + 64;
    const std::string region(p, (size_t)n_region);
    p += n_region;
    // (copies of their own, exactly as long as they claim to be: a read behind one of them is the sanitizer's to find)
    std::vector<uint8_t> ref(p, p + n_ref);
    p += n_ref;
    std::vector<tcmi_variant> recs((size_t)n);
    if (n) std::memcpy(recs.data(), p, (size_t)n * 16);
    p += n * 16;
    std::vector<tcmi_evidence_counts> ev((size_t)n_cols);
    if (n_cols) std::memcpy(ev.data(), p, (size_t)n_cols * 200);
    auto call = [&](char *text, int64_t cap, int64_t *len) {
        return tcmi_variants_evidence_text(recs.data(), n, ev.data(), n_cols, (int32_t)h[2], (int32_t)h[3], (int32_t)h[4], region.c_str(), h[5], ref.data(), n_ref,
                                           text, cap, len);
    };
    int64_t want = -1, len = -1;
    const int rc0 = call(nullptr, 0, &want);                // the sizing call
    std::vector<char> text((size_t)(want > 0 ? want : 0) + 1);
    const int rc = call(text.data(), want > 0 ? want : 0, &len);
    if (rc != rc0) return fail("the sizing call and the call disagree");
    if (rc == TCMI_OK) {
        if (len != want) return fail("*len differs between the sizing call and the call");
        if (want > 0) {                                     // one byte short: refused, *len says how much, nothing is written
            std::vector<char> small((size_t)want - 1 + 1, '\x7f');
            int64_t l2 = -1;
            if (call(small.data(), want - 1, &l2) != TCMI_E_ARG || l2 != want) return fail("a short buffer was not refused with the full length");
            if (!all_are(small, '\x7f')) return fail("a short buffer was written to");
        }
        std::vector<char> big((size_t)want + 64, '\x7f');   // room to spare: nothing behind the rows is written
        int64_t l3 = -1;
        if (call(big.data(), want + 64, &l3) != TCMI_OK || l3 != want || std::memcmp(big.data(), text.data(), (size_t)want)) return fail("a larger buffer gives other rows");
        for (int64_t k = want; k < want + 64; ++k)
            if (big[(size_t)k] != '\x7f') return fail("bytes behind the rows were written");
    } else {
        if (len != 0 || want != 0) return fail("a refusal left a length");
        std::vector<char> big(4096, '\x7f');                // a refusal writes nothing, whatever the room
        int64_t l4 = -1;
        if (call(big.data(), 4096, &l4) != rc || l4 != 0 || !all_are(big, '\x7f')) return fail("a refusal wrote text");
    }
    std::fprintf(out, "%d %lld\n", rc, (long long)(rc == TCMI_OK ? len : 0));
    if (rc == TCMI_OK) std::fwrite(text.data(), 1, (size_t)len, out);
    std::fclose(out);
    std::printf("ok text rc %d\n", rc);
    return 0;
}
