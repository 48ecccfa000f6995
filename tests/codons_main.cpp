// codons_main.cpp — a program of its own over csrc/codon_rule.h and csrc/codons_text.cpp and nothing else (no HIP, no GPU):
// tests/test_codon_rule.py builds it plain and with AddressSanitizer + UBSan and runs it as a program.
//   codons_main aa IN OUT        IN: int64 n, then n x {b0, b1, b2} (int32).  OUT: n bytes, tcmi_codon_aa's letters
//   codons_main select IN OUT    IN: int64 {n, n_cds}, n tcmi_variant, n_cds tcmi_cds.  OUT: "rc n_found\n", then one c0 per line.  The
//                                sizing call and a buffer one entry short (TCMI_E_ARG, the same *n_found) are checked here.
//   codons_main text IN OUT      IN: int64 {n, n_cds, L, ld, num, den, min_alt_depth, min_depth, pos_offset, n_region, n_ref, n_names},
//                                the region's bytes, the reference's, the frames' names (n_names bytes, each ended by a zero byte),
//                                n tcmi_codon_counts, n_cds tcmi_cds, the matrix (7 x ld int32).  OUT: "rc len\n" of the call with a
//                                buffer of exactly the sizing call's length, then the text.  The sizing call, a buffer one byte short
//                                (TCMI_E_ARG, the same *len) and a buffer with room to spare whose tail must stay untouched are
//                                checked here.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../trueconsense_amd/csrc/codon_rule.h"

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

int main(int argc, char **argv)
{
    if (argc != 4) return fail("usage: codons_main aa|select|text IN OUT");
    std::vector<char> in;
    if (!read_all(argv[2], in) || in.size() < 8) return fail("cannot read IN");
    FILE *out = std::fopen(argv[3], "wb");
    if (!out) return fail("cannot open OUT");
    int64_t n;
    std::memcpy(&n, in.data(), 8);
    if (!std::strcmp(argv[1], "aa")) {
        if (n < 0 || in.size() != 8 + (size_t)n * 12) return fail("aa: IN has the wrong size");
        for (int64_t i = 0; i < n; ++i) {
            int32_t b[3];
            std::memcpy(b, in.data() + 8 + (size_t)i * 12, 12);
            const int got = tcmi_codon_aa(b[0], b[1], b[2]);
            if (got != tcmi_codon_aa_rule(b[0], b[1], b[2])) return fail("the ABI's letter is not the header's");
            std::fputc(got, out);
        }
        std::fclose(out);
        std::printf("ok %lld codons\n", (long long)n);
        return 0;
    }
    if (!std::strcmp(argv[1], "select")) {
        int64_t h[2];
        if (in.size() < 16) return fail("select: IN has no header");
        std::memcpy(h, in.data(), 16);
        const int64_t n_cds = h[1];
        if (n < 0 || n_cds < 0 || in.size() != 16 + (size_t)n * 16 + (size_t)n_cds * 16) return fail("select: IN has the wrong size");
        std::vector<tcmi_variant> recs((size_t)n);
        if (n) std::memcpy(recs.data(), in.data() + 16, (size_t)n * 16);
        std::vector<tcmi_cds> cds((size_t)n_cds);
        if (n_cds) std::memcpy(cds.data(), in.data() + 16 + (size_t)n * 16, (size_t)n_cds * 16);
        int64_t want = -1, found = -1;
        const int rc0 = tcmi_codon_select(recs.data(), n, cds.data(), n_cds, nullptr, 0, &want);
        std::vector<int64_t> c0((size_t)(want > 0 ? want : 0));
        const int rc = want > 0 ? tcmi_codon_select(recs.data(), n, cds.data(), n_cds, c0.data(), want, &found) : rc0;
        if (want <= 0) found = want;
        if (rc != rc0 || found != want) return fail("the sizing call and the call disagree");
        if (rc == TCMI_OK && want > 1) {                    // one entry short: refused, *n_found says how many
            std::vector<int64_t> small((size_t)want - 1);
            int64_t f2 = -1;
            if (tcmi_codon_select(recs.data(), n, cds.data(), n_cds, small.data(), want - 1, &f2) != TCMI_E_ARG || f2 != want)
                return fail("a short buffer was not refused with the full number");
        }
        if (rc != TCMI_OK && want != 0) return fail("a refusal left a number");
        std::fprintf(out, "%d %lld\n", rc, (long long)(rc == TCMI_OK ? want : 0));
        for (int64_t i = 0; rc == TCMI_OK && i < want; ++i) std::fprintf(out, "%lld\n", (long long)c0[(size_t)i]);
        std::fclose(out);
        std::printf("ok select rc %d\n", rc);
        return 0;
    }
    if (std::strcmp(argv[1], "text")) return fail("aa, select or text");
    int64_t h[12];
    if (in.size() < 96) return fail("text: IN has no header");
    std::memcpy(h, in.data(), 96);
    const int64_t n_cds = h[1], L = h[2], ld = h[3], n_region = h[9], n_ref = h[10], n_names = h[11];
    if (n < 0 || n_cds < 0 || ld < 0 || n_region < 0 || n_ref < 0 || n_names < 0 ||
        in.size() != 96 + (size_t)n_region + (size_t)n_ref + (size_t)n_names + (size_t)n * sizeof(tcmi_codon_counts) + (size_t)n_cds * 16 + (size_t)ld * 28)
        return fail("text: IN has the wrong size");
    const char *p = in.data() + 96;
    const std::string region(p, (size_t)n_region);
    p += n_region;
    // (copies of their own, exactly as long as they claim to be: a read behind one of them is the sanitizer's to find)
    std::vector<uint8_t> ref(p, p + n_ref);
    p += n_ref;
    std::vector<std::string> names;
    for (const char *q = p; q < p + n_names; q += std::strlen(q) + 1) names.emplace_back(q);
    p += n_names;
    if ((int64_t)names.size() != n_cds) return fail("text: IN does not name every frame");
    std::vector<const char *> name_ptrs;
    for (const std::string &s : names) name_ptrs.push_back(s.c_str());
    std::vector<tcmi_codon_counts> counts((size_t)n);
    if (n) std::memcpy(counts.data(), p, (size_t)n * sizeof(tcmi_codon_counts));
    p += (size_t)n * sizeof(tcmi_codon_counts);
    std::vector<tcmi_cds> cds((size_t)n_cds);
    if (n_cds) std::memcpy(cds.data(), p, (size_t)n_cds * 16);
    p += n_cds * 16;
    std::vector<int32_t> matrix((size_t)ld * 7);
    if (ld) std::memcpy(matrix.data(), p, (size_t)ld * 28);
    auto call = [&](char *text, int64_t cap, int64_t *len) {
        return tcmi_codons_text(counts.data(), n, cds.data(), n_cds, name_ptrs.data(), matrix.data(), L, ld, h[4], h[5], (int32_t)h[6], (int32_t)h[7],
                                region.c_str(), h[8], ref.data(), n_ref, text, cap, len);
    };
    int64_t want = -1, len = -1;
    const int rc0 = call(nullptr, 0, &want);                // the sizing call
    std::vector<char> text((size_t)(want > 0 ? want : 0) + 1);
    const int rc = call(text.data(), want > 0 ? want : 0, &len);
    if (rc != rc0) return fail("the sizing call and the call disagree");
    if (rc == TCMI_OK) {
        if (len != want) return fail("*len differs between the sizing call and the call");
        if (want > 0) {                                     // one byte short: refused, *len says how much
            std::vector<char> small((size_t)want - 1 + 1);
            int64_t l2 = -1;
            if (call(small.data(), want - 1, &l2) != TCMI_E_ARG || l2 != want) return fail("a short buffer was not refused with the full length");
        }
        std::vector<char> big((size_t)want + 64, '\x7f');   // room to spare: nothing behind the rows is written
        int64_t l3 = -1;
        if (call(big.data(), want + 64, &l3) != TCMI_OK || l3 != want || std::memcmp(big.data(), text.data(), (size_t)want)) return fail("a larger buffer gives other rows");
        for (int64_t k = want; k < want + 64; ++k)
            if (big[(size_t)k] != '\x7f') return fail("bytes behind the rows were written");
    } else if (len != 0 || want != 0) return fail("a refusal left a length");
    std::fprintf(out, "%d %lld\n", rc, (long long)(rc == TCMI_OK ? len : 0));
    if (rc == TCMI_OK) std::fwrite(text.data(), 1, (size_t)len, out);
    std::fclose(out);
    std::printf("ok text rc %d\n", rc);
    return 0;
}
