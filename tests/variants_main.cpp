// variants_main.cpp — csrc/variants_rule.h and csrc/variants_text.cpp as a program of their own (tests/test_variant_rule.py
// builds it with a plain compiler under AddressSanitizer + UBSan and runs it as a child process; no GPU, no HIP header).
//   variants_main IN OUT_RECORDS OUT_TEXT
// IN: eight int64 {L, n_ref, num, den, min_alt_depth, min_depth, pos_offset, region bytes}, the region's bytes, the reference's
// n_ref bytes, then the count matrix as int32 rows [L][7].  OUT_RECORDS: the rule's records, 16 bytes each, in the table's order;
// OUT_TEXT: tcmi_variants_text of them, written through a buffer of exactly the length a first call with text = NULL asked for.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/tcmi.h"
#include "../trueconsense_amd/csrc/variants_rule.h"

static bool read_all(const char *path, std::vector<char> &out)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    char buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
    std::fclose(f);
    return true;
}

static bool write_all(const char *path, const void *p, size_t n)
{
    FILE *f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = n == 0 || std::fwrite(p, 1, n, f) == n;
    return std::fclose(f) == 0 && ok;
}

int main(int argc, char **argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: variants_main IN OUT_RECORDS OUT_TEXT\n"); return 2; }
    std::vector<char> in;
    if (!read_all(argv[1], in) || in.size() < 64) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int64_t h[8];
    std::memcpy(h, in.data(), 64);
    const int64_t L = h[0], n_ref = h[1], pos_offset = h[6], n_region = h[7];
    if (L < 0 || n_ref < 0 || n_region < 0 || (int64_t)in.size() != 64 + n_region + n_ref + L * 28) { std::fprintf(stderr, "bad input sizes\n"); return 2; }
    const tcmi_var_rule rule = {h[2], h[3], (int32_t)h[4], (int32_t)h[5]};
    const std::string region(in.data() + 64, (size_t)n_region);
    const std::vector<uint8_t> ref(in.begin() + 64 + n_region, in.begin() + 64 + n_region + n_ref);
    std::vector<int32_t> counts((size_t)L * 7);
    if (L) std::memcpy(counts.data(), in.data() + 64 + n_region + n_ref, (size_t)L * 28);

    std::vector<tcmi_variant> rec;
    for (int64_t p = 0; p < L; ++p) {
        const int32_t *c = counts.data() + p * 7;
        const unsigned m = tcmi_variant_mask(c, p < n_ref ? ref[(size_t)p] : 0, rule);
        for (int a = TCMI_A; a <= TCMI_I; ++a)
            if (m >> (a - 1) & 1u) rec.push_back(tcmi_variant{(int32_t)p, a, c[a], c[0]});
    }
    int64_t need = 0, len = 0;
    int rc = tcmi_variants_text(rec.data(), (int64_t)rec.size(), region.c_str(), pos_offset, ref.data(), n_ref, nullptr, 0, &need);
    if (rc != TCMI_OK) { std::fprintf(stderr, "sizing call returned %d (need %lld)\n", rc, (long long)need); return 1; }
    std::vector<char> text((size_t)need);
    rc = tcmi_variants_text(rec.data(), (int64_t)rec.size(), region.c_str(), pos_offset, ref.data(), n_ref, text.data(), need, &len);
    if (rc != TCMI_OK || len != need) { std::fprintf(stderr, "tcmi_variants_text returned %d, %lld of %lld bytes\n", rc, (long long)len, (long long)need); return 1; }
    if (need > 1) {                 // one byte short: refused, and told how much is needed
        std::vector<char> tight((size_t)need - 1);
        rc = tcmi_variants_text(rec.data(), (int64_t)rec.size(), region.c_str(), pos_offset, ref.data(), n_ref, tight.data(), need - 1, &len);
        if (rc != TCMI_E_ARG || len != need) { std::fprintf(stderr, "a buffer one byte short: %d, %lld\n", rc, (long long)len); return 1; }
    }
    if (!write_all(argv[2], rec.data(), rec.size() * sizeof(tcmi_variant)) || !write_all(argv[3], text.data(), text.size())) {
        std::fprintf(stderr, "cannot write the outputs\n");
        return 2;
    }
    std::printf("ok %zu\n", rec.size());
    return 0;
}
