// tests/cigar_rule_main.cpp — csrc/cigar_rule.h in a program of its own, for tests/test_cigar_rule.py (built with AddressSanitizer + UBSan).
//   cigar_rule_main FILE      FILE: little-endian uint32 — per list its number of words n, then the n CIGAR words (len << 4 | op)
// One line per list: the reference span, the query total Yq, the verdict of the 64-bit sums on a record that would otherwise be kept,
// and the verdict of the 32-bit form the kernels carry (tcmi_cigar_step), which must be the same.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../trueconsense_amd/csrc/cigar_rule.h"

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: cigar_rule_main FILE\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    std::vector<uint32_t> w;
    uint32_t n;
    while (std::fread(&n, 4, 1, f) == 1) {
        w.resize(n);
        if (n && std::fread(w.data(), 4, n, f) != n) { std::fprintf(stderr, "truncated list\n"); std::fclose(f); return 2; }
        const uint32_t *p = w.data();
        const tcmi_cigar_sums s = tcmi_cigar_walk([p](uint32_t k) { return p[k]; }, n);
        int64_t span = 0;
        int32_t yr = TCMI_CIGAR_YR0;
        for (uint32_t k = 0; k < n; ++k) tcmi_cigar_step(span, yr, p[k]);
        std::printf("%lld %lld %d %d\n", (long long)s.span, (long long)s.yq, (int)tcmi_cigar_malformed(s), (int)tcmi_cigar_malformed(span, yr));
        if (span != s.span) { std::fprintf(stderr, "the two walks give other spans\n"); std::fclose(f); return 3; }
    }
    std::fclose(f);
    return 0;
}
