// amplicons_main.cpp — csrc/intervals_rule.h and csrc/amplicons_text.cpp as a program of their own (tests/test_amplicon_scheme.py
// builds it with a plain compiler under AddressSanitizer + UBSan and runs it as a child process; no GPU, no HIP header).
//   amplicons_main IN OUT_RECORDS OUT_TEXT
// IN: eight int64 {L, n, min_depth, pos_offset, sample bytes, region bytes, bytes of the names, bytes of the pools}, the sample's
// and the region's bytes, the n names and the n pools each NUL-terminated, n int64 starts, n int64 ends, then the coverage plane as L
// int32.  OUT_RECORDS: this program's records of the intervals, 32 bytes each; OUT_TEXT: tcmi_amplicons_text of them (starts as
// given), written through a buffer of exactly the length a first call with text = NULL asked for.  Before that the argument checks
// of the header are put through every refusal.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/tcmi.h"
#include "../trueconsense_amd/csrc/intervals_rule.h"

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

// the record of one interval over the coverage plane cov[0..L) (a position at or beyond L has depth 0), by listing and sorting its
// columns: this program's own rule, for the writer to have records to print
static tcmi_interval_stat record_of(const int32_t *cov, int64_t L, int64_t start, int64_t end, int32_t min_depth)
{
    tcmi_interval_stat r = {0, 0, 0, -1, 0, 0, 0};
    const int64_t n = end - start;
    if (n <= 0) return r;
    std::vector<int32_t> d((size_t)n);                      // (exactly the interval: the sanitizer sees a step too far)
    for (int64_t k = 0; k < n; ++k) d[(size_t)k] = start + k < L ? cov[start + k] : 0;
    r.n = (int32_t)n;
    r.min = d[0];
    r.min_pos = (int32_t)start;
    for (int64_t k = 0; k < n; ++k) {
        r.sum += d[(size_t)k];
        r.below += d[(size_t)k] < min_depth;
        if (d[(size_t)k] < r.min) { r.min = d[(size_t)k]; r.min_pos = (int32_t)(start + k); }
    }
    std::sort(d.begin(), d.end());
    r.median = d[(size_t)((n - 1) / 2)];
    return r;
}

static int check_the_checks()
{
    const int64_t s[3] = {0, 5, 7}, e[3] = {0, 9, TCMI_IV_MAX_END};
    int64_t bad = 99;
    if (tcmi_intervals_check(3, s, e, 0, &bad) != 0 || bad != -1) return 1;
    if (tcmi_intervals_check(0, nullptr, nullptr, 0, &bad) != 0) return 2;
    if (tcmi_intervals_check(-1, s, e, 0, &bad) != 1 || tcmi_intervals_check(TCMI_IV_MAX_N + 1, s, e, 0, &bad) != 1) return 3;
    if (tcmi_intervals_check(3, s, e, -1, &bad) != 2) return 4;
    if (tcmi_intervals_check(3, nullptr, e, 0, &bad) != 4 || tcmi_intervals_check(3, s, nullptr, 0, &bad) != 4) return 5;
    const int64_t s1[3] = {0, -1, 7}, e1[3] = {0, 4, 6}, e2[3] = {0, 9, TCMI_IV_MAX_END + 1};
    if (tcmi_intervals_check(3, s1, e, 0, &bad) != 3 || bad != 1) return 6;
    if (tcmi_intervals_check(3, s, e1, 0, &bad) != 3 || bad != 1) return 7;        // end < start (4 < 5)
    if (tcmi_intervals_check(3, s, e2, 0, &bad) != 3 || bad != 2) return 8;
    std::vector<int64_t> many((size_t)TCMI_IV_MAX_N, 3);
    if (tcmi_intervals_check(TCMI_IV_MAX_N, many.data(), many.data(), 2147483647, nullptr) != 0) return 9;
    // the text's refusals
    int64_t len = -1;
    const char *nm[1] = {"a"}, *pl[1] = {"1"};
    const int64_t st[1] = {10};
    tcmi_interval_stat r = {30, 3, 5, 11, 10, 0, 0};
    if (tcmi_amplicons_text(&r, 1, "s", "c", nm, pl, st, 0, nullptr, 0, &len) != TCMI_OK || len <= 0) return 11;
    if (tcmi_amplicons_text(&r, 1, "s", "c", nm, pl, st, 11, nullptr, 0, &len) != TCMI_E_ARG) return 12;      // a start in front of the offset
    r.min_pos = 13;
    if (tcmi_amplicons_text(&r, 1, "s", "c", nm, pl, st, 0, nullptr, 0, &len) != TCMI_E_ARG) return 13;       // min_pos outside the interval
    r.min_pos = 9;
    if (tcmi_amplicons_text(&r, 1, "s", "c", nm, pl, st, 0, nullptr, 0, &len) != TCMI_E_ARG) return 14;
    r.min_pos = 11; r.n = -1;
    if (tcmi_amplicons_text(&r, 1, "s", "c", nm, pl, st, 0, nullptr, 0, &len) != TCMI_E_ARG) return 15;
    r.n = 3;
    if (tcmi_amplicons_text(&r, -1, "s", "c", nm, pl, st, 0, nullptr, 0, &len) != TCMI_E_ARG) return 16;
    if (tcmi_amplicons_text(&r, 1, nullptr, "c", nm, pl, st, 0, nullptr, 0, &len) != TCMI_E_ARG) return 17;
    if (tcmi_amplicons_text(&r, 1, "s", "c", nm, pl, nullptr, 0, nullptr, 0, &len) != TCMI_E_ARG) return 18;
    if (tcmi_amplicons_text(&r, 1, "s", "c", nm, pl, st, 0, nullptr, 5, &len) != TCMI_E_ARG) return 19;       // room without a buffer
    if (tcmi_amplicons_text(nullptr, 0, "s", "c", nullptr, nullptr, nullptr, 0, nullptr, 0, &len) != TCMI_OK || len != 0) return 20;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: amplicons_main IN OUT_RECORDS OUT_TEXT\n"); return 2; }
    const int bad = check_the_checks();
    if (bad) { std::fprintf(stderr, "argument check %d gave the wrong answer\n", bad); return 1; }
    std::vector<char> in;
    if (!read_all(argv[1], in) || in.size() < 64) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int64_t h[8];
    std::memcpy(h, in.data(), 64);
    const int64_t L = h[0], n = h[1], pos_offset = h[3];
    for (int k = 0; k < 8; ++k)
        if (h[k] < 0) { std::fprintf(stderr, "bad input sizes\n"); return 2; }
    if ((int64_t)in.size() != 64 + h[4] + h[5] + h[6] + h[7] + n * 16 + L * 4) { std::fprintf(stderr, "bad input sizes\n"); return 2; }
    const char *p = in.data() + 64;
    const std::string sample(p, (size_t)h[4]), region(p + h[4], (size_t)h[5]);
    p += h[4] + h[5];
    std::vector<std::string> names, pools;
    for (int pass = 0; pass < 2; ++pass) {
        const char *end = p + h[6 + pass];
        for (int64_t i = 0; i < n; ++i) {
            const void *z = p < end ? std::memchr(p, 0, (size_t)(end - p)) : nullptr;
            if (!z) { std::fprintf(stderr, "a name without its end\n"); return 2; }
            (pass ? pools : names).emplace_back(p);
            p = (const char *)z + 1;
        }
        if (p != end) { std::fprintf(stderr, "bytes behind the names\n"); return 2; }
    }
    std::vector<int64_t> start((size_t)n), end((size_t)n);
    std::vector<int32_t> cov((size_t)L);
    if (n) { std::memcpy(start.data(), p, (size_t)n * 8); std::memcpy(end.data(), p + n * 8, (size_t)n * 8); }
    if (L) std::memcpy(cov.data(), p + n * 16, (size_t)L * 4);
    if (tcmi_intervals_check(n, start.data(), end.data(), (int32_t)h[2], nullptr) != 0) { std::fprintf(stderr, "the intervals are refused\n"); return 1; }

    std::vector<tcmi_interval_stat> rec((size_t)n);
    for (int64_t i = 0; i < n; ++i) rec[(size_t)i] = record_of(cov.data(), L, start[i], end[i], (int32_t)h[2]);
    std::vector<const char *> nm, pl;
    for (int64_t i = 0; i < n; ++i) { nm.push_back(names[(size_t)i].c_str()); pl.push_back(pools[(size_t)i].c_str()); }
    int64_t need = 0, len = 0;
    int rc = tcmi_amplicons_text(rec.data(), n, sample.c_str(), region.c_str(), nm.data(), pl.data(), start.data(), pos_offset, nullptr, 0, &need);
    if (rc != TCMI_OK) { std::fprintf(stderr, "sizing call returned %d (need %lld)\n", rc, (long long)need); return 1; }
    std::vector<char> text((size_t)need);
    rc = tcmi_amplicons_text(rec.data(), n, sample.c_str(), region.c_str(), nm.data(), pl.data(), start.data(), pos_offset, text.data(), need, &len);
    if (rc != TCMI_OK || len != need) { std::fprintf(stderr, "tcmi_amplicons_text returned %d, %lld of %lld bytes\n", rc, (long long)len, (long long)need); return 1; }
    if (need > 1) {                 // one byte short: refused, and told how much is needed
        std::vector<char> tight((size_t)need - 1);
        rc = tcmi_amplicons_text(rec.data(), n, sample.c_str(), region.c_str(), nm.data(), pl.data(), start.data(), pos_offset, tight.data(), need - 1, &len);
        if (rc != TCMI_E_ARG || len != need) { std::fprintf(stderr, "a buffer one byte short: %d, %lld\n", rc, (long long)len); return 1; }
    }
    if (!write_all(argv[2], rec.data(), rec.size() * sizeof(tcmi_interval_stat)) || !write_all(argv[3], text.data(), text.size())) {
        std::fprintf(stderr, "cannot write the outputs\n");
        return 2;
    }
    std::printf("ok %zu\n", rec.size());
    return 0;
}
