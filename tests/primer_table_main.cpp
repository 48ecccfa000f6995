// primer_table_main.cpp — a stand-alone program over csrc/primer_table.cpp (no GPU, no Python): tests/test_primer_mask.py builds it with
// AddressSanitizer + UBSan and runs it.  Random tables with overlapping, nested and alternative primers, at several slacks: the compiled
// lists must be sorted and disjoint, and for every (p, q) on the axis the two lookups must equal the rule's brute force over the
// primer list; then each argument limit.  Prints "ok <tables> <lookups>" and exits 0, or says what differs and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/tcmi.h"
#include "../trueconsense_amd/csrc/primer_table.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n)
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 20) % n);
}

int fail(const char *what, long long a, long long b, long long c, long long d)
{
    std::printf("FAILED %s: %lld %lld %lld %lld\n", what, a, b, c, d);
    return 1;
}

int check_table(int axis, int n, int slack, long long *lookups)
{
    std::vector<int64_t> s((size_t)n), e((size_t)n);
    std::vector<int32_t> r((size_t)n);
    for (int i = 0; i < n; ++i) {
        s[(size_t)i] = rnd((uint32_t)axis - 40);
        r[(size_t)i] = (int32_t)rnd(2);
        if (i > 0 && i % 7 == 0) { s[(size_t)i] = s[(size_t)i - 1]; r[(size_t)i] = r[(size_t)i - 1]; }     // an alternative primer: same start
        e[(size_t)i] = s[(size_t)i] + 1 + rnd(i % 5 == 0 ? 120u : 30u);        // (some long ones: nested primers inside them)
    }
    std::vector<tcmi_pseg> head, tail;
    char msg[200] = "";
    if (tcmi_primers_build(n, s.data(), e.data(), r.data(), slack, head, tail, msg, sizeof msg)) return fail(msg, n, slack, 0, 0);
    // the exported form agrees with the lists
    const int32_t cap = 2 * n + 1;
    std::vector<int32_t> eh((size_t)cap * 3), et((size_t)cap * 3);
    int32_t nh = -1, nt = -1;
    if (tcmi_primers_compile(n, s.data(), e.data(), r.data(), slack, cap, eh.data(), &nh, et.data(), &nt, msg, sizeof msg) != TCMI_OK) return fail(msg, n, slack, 1, 0);
    if (nh != (int32_t)head.size() || nt != (int32_t)tail.size()) return fail("exported sizes", nh, (long long)head.size(), nt, (long long)tail.size());
    for (size_t i = 0; i < head.size(); ++i)
        if (eh[3 * i] != head[i].a || eh[3 * i + 1] != head[i].b || eh[3 * i + 2] != head[i].v) return fail("exported head", (long long)i, 0, 0, 0);
    for (size_t i = 0; i < tail.size(); ++i)
        if (et[3 * i] != tail[i].a || et[3 * i + 1] != tail[i].b || et[3 * i + 2] != tail[i].v) return fail("exported tail", (long long)i, 0, 0, 0);
    for (const std::vector<tcmi_pseg> *lst : {&head, &tail})
        for (size_t i = 0; i < lst->size(); ++i) {
            if ((*lst)[i].a >= (*lst)[i].b) return fail("empty segment", (long long)i, (*lst)[i].a, (*lst)[i].b, 0);
            if (i && (*lst)[i - 1].b > (*lst)[i].a) return fail("segments overlap or are unsorted", (long long)i, (*lst)[i - 1].b, (*lst)[i].a, 0);
        }
    if ((int)head.size() > 2 * n || (int)tail.size() > 2 * n) return fail("more than 2 n segments", (long long)head.size(), (long long)tail.size(), n, 0);
    for (int p = 0; p < axis; ++p) {
        int32_t he = p, ts_of_q = p + 1;                                        // brute force, p as a first column and as a last column
        for (int i = 0; i < n; ++i) {
            if (r[(size_t)i] == 0 && s[(size_t)i] - slack <= p && p < e[(size_t)i] && e[(size_t)i] > he) he = (int32_t)e[(size_t)i];
        }
        bool any = false;
        for (int i = 0; i < n; ++i)
            if (r[(size_t)i] == 1 && s[(size_t)i] <= p && p < e[(size_t)i] + slack && (!any || s[(size_t)i] < ts_of_q)) { ts_of_q = (int32_t)s[(size_t)i]; any = true; }
        const int32_t gh = tcmi_pseg_find(head.data(), (int32_t)head.size(), p, p);
        const int32_t gt = tcmi_pseg_find(tail.data(), (int32_t)tail.size(), p, p + 1);
        if (gh != he) return fail("head_end", p, gh, he, slack);
        if (gt != ts_of_q) return fail("tail_start", p, gt, ts_of_q, slack);
        *lookups += 2;
    }
    return 0;
}

int expect_arg_error(const char *what, int32_t n, const int64_t *s, const int64_t *e, const int32_t *r, int32_t slack)
{
    std::vector<tcmi_pseg> head, tail;
    char msg[200] = "";
    if (tcmi_primers_build(n, s, e, r, slack, head, tail, msg, sizeof msg) == 0 || !msg[0]) return fail(what, n, slack, 0, 0);
    int32_t out[6], nh = 0, nt = 0;
    if (tcmi_primers_compile(n, s, e, r, slack, 2, out, &nh, out + 3, &nt, nullptr, 0) != TCMI_E_ARG) return fail(what, n, slack, 1, 0);
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    const int tables = argc > 1 ? std::atoi(argv[1]) : 60;
    long long lookups = 0;
    for (int t = 0; t < tables; ++t)
        if (check_table(600, 1 + (int)rnd(40), t % 3 == 0 ? 0 : t % 3 == 1 ? 5 : 1000, &lookups)) return 1;
    // an empty table, and the largest one
    {
        std::vector<tcmi_pseg> head, tail;
        if (tcmi_primers_build(0, nullptr, nullptr, nullptr, 0, head, tail, nullptr, 0) || !head.empty() || !tail.empty()) return fail("empty table", 0, 0, 0, 0);
        const int32_t n = TCMI_PRIMERS_MAX;
        std::vector<int64_t> s((size_t)n), e((size_t)n);
        std::vector<int32_t> r((size_t)n);
        for (int32_t i = 0; i < n; ++i) { s[(size_t)i] = 100 * (int64_t)(i / 2); e[(size_t)i] = s[(size_t)i] + 24; r[(size_t)i] = i & 1; }
        char msg[200] = "";
        if (tcmi_primers_build(n, s.data(), e.data(), r.data(), 3, head, tail, msg, sizeof msg)) return fail(msg, n, 0, 0, 0);
        if ((int32_t)head.size() != n / 2 || (int32_t)tail.size() != n / 2) return fail("largest table", (long long)head.size(), (long long)tail.size(), 0, 0);
        s.push_back(0); e.push_back(5); r.push_back(0);
        if (expect_arg_error("n above 65536", n + 1, s.data(), e.data(), r.data(), 0)) return 1;
    }
    const int64_t s1[1] = {10}, e1[1] = {34};
    const int32_t r0[1] = {0}, r2[1] = {2}, rm[1] = {-1};
    const int64_t sneg[1] = {-1}, eeq[1] = {10}, elt[1] = {9}, sbig[1] = {(int64_t)1 << 29}, ebig[1] = {((int64_t)1 << 29) + 24}, eat[1] = {(int64_t)1 << 29},
                  shuge[1] = {(int64_t)1 << 40}, ehuge[1] = {((int64_t)1 << 40) + 5};
    if (expect_arg_error("start < 0", 1, sneg, e1, r0, 0) || expect_arg_error("end == start", 1, s1, eeq, r0, 0) || expect_arg_error("end < start", 1, s1, elt, r0, 0) ||
        expect_arg_error("start at 2^29", 1, sbig, ebig, r0, 0) || expect_arg_error("end at 2^29", 1, s1, eat, r0, 0) || expect_arg_error("beyond int32", 1, shuge, ehuge, r0, 0) ||
        expect_arg_error("strand 2", 1, s1, e1, r2, 0) || expect_arg_error("strand -1", 1, s1, e1, rm, 0) || expect_arg_error("slack -1", 1, s1, e1, r0, -1) ||
        expect_arg_error("slack 1001", 1, s1, e1, r0, 1001) || expect_arg_error("n < 0", -1, s1, e1, r0, 0))
        return 1;
    {   // the last coordinate the table takes
        std::vector<tcmi_pseg> head, tail;
        const int64_t sl[1] = {((int64_t)1 << 29) - 25}, el[1] = {((int64_t)1 << 29) - 1};
        const int32_t r1[1] = {1};
        if (tcmi_primers_build(1, sl, el, r1, 1000, head, tail, nullptr, 0) || tail.size() != 1 || tail[0].b != (int32_t)el[0] + 1000) return fail("last coordinate", 0, 0, 0, 0);
    }
    std::printf("ok %d %lld\n", tables, lookups);
    return 0;
}
