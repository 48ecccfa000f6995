// amplicon_reads_main.cpp — a stand-alone program over csrc/amplicon_reads_rule.h + csrc/amplicon_reads_table.cpp (no GPU, no Python):
// tests/test_amplicon_reads_rule.py builds it once plain and once with AddressSanitizer + UBSan and runs it.  For each scheme it
// compiles the table and sweeps EVERY (p, q), p <= q, of a small axis — columns in front of 0 and beyond the last amplicon included —
// against its own brute force (a loop over all amplicons that counts the containments): a tiled scheme with overlaps; nested,
// identical, touching and disjoint amplicons; n = 1; random schemes; slack 0, 1 and 1000 (widened starts go negative: no clamp);
// coordinates at 2^29; then every argument error.  Prints "ok <schemes> <lookups>" and exits 0, or says what differs and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/tcmi.h"
#include "../trueconsense_amd/csrc/amplicon_reads_rule.h"

namespace {

struct Amp { int64_t fs, le, rs, fe; };

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

// the brute force: -> index, TCMI_AR_AMBIGUOUS or TCMI_AR_UNASSIGNED
int32_t brute(const std::vector<Amp> &amps, int32_t slack, int64_t p, int64_t q, bool *full)
{
    int hits = 0, who = -1;
    for (size_t i = 0; i < amps.size(); ++i)
        if (amps[i].fs - slack <= p && q < amps[i].fe + slack) { ++hits; who = (int)i; }
    *full = hits == 1 && p < amps[(size_t)who].le && q >= amps[(size_t)who].rs;
    return hits == 0 ? TCMI_AR_UNASSIGNED : hits > 1 ? TCMI_AR_AMBIGUOUS : who;
}

int split(const std::vector<Amp> &amps, std::vector<int64_t> v[4])
{
    for (int k = 0; k < 4; ++k) v[k].clear();
    for (const Amp &a : amps) { v[0].push_back(a.fs); v[1].push_back(a.le); v[2].push_back(a.rs); v[3].push_back(a.fe); }
    return (int)amps.size();
}

// compile (both forms) and sweep [lo, hi]
int check_scheme(const char *what, const std::vector<Amp> &amps, int32_t slack, int64_t lo, int64_t hi, long long *lookups)
{
    std::vector<int64_t> v[4];
    const int n = split(amps, v);
    std::vector<int32_t> table((size_t)TCMI_AR_WORDS * (size_t)n), exported((size_t)TCMI_AR_WORDS * (size_t)n);
    char msg[256] = "";
    if (tcmi_amplicon_reads_build(n, v[0].data(), v[1].data(), v[2].data(), v[3].data(), slack, table.data(), msg, sizeof msg)) return fail(msg, n, slack, 0, 0);
    if (tcmi_amplicon_reads_compile(n, v[0].data(), v[1].data(), v[2].data(), v[3].data(), slack, exported.data(), (int64_t)exported.size(), msg, sizeof msg) != TCMI_OK)
        return fail(msg, n, slack, 1, 0);
    if (table != exported) return fail("the exported table differs", n, slack, 0, 0);
    const tcmi_ar_table t = tcmi_ar_view(table.data(), n);
    for (int k = 0; k < n; ++k) {
        if (k && t.a[k - 1] > t.a[k]) return fail("starts are not sorted", k, t.a[k - 1], t.a[k], 0);
        if (k && (t.bmax[k] < t.bmax[k - 1] || t.b2[k] < t.b2[k - 1] || t.b2[k] > t.bmax[k])) return fail("prefix maxima", k, t.bmax[k], t.b2[k], 0);
        if (t.idx[k] < 0 || t.idx[k] >= n || amps[(size_t)t.idx[k]].fe + slack != t.bmax[k]) return fail("the stored index", k, t.idx[k], t.bmax[k], 0);
    }
    if (t.b2[0] != TCMI_AR_NONE) return fail("b2[0]", t.b2[0], 0, 0, 0);
    for (int64_t p = lo; p <= hi; ++p)
        for (int64_t q = p; q <= hi; ++q) {
            bool f1 = false, f2 = false;
            const int32_t got = tcmi_ar_lookup(t, (int32_t)p, (int32_t)q, &f1), want = brute(amps, slack, p, q, &f2);
            if (got != want || f1 != f2) { std::printf("FAILED %s slack %d at (%lld, %lld): got %d %d, want %d %d\n", what, slack, (long long)p, (long long)q, got, (int)f1, want, (int)f2); return 1; }
            ++*lookups;
        }
    return 0;
}

// amplicon 0 of a scheme of n (the others, where there are any, are fine) must be refused with `word` in the message
int expect_arg_error(const char *what, int64_t n, const Amp &first, int32_t slack, const char *word)
{
    std::vector<int64_t> v[4];
    for (int k = 0; k < 4; ++k) v[k].assign(70000, k == 0 ? 1 : k == 1 ? 5 : k == 2 ? 7 : 9);                // (room for the "n above 65536" case)
    v[0][0] = first.fs; v[1][0] = first.le; v[2][0] = first.rs; v[3][0] = first.fe;
    std::vector<int32_t> table((size_t)TCMI_AR_WORDS * 70000);
    char msg[256] = "";
    if (tcmi_amplicon_reads_build(n, v[0].data(), v[1].data(), v[2].data(), v[3].data(), slack, table.data(), msg, sizeof msg) == 0 || !std::strstr(msg, word))
        return fail(what, n, slack, 0, 0);
    msg[0] = 0;
    if (tcmi_amplicon_reads_compile(n, v[0].data(), v[1].data(), v[2].data(), v[3].data(), slack, table.data(), (int64_t)table.size(), msg, sizeof msg) != TCMI_E_ARG ||
        !std::strstr(msg, word))
        return fail(what, n, slack, 1, 0);
    if (tcmi_amplicon_reads_compile(n, v[0].data(), v[1].data(), v[2].data(), v[3].data(), slack, table.data(), (int64_t)table.size(), nullptr, 0) != TCMI_E_ARG)
        return fail(what, n, slack, 2, 0);
    return 0;
}

} // namespace

int main()
{
    long long lookups = 0;
    int schemes = 0;
    const int32_t slacks[3] = {0, 1, 1000};
    const int AXIS = 260;
    // a tiled scheme whose neighbours overlap by 30 columns; amplicon 2 has overlapping primers (le > rs)
    std::vector<Amp> tiled;
    for (int k = 0; k < 5; ++k) tiled.push_back({20 + 40 * k, 30 + 40 * k, 80 + 40 * k, 90 + 40 * k});
    tiled[2] = {100, 150, 120, 170};
    // nested, identical, touching and disjoint amplicons, in no order
    const std::vector<Amp> odd = {{100, 110, 190, 200}, {120, 125, 150, 160}, {100, 110, 190, 200}, {200, 205, 230, 240}, {10, 15, 30, 40}, {120, 130, 150, 180}, {0, 1, 2, 3}};
    const std::vector<Amp> one = {{50, 60, 90, 100}};
    for (int32_t s : slacks) {
        const int64_t lo = s == 1000 ? -3 : -s - 3;         // (at slack 1000 every column of the axis lies inside every amplicon: the sweep still says so)
        if (check_scheme("tiled", tiled, s, lo, AXIS, &lookups) || check_scheme("nested / identical / touching / disjoint", odd, s, lo, AXIS, &lookups) ||
            check_scheme("n = 1", one, s, lo, AXIS, &lookups))
            return 1;
        schemes += 3;
    }
    {   // slack 1000 where it matters: the widened starts are negative and the sweep crosses them
        const std::vector<Amp> far = {{0, 10, 1500, 1510}, {900, 910, 1500, 1520}, {3000, 3010, 3090, 3100}};
        for (const int64_t at : {(int64_t)-1010, (int64_t)380, (int64_t)1900, (int64_t)2400, (int64_t)3950})
            if (check_scheme("slack 1000", far, 1000, at, at + 140, &lookups)) return 1;
        ++schemes;
    }
    for (int trial = 0; trial < 40; ++trial) {             // random schemes: overlapping, nested, repeated starts and ends
        std::vector<Amp> r;
        const int n = 1 + (int)rnd(24);
        for (int i = 0; i < n; ++i) {
            Amp a;
            a.fs = rnd(200);
            a.fe = a.fs + 2 + rnd(i % 4 == 0 ? 120u : 50u);
            if (i > 0 && i % 5 == 0) { a.fs = r[(size_t)i - 1].fs; if (a.fe <= a.fs) a.fe = a.fs + 2; }    // the same start
            if (i > 0 && i % 7 == 0) { a.fe = r[(size_t)i - 1].fe; if (a.fe <= a.fs) a.fe = a.fs + 2; }    // the same end
            a.le = a.fs + 1 + rnd((uint32_t)(a.fe - a.fs));                                 // fs < le <= fe
            a.rs = a.fs + rnd((uint32_t)(a.fe - a.fs));                                     // fs <= rs < fe
            r.push_back(a);
        }
        const int32_t s = slacks[trial % 3 == 2 ? 1 : trial % 3];                           // 0, 1, 1
        if (check_scheme("random", r, s, -4, 330, &lookups)) return 1;
        ++schemes;
    }
    {   // coordinates at 2^29, with and without slack
        const int64_t T = (int64_t)1 << 29;
        const std::vector<Amp> top = {{T - 100, T - 90, T - 10, T}, {T - 60, T - 50, T - 1, T}, {0, 1, 2, 3}};
        for (int32_t s : slacks)
            if (check_scheme("2^29", top, s, T - 130 - (s == 1 ? 1 : 0), T + (s ? 40 : 10), &lookups) || check_scheme("2^29 / far end of slack", top, s, T + s - 20, T + s + 20, &lookups))
                return 1;
        ++schemes;
    }
    // every argument error
    const int64_t T = (int64_t)1 << 29;
    const Amp good = {10, 20, 80, 100}, neg = {-1, 20, 80, 100}, big = {10, 20, 80, T + 1}, bigle = {10, T + 1, 80, 100}, negrs = {10, 20, -5, 100};
    const Amp le_eq = {10, 10, 80, 100}, rs_eq = {10, 20, 100, 100}, fe_le = {50, 60, 20, 30}, huge = {10, 20, 80, (int64_t)1 << 40};
    if (expect_arg_error("n = 0", 0, good, 0, "1..65536") || expect_arg_error("n < 0", -1, good, 0, "1..65536") || expect_arg_error("n above 65536", 65537, good, 0, "1..65536") ||
        expect_arg_error("slack -1", 1, good, -1, "slack") || expect_arg_error("slack 1001", 1, good, 1001, "slack") || expect_arg_error("fs < 0", 1, neg, 0, "2^29") ||
        expect_arg_error("fe > 2^29", 1, big, 0, "2^29") || expect_arg_error("le > 2^29", 1, bigle, 0, "2^29") || expect_arg_error("rs < 0", 1, negrs, 0, "2^29") ||
        expect_arg_error("beyond int32", 1, huge, 0, "2^29") || expect_arg_error("fs == le", 1, le_eq, 0, "fs < le") || expect_arg_error("rs == fe", 1, rs_eq, 0, "fs < le") ||
        expect_arg_error("fe <= fs", 1, fe_le, 0, "fs < le"))
        return 1;
    {   // null arrays, no room for the table; the largest scheme compiles
        char msg[256] = "";
        int32_t small[6];
        const int64_t a1[1] = {10}, b1[1] = {20}, c1[1] = {80}, d1[1] = {100};
        if (tcmi_amplicon_reads_compile(1, a1, nullptr, c1, d1, 0, small, 6, msg, sizeof msg) != TCMI_E_ARG || !std::strstr(msg, "null")) return fail("null array", 0, 0, 0, 0);
        if (tcmi_amplicon_reads_compile(1, a1, b1, c1, d1, 0, small, 5, msg, sizeof msg) != TCMI_E_ARG || !std::strstr(msg, "room")) return fail("no room", 0, 0, 0, 0);
        if (tcmi_amplicon_reads_compile(1, a1, b1, c1, d1, 0, nullptr, 6, msg, sizeof msg) != TCMI_E_ARG) return fail("no table", 0, 0, 0, 0);
        if (tcmi_amplicon_reads_compile(1, a1, b1, c1, d1, 0, small, 6, nullptr, 0) != TCMI_OK || small[0] != 10 || small[1] != 100) return fail("n = 1 exported", small[0], small[1], 0, 0);
        const int32_t n = TCMI_AR_MAX_N;
        std::vector<int64_t> v[4];
        for (int32_t i = 0; i < n; ++i) { v[0].push_back(300 * (int64_t)(n - 1 - i)); v[1].push_back(v[0].back() + 20); v[2].push_back(v[0].back() + 350); v[3].push_back(v[0].back() + 400); }
        std::vector<int32_t> table((size_t)TCMI_AR_WORDS * (size_t)n);
        if (tcmi_amplicon_reads_compile(n, v[0].data(), v[1].data(), v[2].data(), v[3].data(), 5, table.data(), (int64_t)table.size(), msg, sizeof msg) != TCMI_OK) return fail(msg, n, 0, 0, 0);
        const tcmi_ar_table t = tcmi_ar_view(table.data(), n);
        bool full = false;
        // (given in descending order: sorted position k is amplicon n - 1 - k, [300 k, 300 k + 400): neighbours overlap by 100 columns)
        if (tcmi_ar_lookup(t, 300 * 7 + 105, 300 * 7 + 290, &full) != n - 1 - 7 || full) return fail("largest scheme", 0, 0, 0, 0);
        if (tcmi_ar_lookup(t, 300 * 7 + 5, 300 * 7 + 399, &full) != n - 1 - 7 || !full) return fail("largest scheme, full length", 0, 0, 0, 0);
        if (tcmi_ar_lookup(t, 300 * 7 + 5, 300 * 7 + 90, &full) != TCMI_AR_AMBIGUOUS) return fail("largest scheme, ambiguous", 0, 0, 0, 0);
        ++schemes;
    }
    std::printf("ok %d %lld\n", schemes, lookups);
    return 0;
}
