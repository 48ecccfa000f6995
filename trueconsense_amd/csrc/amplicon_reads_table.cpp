// amplicon_reads_table.cpp — HOST, GPU-free: the scheme of tcmi_readset_amplicon_reads compiled for the kernel (amplicon_reads_rule.h
// has the layout and the lookup).  Sort by (a, index); then one pass that carries the largest and the second largest b of the prefix.
#include "amplicon_reads_rule.h"

#include <algorithm>
#include <cstdio>
#include <numeric>
#include <vector>

int tcmi_amplicon_reads_build(int64_t n, const int64_t *fs, const int64_t *le, const int64_t *rs, const int64_t *fe, int32_t slack, int32_t *table,
                              char *msg, size_t msg_cap)
{
    auto fail = [&](const char *fmt, long long x, long long y, long long z) {
        if (msg && msg_cap) std::snprintf(msg, msg_cap, fmt, x, y, z);
        return -1;
    };
    int64_t bad = -1;
    switch (tcmi_amplicon_reads_check(n, fs, le, rs, fe, slack, &bad)) {
    case 0: break;
    case 1: return fail("%lld amplicons: a scheme holds 1..%lld", (long long)n, TCMI_AR_MAX_N, 0);
    case 2: return fail("amplicon slack %lld is outside 0..%lld", slack, TCMI_AR_MAX_SLACK, 0);
    case 3: return fail("null amplicon arrays", 0, 0, 0);
    case 4: return fail("amplicon %lld: [%lld, %lld) has a coordinate outside 0..2^29", (long long)bad, (long long)fs[bad], (long long)fe[bad]);
    default:
        if (!msg || !msg_cap) return -1;
        std::snprintf(msg, msg_cap, "amplicon %lld: fs %lld, le %lld, rs %lld, fe %lld do not satisfy fs < le, rs < fe, fs < fe", (long long)bad,
                      (long long)fs[bad], (long long)le[bad], (long long)rs[bad], (long long)fe[bad]);
        return -1;
    }
    if (!table) return fail("no room for the table", 0, 0, 0);
    std::vector<int32_t> order((size_t)n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return fs[x] < fs[y]; });     // (a = fs - slack: the same order; stable: ties by index)
    int32_t *a = table, *bmax = table + n, *idx = table + 2 * n, *b2 = table + 3 * n, *t_le = table + 4 * n, *t_rs = table + 5 * n;
    int32_t best = TCMI_AR_NONE, second = TCMI_AR_NONE, who = -1;
    for (int64_t k = 0; k < n; ++k) {
        const int32_t i = order[(size_t)k];
        const int32_t b = (int32_t)fe[i] + slack;
        if (who < 0 || b > best) { second = best; best = b; who = i; }
        else if (b > second) second = b;                    // (b == best lands here: the second largest counts multiplicity)
        a[k] = (int32_t)fs[i] - slack;                      // (may be negative: no clamp at 0)
        bmax[k] = best; idx[k] = who; b2[k] = second;
    }
    for (int64_t i = 0; i < n; ++i) { t_le[i] = (int32_t)le[i]; t_rs[i] = (int32_t)rs[i]; }
    return 0;
}

extern "C" int tcmi_amplicon_reads_compile(int64_t n, const int64_t *fs, const int64_t *le, const int64_t *rs, const int64_t *fe, int32_t slack,
                                           int32_t *table, int64_t table_cap, char *msg, int64_t msg_cap)
{
    const size_t cap = msg_cap > 0 ? (size_t)msg_cap : 0;
    if (tcmi_amplicon_reads_check(n, fs, le, rs, fe, slack, nullptr) == 0 && (!table || table_cap < TCMI_AR_WORDS * n)) {
        if (msg && cap) std::snprintf(msg, cap, "the table of %lld amplicons takes %lld words, room for %lld", (long long)n, (long long)(TCMI_AR_WORDS * n), (long long)table_cap);
        return TCMI_E_ARG;
    }
    return tcmi_amplicon_reads_build(n, fs, le, rs, fe, slack, table, msg, cap) ? TCMI_E_ARG : TCMI_OK;
}
