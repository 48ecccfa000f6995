// primer_table.cpp — HOST, GPU-free: the primer table of tcmi_ctx_set_primers compiled for the kernels (primer_table.h).
//
// The rule is a maximum (minimum) over the primers whose trigger interval holds a read's first (last) column.  The kernels do not want
// to visit every primer per read, so the trigger intervals are cut at each other's borders into disjoint pieces, each with the extreme
// value of the primers that cover it: one sweep over the sorted borders with a heap of the open intervals.  Overlapping, nested and
// alternative primers resolve here, once; a read then costs one binary search per list.
#include "primer_table.h"

#include <algorithm>
#include <cstdio>
#include <queue>

#include "../../include/tcmi.h"

namespace {

struct Trigger {
    int32_t lo, hi, val;            // reads whose column lies in [lo, hi) take val; the larger val wins
};

// disjoint pieces of the triggers' union, each with the largest val of the triggers that cover it (sign: values are stored as sign * val)
void sweep(std::vector<Trigger> &tr, int32_t sign, std::vector<tcmi_pseg> &out)
{
    out.clear();
    std::sort(tr.begin(), tr.end(), [](const Trigger &x, const Trigger &y) { return x.lo < y.lo; });
    std::vector<int32_t> cut;
    cut.reserve(tr.size() * 2);
    for (const Trigger &t : tr) { cut.push_back(t.lo); cut.push_back(t.hi); }
    std::sort(cut.begin(), cut.end());
    cut.erase(std::unique(cut.begin(), cut.end()), cut.end());
    auto lower = [](const Trigger &x, const Trigger &y) { return x.val < y.val; };
    std::priority_queue<Trigger, std::vector<Trigger>, decltype(lower)> open(lower);
    size_t next = 0;
    for (size_t k = 0; k + 1 < cut.size(); ++k) {
        const int32_t a = cut[k], b = cut[k + 1];
        while (next < tr.size() && tr[next].lo <= a) open.push(tr[next++]);
        while (!open.empty() && open.top().hi <= a) open.pop();       // (a trigger that is open at a border covers the piece up to the next one)
        if (open.empty()) continue;
        const int32_t v = sign * open.top().val;
        if (!out.empty() && out.back().b == a && out.back().v == v) out.back().b = b;
        else out.push_back({a, b, v});
    }
}

} // namespace

int tcmi_primers_build(int32_t n, const int64_t *start, const int64_t *end, const int32_t *reverse, int32_t slack, std::vector<tcmi_pseg> &head,
                       std::vector<tcmi_pseg> &tail, char *msg, size_t msg_cap)
{
    auto fail = [&](const char *fmt, long long x, long long y, long long z) {
        if (msg && msg_cap) std::snprintf(msg, msg_cap, fmt, x, y, z);
        return -1;
    };
    head.clear(); tail.clear();
    if (n < 0 || n > TCMI_PRIMERS_MAX) return fail("%lld primers: a table holds 0..%lld", n, TCMI_PRIMERS_MAX, 0);
    if (slack < 0 || slack > TCMI_PRIMER_SLACK_MAX) return fail("primer slack %lld is outside 0..%lld", slack, TCMI_PRIMER_SLACK_MAX, 0);
    if (n > 0 && (!start || !end || !reverse)) return fail("null primer arrays", 0, 0, 0);
    std::vector<Trigger> hd, tl;
    for (int32_t i = 0; i < n; ++i) {
        if (start[i] < 0 || end[i] <= start[i]) return fail("primer %lld: [%lld, %lld) is not an interval on the axis", i, (long long)start[i], (long long)end[i]);
        if (end[i] >= TCMI_PRIMER_POS_MAX) return fail("primer %lld: [%lld, %lld) reaches 2^29 or beyond", i, (long long)start[i], (long long)end[i]);
        if (reverse[i] != 0 && reverse[i] != 1) return fail("primer %lld: strand %lld is neither 0 ('+') nor 1 ('-')", i, reverse[i], 0);
        const int32_t s = (int32_t)start[i], e = (int32_t)end[i];
        if (reverse[i] == 0) hd.push_back({s - slack, e, e});           // the largest end
        else tl.push_back({s, e + slack, -s});                          // the smallest start
    }
    sweep(hd, 1, head);
    sweep(tl, -1, tail);
    return 0;
}

int32_t tcmi_pseg_find(const tcmi_pseg *seg, int32_t n, int32_t x, int32_t none)
{
    int32_t lo = 0, hi = n;                                             // seg[lo - 1].a <= x < seg[hi].a
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (seg[mid].a <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo > 0 && x < seg[lo - 1].b ? seg[lo - 1].v : none;
}

// the exported form (tests, tools): segments as {a, b, v} triples, at most seg_cap per list (2 n - 1 always suffice)
extern "C" int tcmi_primers_compile(int32_t n, const int64_t *start, const int64_t *end, const int32_t *reverse, int32_t slack, int32_t seg_cap,
                                    int32_t *head, int32_t *n_head, int32_t *tail, int32_t *n_tail, char *msg, int64_t msg_cap)
{
    std::vector<tcmi_pseg> h, t;
    if (seg_cap < 0 || !n_head || !n_tail || (seg_cap > 0 && (!head || !tail))) {
        if (msg && msg_cap > 0) std::snprintf(msg, (size_t)msg_cap, "null argument");
        return TCMI_E_ARG;
    }
    if (tcmi_primers_build(n, start, end, reverse, slack, h, t, msg, msg_cap > 0 ? (size_t)msg_cap : 0)) return TCMI_E_ARG;
    *n_head = (int32_t)h.size(); *n_tail = (int32_t)t.size();
    if ((int64_t)h.size() > seg_cap || (int64_t)t.size() > seg_cap) {
        if (msg && msg_cap > 0) std::snprintf(msg, (size_t)msg_cap, "%zu head and %zu tail segments, room for %d each", h.size(), t.size(), (int)seg_cap);
        return TCMI_E_ARG;
    }
    for (size_t i = 0; i < h.size(); ++i) { head[3 * i] = h[i].a; head[3 * i + 1] = h[i].b; head[3 * i + 2] = h[i].v; }
    for (size_t i = 0; i < t.size(); ++i) { tail[3 * i] = t[i].a; tail[3 * i + 1] = t[i].b; tail[3 * i + 2] = t[i].v; }
    return TCMI_OK;
}
