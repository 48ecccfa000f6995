// huffman_table_main.cpp — csrc/huffman_rule.h in a program of its own (tests/test_huffman_rule.py builds and runs it, plain and under
// AddressSanitizer + UBSan): the rule that build_table (csrc/bgzf_device.h) builds a block's Huffman tables by, against a decoder that
// knows nothing of it — codes handed out as RFC 1951 §3.2.2 says, a slot decoded one bit at a time, entries from the RFC's own tables
// of base values and extra bits.  Three things are compared on every code that is not over-subscribed, at a given number of root bits:
//   the rule       tcmi_huff_limits, tcmi_huff_slot_length, tcmi_huff_key, tcmi_huff_key_index, tcmi_huff_entry, tcmi_huff_fits
//   the wave       the same steps as build_table takes them on 64 lanes, restated lane by lane (ballots of the length's bits, a lane's
//                  rank from the mask of its equals, the 16-entry table of counts, the scans over lanes 0 .. 15, the keys and
//                  their running maximum over the reversed slot indices)
//   the decoder    the naive one
// and on an over-subscribed code the verdict alone.  Usage: huffman_table_main -> "ok <codes> <over-subscribed> <slots>" on stdout.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../trueconsense_amd/csrc/huffman_rule.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n)            // 0 .. n - 1
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 11) % n);
}

[[noreturn]] void fail(const char *what, const std::vector<uint8_t> &lens, int root, long a, long b, long c)
{
    std::printf("FAILED %s (root %d; %ld %ld %ld) lens:", what, root, a, b, c);
    for (size_t i = 0; i < lens.size(); ++i) if (lens[i]) std::printf(" %zu:%d", i, lens[i]);
    std::printf("\n");
    std::exit(1);
}

uint32_t reverse_bits(uint32_t v, int n)
{
    uint32_t r = 0;
    for (int k = 0; k < n; ++k) r |= ((v >> k) & 1u) << (n - 1 - k);
    return r;
}

// ---- the decoder that knows nothing of the rule --------------------------------------------------------------------------------------------
const int LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
const int LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
const int DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
const int DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

uint32_t naive_entry(int kind, int sym, int nbits)
{
    const uint32_t nb = (uint32_t)nbits;
    if (kind == TCMI_HUFF_CODELEN) return nb | ((uint32_t)sym << 16);
    if (kind == TCMI_HUFF_LITLEN) {
        if (sym < 256) return nb | (1u << 8) | ((uint32_t)sym << 16);
        if (sym == 256) return nb | (1u << 10);
        if (sym > 285) return 0;
        const uint32_t eb = (uint32_t)LEN_EXTRA[sym - 257], base = (uint32_t)LEN_BASE[sym - 257];
        return nb | ((nb + eb) << 11) | (1u << 9) | (eb << 16) | (base << 20);
    }
    if (sym > 29) return 0;
    return nb | ((uint32_t)DIST_EXTRA[sym] << 4) | (1u << 9) | ((uint32_t)DIST_BASE[sym] << 16);
}

struct Naive {
    bool over;
    std::vector<uint32_t> code;         // per symbol, RFC 1951 §3.2.2
    std::vector<int> sorted;            // symbols by (length, symbol)
    uint32_t cnt[16];
};

Naive naive_codes(const std::vector<uint8_t> &lens)
{
    Naive v;
    for (int k = 0; k < 16; ++k) v.cnt[k] = 0;
    for (uint8_t l : lens) if (l) ++v.cnt[l];
    long left = 1;
    v.over = false;
    for (int len = 1; len <= 15; ++len) {
        left = left * 2 - (long)v.cnt[len];
        if (left < 0) { v.over = true; break; }
    }
    uint32_t next[16], code = 0;
    next[0] = 0;
    for (int bits = 1; bits <= 15; ++bits) { code = (code + (bits > 1 ? v.cnt[bits - 1] : 0u)) << 1; next[bits] = code; }
    v.code.assign(lens.size(), 0);
    for (size_t s = 0; s < lens.size(); ++s) if (lens[s]) v.code[s] = next[lens[s]]++;
    for (int len = 1; len <= 15; ++len)
        for (size_t s = 0; s < lens.size(); ++s) if (lens[s] == len) v.sorted.push_back((int)s);
    return v;
}

// the symbol whose code the slot's bits begin with, bit by bit (first stream bit = bit 0 of the slot): -> length, or 0
int naive_slot(const std::vector<uint8_t> &lens, const Naive &v, uint32_t slot, int root, int *sym)
{
    uint32_t code = 0;
    for (int len = 1; len <= root; ++len) {
        code = (code << 1) | ((slot >> (len - 1)) & 1u);
        for (size_t s = 0; s < lens.size(); ++s) if (lens[s] == len && v.code[s] == code) { *sym = (int)s; return len; }
    }
    return 0;
}

// ---- build_table's steps, lane by lane -----------------------------------------------------------------------------------------------------
struct Wave {
    bool ok;
    uint32_t cnt[16], rs[2];
    std::vector<int> sym;
    std::vector<uint32_t> ent, tab;
};

Wave wave_build(const std::vector<uint8_t> &lens, int root, int kind)
{
    const int n = (int)lens.size(), groups = (n + 63) / 64;
    Wave w;
    uint32_t ol[16] = {0};
    std::vector<uint32_t> place((size_t)groups * 64);
    for (int g = 0; g < groups; ++g) {
        uint32_t l[64], before[64], tot[64];
        for (int lane = 0; lane < 64; ++lane) l[lane] = g * 64 + lane < n ? lens[(size_t)g * 64 + lane] & 15u : 0u;
        uint64_t ballot[4] = {0, 0, 0, 0};
        for (int k = 0; k < 4; ++k) for (int lane = 0; lane < 64; ++lane) ballot[k] |= (uint64_t)((l[lane] >> k) & 1u) << lane;
        for (int lane = 0; lane < 64; ++lane) {
            uint64_t eq = ~0ull;
            for (int k = 0; k < 4; ++k) eq &= ((l[lane] >> k) & 1u) ? ballot[k] : ~ballot[k];
            const uint32_t below = (uint32_t)__builtin_popcountll(eq & ((1ull << lane) - 1ull));
            before[lane] = ol[l[lane]];
            tot[lane] = (uint32_t)__builtin_popcountll(eq);
            place[(size_t)g * 64 + lane] = before[lane] + below;
        }
        for (int lane = 0; lane < 64; ++lane) ol[l[lane]] = before[lane] + tot[lane];      // (lanes of one length write one value)
    }
    uint32_t c[16], term[16], o_incl[16], lim15[16];
    for (int lane = 0; lane < 16; ++lane) { c[lane] = lane >= 1 ? ol[lane] : 0u; term[lane] = tcmi_huff_term(c[lane], lane); }
    for (int lane = 0; lane < 16; ++lane) { o_incl[lane] = (lane ? o_incl[lane - 1] : 0u) + c[lane]; lim15[lane] = (lane ? lim15[lane - 1] : 0u) + term[lane]; }
    for (int lane = 0; lane < 16; ++lane) { w.cnt[lane] = c[lane]; ol[lane] = o_incl[lane] - c[lane]; }
    w.rs[0] = lim15[root] >> (14 - root);
    w.rs[1] = o_incl[root];
    w.ok = tcmi_huff_fits(lim15[15]);
    if (!w.ok) return w;
    w.sym.assign(o_incl[15], -1);
    w.ent.assign(o_incl[15], 0xDEADBEEFu);
    for (int s = 0; s < n; ++s) {
        if (!lens[s]) continue;
        const uint32_t at = ol[lens[s]] + place[s];
        if (at >= o_incl[15] || w.sym[at] != -1) fail("wave: a symbol's place", lens, root, s, at, o_incl[15]);
        w.sym[at] = s;
        w.ent[at] = tcmi_huff_entry(kind, s, lens[s]);
    }
    // the keys where their lengths' slots begin, in reversed-index order; their running maximum; every slot by its key
    std::vector<uint32_t> keys((size_t)1 << root, 0);
    for (int lane = 1; lane <= root + 1; ++lane) {
        const uint32_t start = tcmi_huff_key_start(lim15[lane] - term[lane], root);
        if ((c[lane] != 0 || lane == root + 1) && start < (1u << root)) {
            if (keys[start] != 0) fail("wave: two keys on one slot", lens, root, lane, start, keys[start]);
            keys[start] = tcmi_huff_key(lane, o_incl[lane] - c[lane], lim15[lane] - term[lane], root);
        }
    }
    if (keys[0] == 0) fail("wave: no key at 0", lens, root, 0, 0, 0);
    w.tab.assign((size_t)1 << root, 0);
    uint32_t k = 0;
    for (uint32_t r = 0; r < (1u << root); ++r) {
        k = std::max(k, keys[r]);
        if (!tcmi_huff_key_filled(k, root)) {
            if (tcmi_huff_key_index(k, r) != 0) fail("wave: an empty slot's index", lens, root, r, k, 0);
            continue;
        }
        const uint32_t at = tcmi_huff_key_index(k, r);
        if (at >= w.ent.size()) fail("wave: a slot's index", lens, root, r, at, (long)w.ent.size());
        w.tab[reverse_bits(r, root)] = w.ent[at];
    }
    return w;
}

long n_codes = 0, n_over = 0, n_slots = 0;

void check(const std::vector<uint8_t> &lens, int root, int kind)
{
    const Naive v = naive_codes(lens);
    uint32_t lim15[16], off[16];
    tcmi_huff_limits(v.cnt, lim15, off);
    const Wave w = wave_build(lens, root, kind);
    if (tcmi_huff_fits(lim15[15]) == v.over) fail("the verdict of the rule", lens, root, lim15[15], v.over, 0);
    if (w.ok == v.over) fail("the verdict of the wave", lens, root, w.ok, v.over, 0);
    if (v.over) { ++n_over; return; }
    ++n_codes;
    for (int len = 1; len <= 15; ++len) {
        if (lim15[len] < lim15[len - 1]) fail("limits decrease", lens, root, len, lim15[len], lim15[len - 1]);
        if (w.cnt[len] != v.cnt[len]) fail("wave: cnt", lens, root, len, w.cnt[len], v.cnt[len]);
    }
    if (w.cnt[0] != 0) fail("wave: cnt[0]", lens, root, w.cnt[0], 0, 0);
    // rs as build_long wants it: the first code longer than root bits, and how many sorted symbols lie in front of it
    uint32_t f = 0, o = 0;
    for (int len = 1; len <= root; ++len) { o += v.cnt[len]; f = (f + v.cnt[len]) << 1; }
    if (w.rs[0] != f || w.rs[1] != o) fail("wave: rs", lens, root, w.rs[0], f, o);
    if (w.sym != v.sorted) fail("wave: the sorted symbols", lens, root, (long)w.sym.size(), (long)v.sorted.size(), 0);
    for (size_t k = 0; k < v.sorted.size(); ++k) {
        const int s = v.sorted[k];
        if (w.ent[k] != naive_entry(kind, s, lens[(size_t)s])) fail("an entry", lens, root, s, w.ent[k], naive_entry(kind, s, lens[(size_t)s]));
    }
    for (uint32_t i = 0; i < (1u << root); ++i) {
        int sym = -1;
        const int len = naive_slot(lens, v, i, root, &sym);
        const uint32_t r = reverse_bits(i, root);
        const int L = tcmi_huff_slot_length(r, lim15, root);
        uint32_t got = 0;
        if (L <= root) {
            const uint32_t at = tcmi_huff_key_index(tcmi_huff_key(L, off[L], lim15[L - 1], root), r);
            if (at >= v.sorted.size()) fail("the rule: a slot's index", lens, root, i, at, L);
            if (len != L || v.sorted[at] != sym) fail("the rule: a slot's symbol", lens, root, i, L, len);
            got = tcmi_huff_entry(kind, v.sorted[at], L);
        } else if (len != 0) fail("the rule: a slot the decoder fills", lens, root, i, L, len);
        const uint32_t want = len ? naive_entry(kind, sym, len) : 0u;
        if (got != want) fail("the rule: a slot's entry", lens, root, i, got, want);
        if (w.tab[i] != want) fail("wave: a slot's entry", lens, root, i, w.tab[i], want);
        ++n_slots;
    }
}

// a complete code of `leaves` codes of at most `maxlen` bits: split a random leaf until there are enough
std::vector<uint8_t> random_depths(int leaves, int maxlen)
{
    std::vector<uint8_t> d;
    if (leaves == 1) { d.push_back(1); return d; }      // (one code of one bit: incomplete by nature)
    d.push_back(1); d.push_back(1);
    int stuck = 0;
    while ((int)d.size() < leaves && stuck < 1000) {
        const size_t k = rnd((uint32_t)d.size());
        if (d[k] >= maxlen) { ++stuck; continue; }
        ++d[k];
        d.push_back(d[k]);
    }
    return d;
}

void random_code(int alphabet, int maxlen, int root, int kind, bool incomplete)
{
    const int used = 1 + (int)rnd((uint32_t)alphabet);
    std::vector<uint8_t> d = random_depths(used, maxlen), lens((size_t)alphabet, 0);
    if (incomplete) for (uint32_t k = 1 + rnd(3); k > 0 && d.size() > 1; --k) d.erase(d.begin() + rnd((uint32_t)d.size()));
    std::vector<int> syms((size_t)alphabet);
    for (int s = 0; s < alphabet; ++s) syms[(size_t)s] = s;
    for (int s = alphabet - 1; s > 0; --s) std::swap(syms[(size_t)s], syms[rnd((uint32_t)s + 1u)]);
    for (size_t k = 0; k < d.size(); ++k) lens[(size_t)syms[k]] = d[k];
    check(lens, root, kind);
}

} // namespace

int main()
{
    // every length vector of 6 symbols with lengths 0 .. 4, three root bits
    for (int v = 0; v < 15625; ++v) {
        std::vector<uint8_t> lens(6);
        for (int k = 0, x = v; k < 6; ++k, x /= 5) lens[(size_t)k] = (uint8_t)(x % 5);
        check(lens, 3, TCMI_HUFF_CODELEN);
    }
    if (n_codes + n_over != 15625 || n_over < 1000 || n_codes < 1000) { std::printf("FAILED the sweep's counts %ld %ld\n", n_codes, n_over); return 1; }
    // random complete and incomplete codes
    for (int root = 7; root <= 9; ++root) {
        for (int k = 0; k < 700; ++k) random_code(286, 15, root, TCMI_HUFF_LITLEN, (k & 1) != 0);
        for (int k = 0; k < 300; ++k) random_code(288, 15, root, TCMI_HUFF_LITLEN, (k & 1) != 0);     // (a fixed block's alphabet: 286, 287 name nothing)
        for (int k = 0; k < 300; ++k) random_code(30, 15, root, TCMI_HUFF_DIST, (k & 1) != 0);
        for (int k = 0; k < 100; ++k) random_code(32, 15, root, TCMI_HUFF_DIST, (k & 1) != 0);
        for (int k = 0; k < 300; ++k) random_code(19, 7, root, TCMI_HUFF_CODELEN, (k & 1) != 0);
    }
    // the edges
    for (int root = 7; root <= 9; ++root) {
        for (int len = 1; len <= 15; ++len) {                       // a single code, of every length, on symbols at the groups' edges
            for (int s : {0, 63, 64, 127, 128, 255, 256, 257, 285}) {
                std::vector<uint8_t> lens(286, 0);
                lens[(size_t)s] = (uint8_t)len;
                check(lens, root, TCMI_HUFF_LITLEN);
            }
            std::vector<uint8_t> one(30, 0);
            one[(size_t)(len % 30)] = (uint8_t)len;
            check(one, root, TCMI_HUFF_DIST);
        }
        for (int extra = 0; extra <= 1; ++extra) {                  // all lengths root / root + 1: complete (2^len codes) and short of it
            for (int count : {1 << (root + extra), (1 << (root + extra)) - 1, 286, 64, 65}) {
                if (count > 288) continue;
                std::vector<uint8_t> lens(288, 0);
                for (int s = 0; s < count; ++s) lens[(size_t)s] = (uint8_t)(root + extra);
                check(lens, root, TCMI_HUFF_LITLEN);
            }
        }
        {   // the fixed code of RFC 1951 §3.2.6
            std::vector<uint8_t> lens(288), d(32, 5);
            for (int s = 0; s < 288; ++s) lens[(size_t)s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
            check(lens, root, TCMI_HUFF_LITLEN);
            check(d, root, TCMI_HUFF_DIST);
        }
        {   // all 15 lengths populated: 1, 2, .., 14 once and 15 twice is complete; without the last it is not
            std::vector<uint8_t> lens(286, 0);
            for (int len = 1; len <= 15; ++len) lens[(size_t)(len * 17)] = (uint8_t)len;
            check(lens, root, TCMI_HUFF_LITLEN);
            lens[3] = 15;
            check(lens, root, TCMI_HUFF_LITLEN);
            for (int s = 100; s < 286; ++s) if (!lens[(size_t)s] && rnd(2)) lens[(size_t)s] = 15;      // (.. and over-subscribed)
            check(lens, root, TCMI_HUFF_LITLEN);
        }
        {   // no code at all
            std::vector<uint8_t> lens(286, 0);
            check(lens, root, TCMI_HUFF_LITLEN);
        }
    }
    // over-subscribed vectors: the verdict alone
    const long over_before = n_over;
    for (int k = 0; k < 3000; ++k) {
        const int alphabet = k % 3 == 0 ? 286 : k % 3 == 1 ? 30 : 19, maxlen = alphabet == 19 ? 7 : 15;
        std::vector<uint8_t> lens((size_t)alphabet);
        if (k & 1) {                                                // one code too many
            std::vector<uint8_t> d = random_depths(2 + (int)rnd((uint32_t)alphabet - 2u), maxlen);
            std::fill(lens.begin(), lens.end(), 0);
            for (size_t j = 0; j < d.size(); ++j) lens[j] = d[j];
            lens[d.size()] = (uint8_t)(1 + rnd((uint32_t)maxlen));   // (d.size() < alphabet)
        } else for (auto &l : lens) l = (uint8_t)rnd((uint32_t)maxlen + 1u);
        check(lens, alphabet == 19 ? 7 : alphabet == 30 ? 8 : 9, alphabet == 19 ? TCMI_HUFF_CODELEN : alphabet == 30 ? TCMI_HUFF_DIST : TCMI_HUFF_LITLEN);
    }
    if (n_over - over_before < 2000) { std::printf("FAILED too few over-subscribed vectors %ld\n", n_over - over_before); return 1; }
    std::printf("ok %ld %ld %ld\n", n_codes, n_over, n_slots);
    return 0;
}
