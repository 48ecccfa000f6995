// mate_rule.h — the rule of --mate-overlap (include/tcmi.h: tcmi_ctx_set_mate_overlap), GPU-free: which kept records are eligible for the
// join, the hash of a record's key, when two records of one key are a pair, which of them loses the shared columns and how many.  It
// includes no HIP header and compiles with any C++ compiler, so the kernels (mate_join.hip) and host programs that check them
// (tests/mate_rule_main.cpp) share one text.  All arithmetic is integer.
//
// The key of an eligible record: (read name without its NUL, refID, min(pos, next_pos), max(pos, next_pos)).  The eligible records of one
// key are a group; a group of exactly two records a, b with a.next_pos == b.pos, b.next_pos == a.pos, one of them FLAG 0x40 and the other
// 0x80, is a pair; every other group stays unjoined, and the records of a group of three or more are ambiguous.  Strand plays no part.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define TCMI_MATE_HD __attribute__((host)) __attribute__((device))
#else
#define TCMI_MATE_HD
#endif

// the fixed fields of a record that the rule reads (SAM spec §4.2)
struct tcmi_mate_fields {
    uint32_t flag;
    int32_t tid, pos, next_tid, next_pos;
};

// paired (0x1) and properly so (0x2), the mate mapped (no 0x8), a primary line (no 0x100, no 0x800), exactly one of first / last
// (0x40 / 0x80), the mate on the same reference at a position that is known
TCMI_MATE_HD inline bool tcmi_mate_eligible(const tcmi_mate_fields &r)
{
    const uint32_t f = r.flag;
    return (f & 0x3u) == 0x3u && (f & (0x8u | 0x100u | 0x800u)) == 0u && (((f >> 6) ^ (f >> 7)) & 1u) != 0u && r.next_tid == r.tid && r.next_pos >= 0;
}

TCMI_MATE_HD inline int32_t tcmi_mate_lo(const tcmi_mate_fields &r) { return r.pos < r.next_pos ? r.pos : r.next_pos; }
TCMI_MATE_HD inline int32_t tcmi_mate_hi(const tcmi_mate_fields &r) { return r.pos < r.next_pos ? r.next_pos : r.pos; }

// The key's hash: 64-bit FNV-1a over the name's bytes, then over the twelve bytes of refID, min(pos, next_pos) and max(pos, next_pos),
// each little-endian.  The join's table takes its slot from the low bits and its 32-bit tag from the high word.
constexpr uint64_t TCMI_MATE_FNV_BASIS = 0xCBF29CE484222325ull, TCMI_MATE_FNV_PRIME = 0x100000001B3ull;
TCMI_MATE_HD inline uint64_t tcmi_mate_hash_byte(uint64_t h, uint32_t byte) { return (h ^ (uint64_t)(byte & 0xFFu)) * TCMI_MATE_FNV_PRIME; }
// (four bytes of a little-endian word, lowest first; n <= 4 of them)
TCMI_MATE_HD inline uint64_t tcmi_mate_hash_word(uint64_t h, uint32_t w, int n = 4)
{
    for (int k = 0; k < n; ++k) h = tcmi_mate_hash_byte(h, w >> (8 * k));
    return h;
}
// h: the hash of the name's bytes so far -> the key's hash
TCMI_MATE_HD inline uint64_t tcmi_mate_hash_finish(uint64_t h, const tcmi_mate_fields &r)
{
    h = tcmi_mate_hash_word(h, (uint32_t)r.tid);
    h = tcmi_mate_hash_word(h, (uint32_t)tcmi_mate_lo(r));
    return tcmi_mate_hash_word(h, (uint32_t)tcmi_mate_hi(r));
}
TCMI_MATE_HD inline uint64_t tcmi_mate_hash(const uint8_t *name, int n_name, const tcmi_mate_fields &r)
{
    uint64_t h = TCMI_MATE_FNV_BASIS;
    for (int k = 0; k < n_name; ++k) h = tcmi_mate_hash_byte(h, name[k]);
    return tcmi_mate_hash_finish(h, r);
}
TCMI_MATE_HD inline uint32_t tcmi_mate_tag(uint64_t h) { return (uint32_t)(h >> 32); }

// the integers of two eligible records' keys are equal (the names are compared by the caller)
TCMI_MATE_HD inline bool tcmi_mate_same_ints(const tcmi_mate_fields &a, const tcmi_mate_fields &b)
{
    return a.tid == b.tid && tcmi_mate_lo(a) == tcmi_mate_lo(b) && tcmi_mate_hi(a) == tcmi_mate_hi(b);
}

// the names of two keys, as the kernels read them: whole dwords — get_a(k), get_b(k): the little-endian word at byte k of either name;
// what its bytes behind the name hold plays no part —, then the tail of one to three bytes under a mask
template <class GetA, class GetB> TCMI_MATE_HD inline bool tcmi_mate_same_name(uint32_t n_a, uint32_t n_b, GetA get_a, GetB get_b)
{
    if (n_a != n_b) return false;
    uint32_t k = 0;
    for (; k + 4 <= n_a; k += 4)
        if (get_a(k) != get_b(k)) return false;
    if (k < n_a) {
        const uint32_t mask = (1u << (8 * (n_a - k))) - 1u;
        if ((get_a(k) ^ get_b(k)) & mask) return false;
    }
    return true;
}

// a group of exactly the two eligible records a, b: a pair?
TCMI_MATE_HD inline bool tcmi_mate_pair(const tcmi_mate_fields &a, const tcmi_mate_fields &b)
{
    return a.next_pos == b.pos && b.next_pos == a.pos && ((a.flag & 0x40u) != 0u) != ((b.flag & 0x40u) != 0u);
}

// of the pair a, b: does a lose?  The record with the larger pos; at equal pos the one with 0x80.
TCMI_MATE_HD inline bool tcmi_mate_loses(const tcmi_mate_fields &a, const tcmi_mate_fields &b)
{
    return a.pos > b.pos || (a.pos == b.pos && (a.flag & 0x80u) != 0u);
}

// [p, q]: a record's first and last column.  The loser's first `clip` columns are the winner's too: p_loser >= p_winner, so the shared
// columns are a prefix of the loser.
TCMI_MATE_HD inline uint32_t tcmi_mate_clip(int64_t p_loser, int64_t q_loser, int64_t q_winner)
{
    const int64_t c = (q_winner < q_loser ? q_winner : q_loser) - p_loser + 1;
    return c > 0 ? (uint32_t)c : 0u;
}
