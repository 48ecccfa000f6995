// dedup_rule.h — the rule of --dedup (include/tcmi.h: tcmi_ctx_set_dedup), GPU-free: a record's end and score, a template's key, its
// hash, and which of two templates of one key is the better.  It includes no HIP header and compiles with any C++ compiler, so the kernels
// (dedup.hip) and a host program that checks them (tests/dedup_rule_main.cpp) share one text.  All arithmetic is integer.
//
// Examined: the kept records without FLAG 0x100 / 0x800.  A record's end is (refID, u5, rev): rev FLAG 0x10, u5 its unclipped 5'
// coordinate on its own reference — forward pos - (leading S + H), reverse pos + span - 1 + (trailing S + H).  Its score: the sum of its
// QUAL bytes >= 15, saturating at 2^32 - 1 (a QUAL of 0xFF bytes scores 0).  A pair of the mate join (mate_rule.h) is one template, led
// by its record of the lower index, scored by the saturating sum of both; every other examined record is a fragment that leads itself.
// Key of a fragment (F, refID, u5, rev), of a pair (P, refID, end_a, end_b) with the ends ordered by (u5, rev).  Of the templates of one
// key the highest score wins, at equal score the lowest leader; all records of every other template are duplicates.
#pragma once
#include <stdint.h>

#include "mate_rule.h"

#define TCMI_DUP_HD TCMI_MATE_HD

constexpr uint32_t TCMI_DUP_MIN_QUAL = 15;          // Picard's SUM_OF_BASE_QUALITIES counts a base from here on
constexpr uint32_t TCMI_DUP_SCORE_MOST = 0xFFFFFFFFu;

// examined: a kept record that is neither secondary nor supplementary (the caller has asked kept_span)
TCMI_DUP_HD inline bool tcmi_dup_examined(uint32_t flag) { return (flag & (0x100u | 0x800u)) == 0u; }

// ---- the end: one walk over the CIGAR words (cg[k] = len << 4 | op, as in BAM; get(k) reads word k) --------------------------------
// -> u5 (64 bits wide here; tcmi_dup_end_make narrows it).  S is 4, H is 5; the reference span is the sum of M, D, N, =, X.
template <class Get> TCMI_DUP_HD inline int64_t tcmi_dup_u5(int32_t pos, bool rev, uint32_t n_cigar, Get get)
{
    int64_t lead = 0, trail = 0, span = 0;
    bool inner = false;                             // an op that is no clip has been seen
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t c = get(k), op = c & 0xFu, len = c >> 4;
        if (op == 4u || op == 5u) {
            if (inner) trail += len; else lead += len;
        } else {
            inner = true;
            trail = 0;                              // (clips in the middle of a CIGAR are not trailing ones)
            if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) span += len;
        }
    }
    return rev ? (int64_t)pos + span - 1 + trail : (int64_t)pos - lead;
}

// ---- the score: QUAL four bytes at a time (a little-endian word, n <= 4 of its bytes count, lowest first) ---------------------------
TCMI_DUP_HD inline uint32_t tcmi_dup_score_word(uint32_t w, int n = 4)
{
    uint32_t s = 0;
    for (int k = 0; k < n; ++k) {
        const uint32_t q = (w >> (8 * k)) & 0xFFu;
        if (q >= TCMI_DUP_MIN_QUAL && q != 0xFFu) s += q;
    }
    return s;
}
TCMI_DUP_HD inline uint32_t tcmi_dup_score_add(uint32_t a, uint32_t b)
{
    const uint64_t s = (uint64_t)a + b;
    return s > TCMI_DUP_SCORE_MOST ? TCMI_DUP_SCORE_MOST : (uint32_t)s;
}
TCMI_DUP_HD inline uint32_t tcmi_dup_score(const uint8_t *qual, int64_t l_seq)
{
    uint32_t s = 0;
    for (int64_t k = 0; k < l_seq; ++k) s = tcmi_dup_score_add(s, tcmi_dup_score_word(qual[k], 1));
    return s;
}

// ---- what the kernels keep of a record: ends[i], sixteen bytes ------------------------------------------------------------------------
// meta: 0 for a record that is not examined, else refID << 2 | rev << 1 | 1 (a kept record's refID is 0 or an index into the contig
// layout: far below 2^30).  u5 narrowed to 32 bits by saturation: a kept record's pos and span are below 2^30, only clips of a forged
// length get there.  span: the record's reference span, what a duplicate's clip is raised to — kept here so that the verdicts are
// written without going back to the record.
struct tcmi_dup_end {
    int32_t u5;
    uint32_t score, meta, span;
};
TCMI_DUP_HD inline tcmi_dup_end tcmi_dup_end_make(int32_t tid, int64_t u5, bool rev, uint32_t score, uint32_t span)
{
    tcmi_dup_end e;
    e.u5 = u5 > 0x7FFFFFFFll ? 0x7FFFFFFF : u5 < -0x7FFFFFFFll - 1 ? (int32_t)(-0x7FFFFFFFll - 1) : (int32_t)u5;
    e.score = score;
    e.span = span;
    e.meta = ((uint32_t)tid << 2) | (rev ? 2u : 0u) | 1u;
    return e;
}
TCMI_DUP_HD inline bool tcmi_dup_end_examined(const tcmi_dup_end &e) { return (e.meta & 1u) != 0u; }
TCMI_DUP_HD inline uint32_t tcmi_dup_end_rev(const tcmi_dup_end &e) { return (e.meta >> 1) & 1u; }
TCMI_DUP_HD inline uint32_t tcmi_dup_end_tid(const tcmi_dup_end &e) { return e.meta >> 2; }

// ---- the key: three words --------------------------------------------------------------------------------------------------------------
// w[0] = refID << 3 | pair << 2 | rev_a << 1 | rev_b, w[1] = u5_a, w[2] = u5_b (a fragment: rev_b and u5_b are 0; bit 2 keeps it
// apart from every pair).  Which end is read 1 plays no part: a is the end that is lower by (u5, rev).
struct tcmi_dup_key { uint32_t w[3]; };
TCMI_DUP_HD inline bool tcmi_dup_key_same(const tcmi_dup_key &a, const tcmi_dup_key &b) { return a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2]; }
TCMI_DUP_HD inline tcmi_dup_key tcmi_dup_key_fragment(const tcmi_dup_end &e)
{
    tcmi_dup_key k;
    k.w[0] = (tcmi_dup_end_tid(e) << 3) | (tcmi_dup_end_rev(e) << 1);
    k.w[1] = (uint32_t)e.u5;
    k.w[2] = 0u;
    return k;
}
// (the two records of a pair lie on one reference: the join's key holds refID)
TCMI_DUP_HD inline tcmi_dup_key tcmi_dup_key_pair(const tcmi_dup_end &x, const tcmi_dup_end &y)
{
    const bool x_first = x.u5 < y.u5 || (x.u5 == y.u5 && tcmi_dup_end_rev(x) <= tcmi_dup_end_rev(y));
    const tcmi_dup_end &a = x_first ? x : y, &b = x_first ? y : x;
    tcmi_dup_key k;
    k.w[0] = (tcmi_dup_end_tid(a) << 3) | 4u | (tcmi_dup_end_rev(a) << 1) | tcmi_dup_end_rev(b);
    k.w[1] = (uint32_t)a.u5;
    k.w[2] = (uint32_t)b.u5;
    return k;
}
// 64-bit FNV-1a over the key's twelve bytes, each word little-endian; slot from the low bits, tag from the high word (tcmi_mate_tag)
TCMI_DUP_HD inline uint64_t tcmi_dup_hash(const tcmi_dup_key &k)
{
    uint64_t h = TCMI_MATE_FNV_BASIS;
    for (int i = 0; i < 3; ++i) h = tcmi_mate_hash_word(h, k.w[i]);
    return h;
}

// ---- the winner: one 64-bit word per template, the largest wins ------------------------------------------------------------------------
// score << 32 | (2^32 - 1 - leader): the higher score, at equal score the lower leader
TCMI_DUP_HD inline uint64_t tcmi_dup_rank(uint32_t score, uint32_t leader) { return ((uint64_t)score << 32) | (uint64_t)(0xFFFFFFFFu - leader); }
TCMI_DUP_HD inline uint32_t tcmi_dup_rank_leader(uint64_t rank) { return 0xFFFFFFFFu - (uint32_t)rank; }
TCMI_DUP_HD inline bool tcmi_dup_better(uint32_t score_a, uint32_t leader_a, uint32_t score_b, uint32_t leader_b)
{
    return tcmi_dup_rank(score_a, leader_a) > tcmi_dup_rank(score_b, leader_b);
}
