// indel_rule.h — the rule of --indel-table (include/tcmi.h: tcmi_readset_indel_events), stated once for the kernels
// (indel_events.hip), the library's host code (indels_text.cpp) and host programs that check them (tests/indel_main.cpp): it includes no
// HIP header and compiles with any C++ compiler.  All arithmetic is integer.
//   what an event is      a kept record (pack_device.h: kept_span) with the walk of stream_walk.h yields at a queried column c
//                         INS  iff token_at(w, c, Q) has bit TCMI_I; its bases are the query nibbles of exactly the I ops that ins_after
//                              adds up, in CIGAR order (tcmi_ins_iter below; a query index at or beyond l_seq reads as nibble 15);
//                         DEL  iff the op that holds c is a D op, c is its first column and token_at(w, c, Q) != 0; its length is the op's.
//   which event passes    tcmi_indel_rule_passes: the variant table's rule (variants_rule.h) with the same tie.
//   the table's key       tcmi_indel_key: column | kind | h, h = the length of a DEL (exact), tcmi_indel_hash of an INS.
#pragma once
#include <stdint.h>

#include "variants_rule.h"

#define TCMI_INDEL_HD TCMI_VAR_HD

enum { TCMI_INDEL_INS = 1, TCMI_INDEL_DEL = 2 };
enum { TCMI_INDEL_HASH_BITS = 34, TCMI_INDEL_SEEDS = 4 };

// ---- the inserted bases of the insertion behind op k ------------------------------------------------------------------------------------
// The iterator restates ins_after (pack_device.h; cigar_host.h) and keeps the query index: when op k + 1 is an I op, the I ops behind op k
// with only P ops between them; when it is a P op with an op behind it, every I op up to the next reference-consuming op — S ops on the
// way consume query, H and P do not.  y: the query index behind op k.  ld(j): CIGAR word j (len << 4 | op).  next(): the query index of
// the next inserted base, -1 when there is none (any more).
template <class Ld> struct tcmi_ins_iter {
    Ld ld;
    uint32_t n, j, left;
    int64_t y;
    bool strict, done;
    TCMI_INDEL_HD tcmi_ins_iter(Ld ld_, uint32_t n_, uint32_t k, int64_t y_) : ld(ld_), n(n_), j(k + 1), left(0), y(y_), strict(false), done(true)
    {
        if (k + 1 >= n) return;
        const uint32_t op2 = ld(k + 1) & 0xFu;
        strict = op2 == 1;
        done = !(op2 == 1 || (op2 == 6 && k + 2 < n));
    }
    TCMI_INDEL_HD int64_t next()
    {
        while (!done) {
            if (left) { --left; return y++; }
            if (j >= n) break;
            const uint32_t c = ld(j++), o = c & 0xFu;
            if (o == 1) left = c >> 4;
            else if (strict ? o != 6 : (o == 0 || o == 2 || o == 3 || o == 7 || o == 8)) break;
            else if (o == 4) y += c >> 4;
        }
        done = true;
        return -1;
    }
};

// ---- the hash of an insertion: (seed, nibbles..., len) -> bits in 0..34 low bits, the rest zero ---------------------------------------------
// Fed base by base, so that a kernel hashes while it walks.  FNV-1a's prime with a fold per step; the finish is a multiply-fold that
// spreads the last nibble over the bits that are kept.
TCMI_INDEL_HD inline uint64_t tcmi_indel_hash_begin(uint32_t seed) { return 0xCBF29CE484222325ull ^ ((uint64_t)seed * 0x9E3779B97F4A7C15ull); }
TCMI_INDEL_HD inline uint64_t tcmi_indel_hash_step(uint64_t h, uint32_t nib)
{
    h = (h ^ (uint64_t)(nib & 15u)) * 0x100000001B3ull;
    return h ^ (h >> 29);
}
TCMI_INDEL_HD inline uint64_t tcmi_indel_hash_end(uint64_t h, int64_t len, int bits)
{
    h = (h ^ (uint64_t)len) * 0xD6E8FEB86659FD93ull;
    h ^= h >> 32;
    h *= 0xD6E8FEB86659FD93ull;
    h ^= h >> 32;
    return bits <= 0 ? 0ull : h & ((1ull << (bits > TCMI_INDEL_HASH_BITS ? TCMI_INDEL_HASH_BITS : bits)) - 1ull);
}

// ---- the key of an event in the device table: column (29 bits) | kind (1 bit: 1 INS, 0 DEL) | h (34 bits) -------------------------------
// Never 0, the empty slot: an INS has the kind bit, a DEL a length of at least 1 (an op of length 0 holds no column).  CIGAR lengths
// have 28 bits, so a DEL's key is exact.
TCMI_INDEL_HD inline uint64_t tcmi_indel_key(int32_t col, int kind, uint64_t h)
{
    return ((uint64_t)(uint32_t)col << 35) | ((uint64_t)(kind == TCMI_INDEL_INS) << 34) | (h & ((1ull << 34) - 1ull));
}
TCMI_INDEL_HD inline int32_t tcmi_indel_key_col(uint64_t key) { return (int32_t)(key >> 35); }
TCMI_INDEL_HD inline int tcmi_indel_key_kind(uint64_t key) { return ((key >> 34) & 1ull) ? TCMI_INDEL_INS : TCMI_INDEL_DEL; }
TCMI_INDEL_HD inline uint64_t tcmi_indel_key_h(uint64_t key) { return key & ((1ull << 34) - 1ull); }
// where a key's probe sequence starts in a table of 2^k slots (linear from there)
TCMI_INDEL_HD inline uint64_t tcmi_indel_slot0(uint64_t key)
{
    key *= 0x9E3779B97F4A7C15ull;
    return key ^ (key >> 31);
}

// ---- which event is reported: the variant table's rule, the same tie -------------------------------------------------------------------
TCMI_INDEL_HD inline bool tcmi_indel_rule_ok(const tcmi_var_rule &r)
{
    return r.den >= 1 && r.den <= 1000000 && r.num >= 0 && r.num <= r.den && r.min_alt_depth >= 1 && r.min_depth >= 0;
}
// count, cov >= 0 below 2^31, num <= den <= 10^6: the products stay below 2^51
TCMI_INDEL_HD inline bool tcmi_indel_rule_passes(int32_t count, int32_t cov, const tcmi_var_rule &r)
{
    return cov >= (r.min_depth > 1 ? r.min_depth : 1) && count >= r.min_alt_depth && (int64_t)count * r.den >= r.num * (int64_t)cov;
}

// the letter of a SEQ nibble (SAM spec §4.2)
TCMI_INDEL_HD inline char tcmi_indel_letter(uint32_t nib) { return "=ACMGRSVTWYHKDBN"[nib & 15u]; }

// ---- HOST: lists of events (indels_text.cpp) --------------------------------------------------------------------------------------------
#include <string>
#include <vector>

#include "../../include/tcmi.h"

static_assert(sizeof(tcmi_indel_event) == 32, "tcmi_indel_event is six int32 and an int64");
static_assert(sizeof(tcmi_indel_totals) == 16, "tcmi_indel_totals is four int32");

// events with the letters of their insertions (text_off into `text`, -1 for a DEL)
struct tcmi_indel_list {
    std::vector<tcmi_indel_event> ev;
    std::string text;
};
// `parts` (each in any order; a part's event may repeat another part's) -> out in THE order (pos, kind, len, bases), equal events merged
// with their counts summed, the text repacked in that order; with `rule` only the events that pass it (count summed, their own cov).
// false: an event's text_off / len does not lie in its part's text, or equal events disagree on cov.
__attribute__((visibility("hidden"))) bool tcmi_indel_merge(const std::vector<tcmi_indel_list> &parts, const tcmi_var_rule *rule, tcmi_indel_list &out);
