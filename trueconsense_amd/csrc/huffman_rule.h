// huffman_rule.h — how a canonical Huffman code's decoding tables follow from its code lengths (RFC 1951 §3.2.2), stated once for the
// device decoder (bgzf_device.h: build_table; bgzf_symbols.hip) and for a host program that holds it against a bit-by-bit decoder
// (tests/huffman_table_main.cpp): it includes no HIP header and compiles with any C++ compiler.  All arithmetic is integer.
//
//   the limits       cnt[len] codes of length len, len = 1 .. 15.  The codes of a canonical code are ordered by length; left-aligned
//                    in 15 bits, those of length len end at lim15[len] = sum over k <= len of cnt[k] << (15 - k)  (tcmi_huff_term is
//                    the summand), and they begin where the length before ends: lim15[len - 1], lim15[0] = 0.  The limits never
//                    decrease with len, empty lengths included.
//   the verdict      the code is over-subscribed iff lim15[15] > 1 << 15  (Kraft); an incomplete code — lim15[15] < 1 << 15 — is
//                    accepted: the bits from lim15[15] on name no symbol.
//   a slot           of a root table of `root` bits: r = the slot's index with its bits reversed (the first bit of the stream is the
//                    code's top bit).  The code that r begins with has length L = 1 + #{len <= root : r >= lim15[len] >> (15 - root)};
//                    L > root: no code of at most root bits (a longer one, or the unused space).  In the canonically sorted symbol
//                    array — by length, then by symbol — it is entry off[L] + ((r - (lim15[L - 1] >> (15 - root))) >> (root - L)),
//                    off[L] = the codes shorter than L.  The limit below L is a multiple of 1 << (root - L + 1), so that is
//                    (r >> (root - L)) + bias, bias = off[L] - (lim15[L - 1] >> (15 - L)).
//   a key            says all of that about a length in one word, L on top: tcmi_huff_key.  Put where its length's slots begin (r =
//                    the limit below; only lengths that have codes, and L = root + 1 where the codes of at most root bits end, if
//                    that is inside the table), the keys turn the count above into a running maximum over r: the key in force at r
//                    is the largest at or below r, and r = 0 always has one.  tcmi_huff_key_index, tcmi_huff_key_filled read it.
//   an entry         tcmi_huff_entry: what a table holds for a symbol of nbits bits (the layout: bgzf_device.h).
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define TCMI_HUFF_HD __attribute__((host)) __attribute__((device))
#else
#define TCMI_HUFF_HD
#endif

enum { TCMI_HUFF_LITLEN = 0, TCMI_HUFF_DIST = 1, TCMI_HUFF_CODELEN = 2 };
enum { TCMI_HUFF_E_LIT = 1 << 8, TCMI_HUFF_E_BASE = 1 << 9, TCMI_HUFF_E_EOB = 1 << 10 };

// cnt codes of length len (1 .. 15): their share of the 15-bit code space
TCMI_HUFF_HD inline uint32_t tcmi_huff_term(uint32_t cnt, int len) { return cnt << (15 - len); }
// lim15 of the longest length -> the code is not over-subscribed
TCMI_HUFF_HD inline bool tcmi_huff_fits(uint32_t lim15_of_15) { return lim15_of_15 <= (1u << 15); }
// a 15-bit limit as the root table's slots see it (exact for len <= root: the low bits are zero)
TCMI_HUFF_HD inline uint32_t tcmi_huff_root_limit(uint32_t lim15, int root) { return lim15 >> (15 - root); }
// The key of length L (1 .. root + 1): L << 27 | (bias + 512) << 5 | the shift root - L.  bias + 512 lies in 0 .. 832 (off <= 320,
// the limit below L in units of L-bit codes <= 512).  L = root + 1 — no entry — shifts by 31 bits and points at entry 0, which a reader
// may fetch and must drop (tcmi_huff_key_filled).
TCMI_HUFF_HD inline uint32_t tcmi_huff_key(int L, uint32_t off, uint32_t lim15_before, int root)
{
    if (L > root) return ((uint32_t)L << 27) | (512u << 5) | 31u;
    return ((uint32_t)L << 27) | (((off + 512u - (lim15_before >> (15 - L))) & 0x3FFFFFu) << 5) | (uint32_t)(root - L);
}
// where the key goes: the first reversed slot index of its length
TCMI_HUFF_HD inline uint32_t tcmi_huff_key_start(uint32_t lim15_before, int root) { return tcmi_huff_root_limit(lim15_before, root); }
// the slot's place in the sorted symbol array, by the key in force at r
TCMI_HUFF_HD inline uint32_t tcmi_huff_key_index(uint32_t key, uint32_t r) { return (r >> (key & 31u)) + ((key >> 5) & 0x3FFFFFu) - 512u; }
TCMI_HUFF_HD inline bool tcmi_huff_key_filled(uint32_t key, int root) { return key < ((uint32_t)(root + 1) << 27); }

// cnt[1 .. 15] -> lim15[0 .. 15], off[0 .. 15] (index 0: 0)
TCMI_HUFF_HD inline void tcmi_huff_limits(const uint32_t cnt[16], uint32_t lim15[16], uint32_t off[16])
{
    uint32_t lim = 0, o = 0;
    lim15[0] = 0;
    off[0] = 0;
    for (int len = 1; len <= 15; ++len) {
        off[len] = o;
        o += cnt[len];
        lim += tcmi_huff_term(cnt[len], len);
        lim15[len] = lim;
    }
}
// the length of the code that the reversed slot bits r begin with; root + 1: none of at most root bits
TCMI_HUFF_HD inline int tcmi_huff_slot_length(uint32_t r, const uint32_t lim15[16], int root)
{
    int L = 1;
    for (int len = 1; len <= root; ++len) L += r >= tcmi_huff_root_limit(lim15[len], root) ? 1 : 0;
    return L;
}

// The table entry of symbol sym with a code of nbits bits; 0: not a symbol of this alphabet (286, 287; distances 30, 31).  A LENGTH entry
// is laid out for pass A's rounds: extra-bit count in bits 16-19 (with the code length in bits 0-3 that is an s_bfe_u32 operand:
// entry & 0x000F000F), code + extra bits in bits 11-15, base length in bits 20-28.
TCMI_HUFF_HD inline uint32_t tcmi_huff_entry(int kind, int sym, int nbits)
{
    if (sym < 0) return 0u;
    if (kind == TCMI_HUFF_CODELEN) return (uint32_t)nbits | ((uint32_t)sym << 16);
    if (kind == TCMI_HUFF_LITLEN) {
        if (sym < 256) return (uint32_t)nbits | TCMI_HUFF_E_LIT | ((uint32_t)sym << 16);
        if (sym == 256) return (uint32_t)nbits | TCMI_HUFF_E_EOB;
        const int s = sym - 257;
        if (s > 28) return 0u;
        int eb = 0, base = 3 + s;
        if (s == 28) base = 258;
        else if (s >= 8) { eb = (s >> 2) - 1; base = 3 + ((4 + (s & 3)) << eb); }
        return (uint32_t)nbits | ((uint32_t)(nbits + eb) << 11) | TCMI_HUFF_E_BASE | ((uint32_t)eb << 16) | ((uint32_t)base << 20);
    }
    if (sym > 29) return 0u;
    int eb = 0, base = 1 + sym;
    if (sym >= 4) { eb = (sym >> 1) - 1; base = 1 + ((2 + (sym & 1)) << eb); }
    return (uint32_t)nbits | ((uint32_t)eb << 4) | TCMI_HUFF_E_BASE | ((uint32_t)base << 16);
}
