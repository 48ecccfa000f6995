// bgzf_device.h — what the device BGZF decoder's translation units share (bam_device.hip: the drivers, record index;
// bgzf_symbols.hip, bgzf_copy.hip: the decode kernels): block descriptors, status words, Huffman table entries and the table
// builder — and the contract between the two kernels: the token format, the stamp buffer, their launch functions.
// Wire format: SAM spec §4.1 (BGZF), RFC 1951 (DEFLATE); pysam / htslib's role for indexing.py:19,96-100.
//
// DEVICE: the BGZF blocks of a BAM file -> the inflated BAM byte stream + the record starts of every block, in two kernels:
//
//   bgzf_symbols   Huffman symbols -> tokens.  A block's symbols are decoded by 32 lanes (two blocks per workgroup; 64 when a
//                  payload exceeds 4 KB: one block per workgroup, staged a window at a time beyond 16 KB), speculatively in parallel.
//   bgzf_copy      tokens -> bytes: the LZ77 copies through an LDS ring of the recent output, the chain of BAM records, the flush —
//                  and the block's CRC-32 against its trailer, taken from the ring while a segment is flushed.
//
// Why two kernels.  A deflate stream is serial twice over: the position of symbol k + 1 is known only when symbol k is decoded,
// and a match may copy what the previous match produced.  Round 2's one-kernel decoder walked both chains in one wavefront, one
// symbol at a time: ~60 wave-instructions per symbol, all of them issued for a single useful lane, and the kernel was bound by
// instruction issue.  bgzf_symbols cuts the first chain into pieces that 32 or 64 lanes decode at once (its file says how),
// bgzf_copy takes the second 64 tokens at a time (its file).  What passes between them is the token array:
//
// Tokens (32 bits): literal 1<<31 | byte — or two literals in one token, 1<<31 | 1<<24 | byte | next byte << 8: a lane whose symbol is a
// literal of at most nine bits takes the next code in the same round if that is such a literal too and starts in the same stretch
// of bits (meeting points stay round starts; literal-heavy chunks are the ones whose lanes take longest) —; match len (9 bits) | (dist - 1) << 9; raw 1<<30 | len << 17 | offset of the bytes from
// the block's payload start (a stored deflate block, in pieces of <= 8 191 bytes).  Block b's tokens lie in order at
// BlockDesc::tok, n_tok[b] of them; two-literal tokens are written by bgzf_symbols<1, *> only and read by bgzf_copy<true, *> only.
// A launch takes a range of the file's blocks and the token array's base: a file whose tokens do not fit the context's scratch is
// decoded a batch of blocks at a time (bam_device.hip: decode_enqueue).
//
// Bit / byte work, bound by instruction issue and the LDS pipe, not by HBM and not a contraction: no MFMA.
#pragma once
#include "bgzf_host.h"          // BlockDesc, the blocks' status words ST_*
#include "huffman_rule.h"       // limits, slots and entries of a canonical code
#include "tcmi_internal.h"

namespace {

#ifndef TCMI_INFLATE_LL_ROOT
#define TCMI_INFLATE_LL_ROOT 9
#endif
#ifndef TCMI_INFLATE_D_ROOT
#define TCMI_INFLATE_D_ROOT 8
#endif
constexpr int LL_ROOT = TCMI_INFLATE_LL_ROOT, D_ROOT = TCMI_INFLATE_D_ROOT, CL_ROOT = 7;   // root-table bits; longer codes take slow_decode
static_assert(D_ROOT >= CL_ROOT, "the code-length table borrows the distance table's LDS");
constexpr int MAX_REC_PER_BLOCK = 65536 / 36 + 2;   // a record is at least 36 bytes (block_size + 32 fixed + 1 name byte ..)

static __constant__ uint8_t CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ inline uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
// LDS written by some lanes of a wavefront and read by others of the same wavefront: the hardware keeps a wavefront's LDS
// operations in order, so all this has to do is keep the compiler from moving them (no barrier: a workgroup may hold several
// wavefronts that each work on a block of their own)
__device__ __forceinline__ void wave_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }

// Inclusive scans over the 64 lanes of a wavefront with data-parallel-primitive moves (no LDS, no waits): four shifts inside
// the rows of 16 lanes, then the last lane of row 0 / 2 into row 1 / 3 and lane 31 into the upper half.  Lanes shifted in
// from outside a row read 0, the identity of both operators below (the maximum is over unsigned values).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_shift(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, true);
}
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v)
{
    v += dpp_shift<0x111, 0xF>(v);          // row_shr:1
    v += dpp_shift<0x112, 0xF>(v);          // row_shr:2
    v += dpp_shift<0x114, 0xF>(v);          // row_shr:4
    v += dpp_shift<0x118, 0xF>(v);          // row_shr:8
    v += dpp_shift<0x142, 0xA>(v);          // row_bcast:15 into rows 1 and 3
    v += dpp_shift<0x143, 0xC>(v);          // row_bcast:31 into rows 2 and 3
    return v;
}
__device__ __forceinline__ uint32_t wave_scan_max(uint32_t v)
{
    v = max(v, dpp_shift<0x111, 0xF>(v));
    v = max(v, dpp_shift<0x112, 0xF>(v));
    v = max(v, dpp_shift<0x114, 0xF>(v));
    v = max(v, dpp_shift<0x118, 0xF>(v));
    v = max(v, dpp_shift<0x142, 0xA>(v));
    v = max(v, dpp_shift<0x143, 0xC>(v));
    return v;
}

// Root-table entries (32 bits): code length in bits 0-3 (0: not in the root table — a longer code or none), kind in bits 8-10;
// a literal in bits 16-23; a distance: extra bits in bits 4-7, base in bits 16-31; a length: see tcmi_huff_entry (huffman_rule.h).
// The hot loop needs no arithmetic on symbols.
constexpr uint32_t E_LIT = TCMI_HUFF_E_LIT, E_BASE = TCMI_HUFF_E_BASE, E_EOB = TCMI_HUFF_E_EOB;
enum { K_LITLEN = TCMI_HUFF_LITLEN, K_DIST = TCMI_HUFF_DIST, K_CODELEN = TCMI_HUFF_CODELEN };

typedef uint32_t tab_t;             // (16-bit entries with base / extra bits computed per symbol: half the table LDS, measured slower)

__device__ inline uint32_t make_entry(int kind, int sym, int nbits) { return tcmi_huff_entry(kind, sym, nbits); }

// an inclusive sum over each row of 16 lanes (the per-length counters live in lanes 0 .. 15)
__device__ __forceinline__ uint32_t row_scan_add(uint32_t v)
{
    v += dpp_shift<0x111, 0xF>(v);
    v += dpp_shift<0x112, 0xF>(v);
    v += dpp_shift<0x114, 0xF>(v);
    v += dpp_shift<0x118, 0xF>(v);
    return v;
}

// lens[0 .. n) -> cnt[1 .. 15], the canonically ordered symbols sym[] with their ready table entries ent[] beside them, and the root
// table.  Returns false for an over-subscribed code.  huffman_rule.h states the rule; tests/huffman_table_main.cpp holds it against a
// bit-by-bit decoder.  The kernel is bound by instruction issue, so what counts here is instructions:
//   the rank    a symbol's place among those of its length.  Per group of 64 symbols, four ballots — one per bit of the length — give
//               every lane the mask of the lanes whose length equals ITS OWN (bit set: the ballot, else its complement; the four
//               ANDed): mbcnt of that mask is the lane's rank inside the group, its popcount the group's count for that length.  The
//               counts of the groups in front come from a 16-entry LDS table that every group reads at its own lengths and then
//               raises (lanes of one length write one value); after the last group the table IS the histogram.  (One ballot and one
//               rank per (group, length) pair — 75 pairs for the literal/length code — was 1 832 static instructions.)
//   the scan    lane len holds cnt[len]: a row scan gives off[len] (into the same 16-entry table: a symbol's slot is off[len] + its
//               place), a second one over cnt[len] << (15 - len) the left-aligned limits (tcmi_huff_term), whose last says whether
//               the code is over-subscribed.
//   an entry    is made once per symbol, with its length, when the symbol is ranked (make_entry on a group's symbols: for four of the
//               five literal/length groups the compiler knows they are literals), not once per slot.
//   a slot      needs the length of the code its reversed bits begin with: the number of limits at or below them.  Nobody counts:
//               the lanes of the lengths that have codes put a key (tcmi_huff_key: length, shift, where the length's entries lie)
//               where their slots begin, and a running maximum over the reversed indices — a lane takes 2^(ROOT - 6) consecutive
//               ones, a maximum scan joins the lanes — hands every slot its key; the slot shifts, adds, takes the ready entry
//               from ent[] and is done: ~ 10 instructions (was: nine steps of shift, subtract, compare and two selects, an LDS read
//               of sym[] and the whole of make_entry: ~ 110 instructions per 64 slots).
// MAXG: groups of 64 symbols (5 for the 286 literal/length codes).  ol: 16 words of scratch.  ent: an entry per coded symbol (entry 0 is
// read, and dropped, by a slot without a code even when there is none); it may lie where the long-code table will: build_long only
// moves its tail down.  tab serves as scratch on the way (the keys, in reversed-index order) and is written whole.
template <int MAXG, int ROOT>
__device__ __forceinline__ bool build_table(const uint8_t *lens, int n, uint16_t *cnt, uint16_t *sym, tab_t *ent, uint32_t *ol, tab_t *tab, int kind, uint32_t *rs)
{
    static_assert(ROOT >= 7 && ROOT <= 14, "a turn of the slot loop is 64 slots");
    // (the lane, opaque to the compiler: what follows from the lane alone — reversed slot bits, symbol numbers, the literals' entries — is
    // a few instructions here and would otherwise be kept in registers, or spilled, across the whole loop over a block's headers)
    int lane = threadIdx.x & 63;
    asm volatile("" : "+v"(lane));
    wave_sync();                                // (LDS hand-offs between the lanes of this wavefront)
    uint32_t lp[MAXG];                          // per group: the symbol's length | its place among the symbols of that length << 4
#pragma unroll
    for (int g = 0; g < MAXG; ++g) lp[g] = g * 64 + lane < n ? (uint32_t)lens[g * 64 + lane] & 15u : 0u;
    if (lane < 16) ol[lane] = 0;
    wave_sync();
#pragma unroll
    for (int g = 0; g < MAXG; ++g) {
        const uint32_t len = lp[g];
        uint32_t eq_lo = ~0u, eq_hi = ~0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t mine = (uint32_t)((int32_t)(len << (31 - k)) >> 31);     // bit k of the length, on every bit
            const unsigned long long m = __ballot(mine != 0);
            eq_lo &= ~((uint32_t)m ^ mine);
            eq_hi &= ~((uint32_t)(m >> 32) ^ mine);
        }
        const uint32_t below = __builtin_amdgcn_mbcnt_hi(eq_hi, __builtin_amdgcn_mbcnt_lo(eq_lo, 0u));
        const uint32_t before = ol[len];        // of this length in the groups in front
        lp[g] = len | ((before + below) << 4);
        asm volatile("" : "+v"(lp[g]));         // (here, not where it is used: the masks need not live that long)
        wave_sync();
        ol[len] = before + (uint32_t)__popc(eq_lo) + (uint32_t)__popc(eq_hi);
        wave_sync();
    }
    // lanes 0 .. 15: the histogram (length 0 is no code), offsets, limits
    const uint32_t c = lane >= 1 && lane < 16 ? ol[lane] : 0u;
    const uint32_t term = tcmi_huff_term(c, lane & 15);
    const uint32_t o_incl = row_scan_add(c), lim15 = row_scan_add(term);
    // (the table in slot-index-reversed order for now: a lane's S slots are consecutive there.  Cleared for the keys.)
    constexpr int S = 1 << (ROOT - 6);
    uint32_t *const mine = tab + lane * S;
#pragma unroll
    for (int j = 0; j < S; ++j) mine[j] = 0u;
    wave_sync();
    if (lane < 16) {
        cnt[lane] = (uint16_t)c;                // ... to LDS for the long codes (build_long)
        ol[lane] = o_incl - c;
    }
    if (lane == ROOT) { rs[0] = lim15 >> (14 - ROOT); rs[1] = o_incl; }     // the first code longer than ROOT bits, the entries in front of it
    {   // lane L = 1 .. ROOT + 1: the key of its length where that length's slots begin
        const uint32_t start = tcmi_huff_key_start(lim15 - term, ROOT);
        if (lane >= 1 && lane <= ROOT + 1 && (c != 0 || lane == ROOT + 1) && start < (1u << ROOT)) tab[start] = tcmi_huff_key(lane & 15, o_incl - c, lim15 - term, ROOT);
    }
    const bool ok = tcmi_huff_fits((uint32_t)__builtin_amdgcn_readlane((int)lim15, 15));
    wave_sync();
    // every symbol to its slot in the sorted array, its entry beside it
#pragma unroll
    for (int g = 0; g < MAXG; ++g) {
        const uint32_t len = lp[g] & 15u;
        if (len) {
            const uint32_t at = ol[len] + (lp[g] >> 4);
            sym[at] = (uint16_t)(g * 64 + lane);
            ent[at] = make_entry(kind, g * 64 + lane, (int)len);
        }
    }
    // the key in force at every reversed slot index: the running maximum — inside the lane, then over the lanes in front
    uint32_t key[S];
#pragma unroll
    for (int j = 0; j < S; ++j) key[j] = mine[j];
#pragma unroll
    for (int j = 1; j < S; ++j) key[j] = max(key[j], key[j - 1]);
    const uint32_t in_front = dpp_shift<0x138, 0xF>(wave_scan_max(key[S - 1]));      // wave_shr:1 (lane 0: 0)
    wave_sync();                                // (every lane has its keys, every entry is in place)
    // root table: slot i holds the symbol whose code is a prefix of the bits of i (first stream bit = bit 0); this lane's
    // S reversed indices lane * S + j are the slots reverse(lane) + 64 * reverse(j)
    const uint32_t i0 = __builtin_bitreverse32((uint32_t)lane) >> 26;
#pragma unroll
    for (int j = 0; j < S; ++j) {
        const uint32_t k = max(key[j], in_front);
        const uint32_t e = ent[tcmi_huff_key_index(k, (uint32_t)(lane * S + j))];        // (no entry: entry 0, dropped)
        tab[i0 + 64u * (__builtin_bitreverse32((uint32_t)j) >> (38 - ROOT))] = tcmi_huff_key_filled(k, ROOT) ? e : 0u;
    }
    wave_sync();
    return ok;
}

// ---- between bgzf_symbols and bgzf_copy: the tokens (see the head of this file) ----------------------------------------------------
constexpr uint32_t TOK_LIT = 1u << 31, TOK_RAW = 1u << 30;
constexpr uint32_t TOK_LIT2 = 1u << 24;              // a literal token that carries TWO bytes (the second in bits 8 - 15): bits 24 - 25 = literals - 1
constexpr uint32_t RAW_PIECE = 8191;

// ---- the stamp buffer (diagnostic, TCMI_INFLATE_STAMPS; tools/inflate_stamps.py reads it): 16 words per block and kernel, bgzf_symbols'
// for all the launch's blocks first, then bgzf_copy's; s_memtime at the phase boundaries and a few counters.  Null: no stamps.
#define TCMI_STAMP(buf_, blk_, k_) do { if (buf_) { if ((threadIdx.x & 63) == 0) (buf_)[(size_t)(blk_) * 16 + (k_)] = __builtin_amdgcn_s_memtime(); } } while (0)
#define TCMI_STAMP_ADD(buf_, blk_, k_, v_) do { if (buf_) { if ((threadIdx.x & 63) == 0) (buf_)[(size_t)(blk_) * 16 + (k_)] += (v_); } } while (0)

} // namespace

// bgzf_symbols.hip / bgzf_copy.hip: compressed file + block table in HBM -> inflated stream, record starts per block, a status word per block
// (everything on ctx->stream; the arrays are the caller's, sized as bam_device.hip's decode_on_device sizes them)
struct tcmi_bgzf_decode_args {
    const uint8_t *d_file;          // compressed file, 16-byte aligned, >= 4 KiB of slack behind it
    const void *d_desc;             // BlockDesc [n_blocks]
    uint32_t *d_tok;                // token array (BlockDesc::tok / tok_cap)
    uint32_t *d_ntok;               // [n_blocks]
    uint8_t *d_out;                 // inflated stream (BlockDesc::uout)
    uint32_t *d_slot;               // [n_blocks][MAX_REC_PER_BLOCK] record starts
    uint32_t *d_nrec;               // [n_blocks]
    int32_t *d_over;                // [n_blocks] bytes by which a block's last record runs into the next blocks
    uint32_t *d_first;              // [n_blocks] offset of the first record start the block found in itself (0xFFFFFFFF: none)
    uint32_t *d_stat;               // [n_blocks] ST_*
    size_t n_blocks;                // of the file (or range): the arrays' length
    size_t first_block = 0, count = ~(size_t)0;    // the blocks this launch decodes ([first_block, first_block + count), clipped): a batch
    uint64_t tok_base = 0;          // d_tok holds the tokens from BlockDesc::tok = tok_base on (the batch's first block's)
    uint32_t pay_dwords;            // the largest block's payload in dwords + slack
    uint32_t n_ref;                 // reference sequences of the BAM header (a record's refID must be one of them)
    int verify_crc = 1;             // bgzf_copy checks every block's CRC-32 against its trailer while it flushes the bytes (ST_BAD_CRC)
    int scratch_div = 1;            // (tests) a lane of bgzf_symbols may park 1 / scratch_div of its share of the token scratch: overflowing lanes send their block through pass B
    int short_tokens;               // the file compresses less than ~12 : 1 (many short matches): bgzf_copy's variant with teams; 2: less than ~4 : 1: ... and short far matches finished in the set-up
};
int tcmi_bgzf_decode_launch(tcmi_ctx *ctx, const tcmi_bgzf_decode_args &a);          // (bgzf_copy.hip) both kernels, in order
// Its two halves, on ctx->stream, for the launch's nb blocks from b_first on.  `stamps`: that kernel's part of the stamp buffer, or
// null; `report`: a line on stderr about the variant chosen and how many workgroups of it a compute unit holds (diagnostic).
// bgzf_symbols.hip: *two_literals = the variant chosen may have written tokens of two literals
int tcmi_bgzf_symbols_launch(tcmi_ctx *ctx, const tcmi_bgzf_decode_args &a, size_t b_first, size_t nb, uint64_t *stamps, bool report, bool *two_literals);
// bgzf_copy.hip: two_literals as bgzf_symbols_launch said
int tcmi_bgzf_copy_launch(tcmi_ctx *ctx, const tcmi_bgzf_decode_args &a, size_t b_first, size_t nb, uint64_t *stamps, bool report, bool two_literals);
