// bgzf_symbols.hip — DEVICE: the Huffman symbols of every BGZF block's deflate stream -> tokens (RFC 1951; the first of the device
// decoder's two kernels: bgzf_device.h says why there are two and what a token is; bgzf_copy.hip turns the tokens into bytes).
//
// The position of symbol k + 1 is known only when symbol k is decoded.  That chain is cut into pieces: lane c starts decoding at
// bit s_c = start + c * chunk — in the middle of nowhere, except for lane 0 — and notes where its symbols cross into each new
// stretch of bits.  Huffman streams resynchronise: after a few dozen bits a decoder that started on a wrong bit starts a symbol on
// a right one, and from there on it IS the serial decoder.  A lane stops when a symbol of its own starts on a position that the
// lane in front of it has noted: from there the two would decode the same (pass A).  Starting from lane 0 the chain of these
// meeting points says which lane holds the true symbols of which bit range, and how many they are; the lanes then put the true
// tokens in order (gathered in output order, or — blocks of thousands of tokens — moved row by row; a lane that overflows its
// scratch sends the block through pass B: the true ranges once more, tokens straight to their places).  Nothing in this depends on
// luck or timing: a lane that never meets anyone simply goes on to the block's end, and lane 0 alone is the serial decoder.
// (tools/spec_inflate_proto.py: the same scheme in Python.)
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "bgzf_device.h"

namespace {

constexpr int CL_SLAB = 496;                        // bit positions of the code-length stream looked up at a time
// bgzf_symbols<NB>: NB BGZF blocks per workgroup — one wavefront each for header and tables, then wavefront 0 decodes all of
// them, 64 / NB lanes per block.  NB = 2 (32 lanes: two rows of the data-parallel moves) unless a payload exceeds 4 KB; then
// NB = 1 (tcmi_bgzf_symbols_launch has the measurements).
struct BlkTabs {                                    // per block
    tab_t ll[1 << LL_ROOT];                         // (first: the code-length stream's table of all positions, CL_SLAB + 16 entries)
    tab_t dt[1 << D_ROOT];                          // (first: the code-length code's root table)
    tab_t long_ll[288], long_d[32];                 // entries of the codes longer than the root bits, in canonical order
    // per such length, for the look-up by range compare: the end of its codes, left-aligned in 15 bits (ascending: canonical codes are
    // ordered by length), and first code | index of its first entry in long_* << 16
    uint32_t lim_ll[16 - LL_ROOT], fb_ll[16 - LL_ROOT], lim_d[16 - D_ROOT], fb_d[16 - D_ROOT];
    // what the block's wavefront hands to the decoding wavefront and gets back
    uint32_t pos;               // first symbol / behind the end-of-block code
    uint32_t end;               // first bit behind the payload
    uint32_t ntok;              // tokens so far
    uint32_t err;               // ST_*
    uint32_t go;                // 1: symbols to decode at pos
    uint32_t last;              // 1: the stream's last deflate block
};
struct HdrScratch {                                 // per block, while its header is decoded and its tables are built
    uint8_t lens[320];
    uint8_t cll[20];
    uint16_t sym_ll[288], sym_d[32], sym_cl[20];
    uint16_t cnt_ll[16], cnt_d[16], cnt_cl[16];
    uint32_t rs[6];
    uint32_t ol[16];                                // build_table: per length, the counts so far; then offset | limit (tcmi_huff_word)
};
#ifndef TCMI_SYM_MOVE
#define TCMI_SYM_MOVE 8                             // bgzf_symbols: tokens a lane has in flight when the tokens are gathered to their places
#endif
#ifndef TCMI_SYM_ROWS
#define TCMI_SYM_ROWS 32                            // bgzf_symbols: parked rows a turn of the row-by-row mover takes (a load each, all in flight)
#endif
#ifndef TCMI_SYM_WAVES
#define TCMI_SYM_WAVES 5                            // bgzf_symbols: wavefronts per SIMD the register budget is cut for (5: 96 VGPRs; with 4 — 128 —
                                                    // a BAM's 2 094 workgroups fill every CU's register file: 182 us instead of 173)
#endif
constexpr int RING = 8;
struct PassALds {
    uint2 ring[64][RING];       // pass A, per lane: {first symbol start in a stretch, symbols decoded before it}
    uint2 rec[64];              // per lane: {state | target << 8, position}
};
// The header scratch and pass A's notes share their LDS: a workgroup barrier separates the two phases, and with 2.3 KB less a
// workgroup of two blocks stays under the 18.2 KB at which nine of them fit a compute unit.
template <int NB>
struct SymLds {
    BlkTabs b[NB];
    union {
        HdrScratch h[NB];
        PassALds a;
    };
};
static_assert((CL_SLAB + 16) * 4 <= sizeof(tab_t) * (1 << LL_ROOT), "the code-length position table borrows the literal/length table's LDS");

struct SymArgs {
    const uint32_t *__restrict__ file32;
    const BlockDesc *blocks;
    uint32_t *tokens;           // block b's tokens at tokens + blocks[b].tok: tok_cap final ones, then tok_cap of scratch
    uint32_t *n_tok;            // [n_blocks]
    uint32_t *status;           // [n_blocks]
    int32_t n_blocks;           // (the launch's blocks end here)
    int32_t first_block;        // ... and start here: workgroup 0's first block
    uint32_t pay_dwords;        // dwords of dynamic LDS per block behind SymLds: the largest block's payload + slack
    uint32_t win_dwords;        // bgzf_symbols<1, true>: dwords of payload staged at a time (a window that moves along the block)
    uint32_t gather_max;        // a pass with more true tokens than this moves them row by row (else: gathered in output order)
    uint32_t shift_bias;        // (A/B) pass A's stretches this many powers of two shorter than chunk / 4 .. chunk / 2
    uint32_t scratch_div;       // a lane's scratch is cut to 1 / scratch_div of its share (tests: lanes overflow and the block goes through pass B)
    uint64_t *stamps;           // diagnostic (TCMI_INFLATE_STAMPS): 16 words per block, s_memtime at the phase boundaries; or null
};

// 32 bits of the staged payload from bit p on (any lane, any position)
__device__ __forceinline__ uint32_t peek32(const uint32_t *pay, uint32_t p)
{
    const uint32_t w = p >> 5;
    return __builtin_amdgcn_alignbit(pay[w + 1], pay[w], p);
}
// ... 64 bits: what one symbol can take (15 + 5 bits of a length, 15 + 13 of a distance)
__device__ __forceinline__ void peek64(const uint32_t *pay, uint32_t p, uint32_t &lo, uint32_t &hi)
{
    const uint32_t w = p >> 5;
    const uint32_t w0 = pay[w], w1 = pay[w + 1], w2 = pay[w + 2];
    lo = __builtin_amdgcn_alignbit(w1, w0, p);
    hi = __builtin_amdgcn_alignbit(w2, w1, p);
}

// The codes longer than the root bits: one ready-made table entry per such code, in canonical order.  A lane finds its code
// without a walk through memory: canonical codes are ordered by length, so the code's first 15 bits, left-aligned, lie below the
// end of exactly the lengths that are long enough — counting the ends at or below them gives the length.
// build_table has left every symbol's entry in `out`, in canonical order; those of the long codes are its tail, from rs[1] on, and
// move down to the front (a turn reads 64 entries before it writes them further down, and later turns read further up).
template <int ROOT>
__device__ __forceinline__ void build_long(const uint16_t *cnt, const uint32_t *rs, tab_t *out, uint32_t *lim_out, uint32_t *fb_out)
{
    const int lane = threadIdx.x & 63;
    uint32_t first = uni(rs[0]);
    const uint32_t at = uni(rs[1]);
    uint32_t n = 0;
    uint32_t my_lim = 0x10000u, my_fb = 0;                 // (entry 15 - ROOT: above every code)
#pragma unroll
    for (int len = ROOT + 1; len <= 15; ++len) {
        const uint32_t c = uni(cnt[len]);
        if (lane == len - ROOT - 1) { my_lim = (first + c) << (15 - len); my_fb = (first & 0xFFFFu) | (n << 16); }
        first = (first + c) << 1;
        n += c;
    }
    if (lane <= 15 - ROOT) { lim_out[lane] = my_lim; fb_out[lane] = my_fb; }
    if (at == 0) return;                                    // (every code is a long one: they lie in place)
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        const uint32_t i = i0 + (uint32_t)lane;
        uint32_t e = 0;
        if (i < n) e = out[at + i];
        wave_sync();
        if (i < n) out[i] = e;
        wave_sync();
    }
}

template <int ROOT>
__device__ __forceinline__ uint32_t long_lookup(const uint32_t *lim, const uint32_t *fb, const tab_t *tab, uint32_t bits)
{
    const uint32_t r15 = __builtin_bitreverse32(bits) >> 17;
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < 15 - ROOT; ++k) n += r15 >= lim[k] ? 1u : 0u;
    if (n >= (uint32_t)(15 - ROOT)) return 0u;
    const uint32_t f = fb[n];
    const uint32_t code = r15 >> (14 - ROOT - n);
    if (code < (f & 0xFFFFu)) return 0u;                    // (a slot of the root table whose short code names no symbol)
    return tab[(f >> 16) + (code - (f & 0xFFFFu))];
}

// an inclusive sum over each group of 64 / NB lanes (one block's lanes): pairs of rows of 16, or the wavefront
template <int NB>
__device__ __forceinline__ uint32_t group_scan_add(uint32_t v)
{
    v += dpp_shift<0x111, 0xF>(v);
    v += dpp_shift<0x112, 0xF>(v);
    v += dpp_shift<0x114, 0xF>(v);
    v += dpp_shift<0x118, 0xF>(v);
    v += dpp_shift<0x142, 0xA>(v);
    if (NB == 1) v += dpp_shift<0x143, 0xC>(v);
    return v;
}

enum { SY_LIT = 0, SY_MATCH = 1, SY_EOB = 2, SY_BAD = 3 };

// ---- header of one deflate block and its tables: one wavefront, the block's own (T, pay) ------------------------------------------
// -> T.go = 1 and T.pos at the first symbol (a Huffman block), or the block's stream is finished / damaged (T.go = 0).  Stored
// deflate blocks are turned into raw tokens here and the next header is taken at once.
__device__ __forceinline__ void block_header(BlkTabs &T, HdrScratch &H, const uint32_t *pay, uint32_t base_bit, uint32_t *toks, uint32_t cap, bool &last,
                                          uint64_t *stamps, int blk, bool one_header = false)
{
    const int lane = threadIdx.x & 63;
    uint32_t pos = uni(T.pos), ntok = uni(T.ntok), err = ST_OK;
    const uint32_t end = uni(T.end);
    bool go = false;
    while (!last && err == ST_OK && !go) {
        if (pos + 3u > end) { err = ST_BAD_STREAM; break; }
        const uint32_t h = uni(peek32(pay, pos));
        last = (h & 1u) != 0;
        const uint32_t type = (h >> 1) & 3u;
        pos += 3;
        if (type == 0) {
            // ---- stored block: byte-align, LEN / NLEN, LEN raw bytes -> raw tokens ------------------------------------------
            pos = (pos + 7u) & ~7u;
            if (pos + 32u > end) { err = ST_BAD_STREAM; break; }
            const uint32_t v = uni(peek32(pay, pos));
            const uint32_t len = v & 0xFFFFu;
            if (((v >> 16) ^ len) != 0xFFFFu) { err = ST_BAD_STREAM; break; }
            pos += 32;
            if (pos + len * 8u > end) { err = ST_BAD_STREAM; break; }
            const uint32_t off = (pos - base_bit) >> 3;
            const uint32_t pieces = (len + RAW_PIECE - 1u) / RAW_PIECE;
            if (ntok + pieces > cap) { err = ST_BAD_STREAM; break; }
            if ((uint32_t)lane < pieces) {
                const uint32_t o = (uint32_t)lane * RAW_PIECE;
                toks[ntok + (uint32_t)lane] = TOK_RAW | (min(len - o, RAW_PIECE) << 17) | (off + o);
            }
            ntok += pieces;
            pos += len * 8u;
            if (one_header) break;                              // (the caller stages the payload behind the stored bytes first)
            continue;
        }
        if (type == 3) { err = ST_BAD_STREAM; break; }
        // ---- code lengths -------------------------------------------------------------------------------------------------------
        int nlen = 288, ndist = 32;
        wave_sync();
        if (type == 1) {
            for (int i = lane; i < 320; i += 64) H.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5;
        } else {
            if (pos + 14u > end) { err = ST_BAD_STREAM; break; }
            const uint32_t hh = uni(peek32(pay, pos));
            nlen = (int)(hh & 31u) + 257;
            ndist = (int)((hh >> 5) & 31u) + 1;
            const int ncode = (int)((hh >> 10) & 15u) + 4;
            pos += 14;
            if (nlen > 286 || ndist > 30) { err = ST_BAD_STREAM; break; }
            if (lane < 19) H.cll[lane] = 0;
            wave_sync();
            // (19 x 3 bits: three looks of up to 8 lengths each, lane k takes the k-th)
            for (int i0 = 0; i0 < ncode; i0 += 8) {
                const uint32_t v = uni(peek32(pay, pos + (uint32_t)i0 * 3u));
                const int k = i0 + lane;
                if (lane < 8 && k < ncode) H.cll[CL_ORDER[k]] = (uint8_t)((v >> (3 * lane)) & 7u);
            }
            pos += (uint32_t)ncode * 3u;
            if (!build_table<1, CL_ROOT>(H.cll, 19, H.cnt_cl, H.sym_cl, T.long_d, H.ol, T.dt, K_CODELEN, H.rs + 4)) { err = ST_BAD_STREAM; break; }
            for (int i = lane; i < 320; i += 64) H.lens[i] = 0;
            // The code-length symbols (0 .. 15: a length; 16: the previous length 3 - 6 times; 17 / 18: 3 - 10 / 11 - 138 zeros) are
            // a serial chain too, but a short one over few bits.  Every bit position of a slab is looked up by some lane (what
            // symbol would start here, how many lengths would it give, how many bits would it take: step | rep << 4 | val << 12);
            // the chain is then followed through that table with one scalar look-up per symbol that only notes the entry
            // (lane j keeps the j-th of 64), and what the symbols mean is worked out for 64 of them at a time: a sum scan of
            // the repeat counts places them, a maximum scan finds for every "16" the last symbol in front that names a length.
            uint32_t *const P = T.ll;
            uint32_t got = 0, prev = 0;
            const uint32_t total = (uint32_t)(nlen + ndist);
            bool first = true;
            while (got < total && err == ST_OK) {
                wave_sync();
#pragma unroll 2
                for (int o = lane; o < CL_SLAB + 16; o += 64) {
                    const uint32_t v = peek32(pay, pos + (uint32_t)o);
                    const uint32_t e = T.dt[v & ((1u << CL_ROOT) - 1u)];
                    const uint32_t nb = e & 15u, sym = e >> 16;
                    const uint32_t x = v >> nb;
                    const uint32_t eb = sym < 16u ? 0u : sym == 16u ? 2u : sym == 17u ? 3u : 7u;
                    const uint32_t rep = sym < 16u ? 1u : sym == 18u ? 11u + (x & 127u) : 3u + (x & (sym == 16u ? 3u : 7u));
                    const uint32_t val = sym <= 16u ? sym : 0u;
                    P[o] = nb && o < CL_SLAB ? (nb + eb) | (rep << 4) | (val << 12) : 0u;      // (0 behind the slab: the chain stops there)
                }
                wave_sync();
                // The chain of symbols through the table — a symbol's place is known when its predecessor is decoded — was followed one
                // LDS round trip per symbol (~300 of them per header: a fifth of this kernel's time).  Pointer doubling instead: J holds,
                // for every bit position, where the chain stands 2^k symbols later (a position without a code stays where it is);
                // six squarings of the table — every lane takes eight positions — and lane j, applying the squarings its bits ask for,
                // knows where symbol j starts; symbols j + 64, j + 128, .. lie J_6 further each.
                uint16_t *const J = reinterpret_cast<uint16_t *>(T.long_ll);       // 512 entries (the long-code tables are built later)
                static_assert(sizeof(T.long_ll) >= 512 * sizeof(uint16_t) && CL_SLAB + 16 <= 512, "the doubling table borrows the long-code table's LDS");
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const uint32_t at0 = (uint32_t)lane + 64u * i;
                    const uint32_t e0 = at0 < (uint32_t)CL_SLAB + 16u ? P[at0] : 0u;
                    J[at0] = (uint16_t)(e0 ? at0 + (e0 & 15u) : at0);
                }
                wave_sync();
                uint32_t pm[5];
                pm[0] = 0;
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    if (((uint32_t)lane >> k) & 1u) pm[0] = J[pm[0]];
                    uint32_t t8[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) t8[i] = J[lane + 64 * i];
#pragma unroll
                    for (int i = 0; i < 8; ++i) t8[i] = J[t8[i]];
                    wave_sync();                                            // (every lane has read before any lane writes)
#pragma unroll
                    for (int i = 0; i < 8; ++i) J[lane + 64 * i] = (uint16_t)t8[i];
                    wave_sync();
                }
#pragma unroll
                for (int m = 1; m < 5; ++m) pm[m] = J[pm[m - 1]];
                uint32_t o = 0;
                bool stopped = false;
#pragma unroll
                for (int m = 0; m < 5; ++m) {
                    if (!(got < total && err == ST_OK && !stopped)) break;
                    uint32_t mine = P[pm[m]];
                    // the symbols of this batch that lie on the chain (a prefix of the lanes), and of them those that are still wanted:
                    // up to and including the one that completes the `total` lengths
                    const unsigned long long zmask = __ballot(mine == 0);
                    const uint32_t nv = zmask ? (uint32_t)__builtin_ctzll(zmask) : 64u;
                    if ((uint32_t)lane >= nv) mine = 0;
                    uint32_t rep = (mine >> 4) & 255u;
                    const uint32_t incl0 = wave_scan_add(rep);
                    const unsigned long long reach = __ballot(mine != 0 && got + incl0 >= total);
                    const uint32_t n_take = reach ? min(nv, (uint32_t)__builtin_ctzll(reach) + 1u) : nv;
                    if ((uint32_t)lane >= n_take) { mine = 0; rep = 0; }
                    // lane j: its symbol's place and value
                    const uint32_t v = mine >> 12;
                    const uint32_t at = got + incl0 - ((mine >> 4) & 255u);
                    const uint32_t named = wave_scan_max(mine != 0 && v != 16u ? (uint32_t)lane + 1u : 0u);     // 1 + the lane whose value a "16" here repeats
                    const uint32_t theirs = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((named - 1u) << 2), (int)v);
                    const uint32_t val = named ? theirs : prev;
                    if (__ballot(mine != 0 && (at + rep > total || (first && lane == 0 && v == 16u)))) { err = ST_BAD_STREAM; break; }
                    if (mine != 0 && val != 0) {
#pragma unroll
                        for (uint32_t i = 0; i < 6; ++i)            // (zeros are not stored, so rep <= 6)
                            if (i < rep) H.lens[at + i] = (uint8_t)val;
                    }
                    if (n_take) {
                        prev = (uint32_t)__builtin_amdgcn_readlane((int)val, (int)(n_take - 1u));
                        got += (uint32_t)__builtin_amdgcn_readlane((int)incl0, (int)(n_take - 1u));
                        // behind the last symbol taken
                        o = (uint32_t)__builtin_amdgcn_readlane((int)(pm[m] + (mine & 15u)), (int)(n_take - 1u));
                        first = false;
                    }
                    if (n_take < 64u && got < total) {                     // the chain ends here: no such code, or the slab's end
                        stopped = true;
                        o = (uint32_t)__builtin_amdgcn_readlane((int)pm[m], (int)n_take);
                        if (o < (uint32_t)CL_SLAB) err = ST_BAD_STREAM;
                    }
                }
                if (err == ST_OK && got < total && !stopped) err = ST_BAD_STREAM;      // (320 symbols give at least 320 lengths: not reached)
                pos += o;
                if (pos > end) err = ST_BAD_STREAM;
            }
            if (err != ST_OK) break;
            wave_sync();
            if (uni(H.lens[256]) == 0) { err = ST_BAD_STREAM; break; }    // no end-of-block code
        }
        TCMI_STAMP(stamps, blk, 2);
        // ---- tables: the root tables as in bgzf_inflate, the longer codes as ready-made entries ------------------------------------
        // (the sorted entries are made where the long-code tables will be: the doubling table above is done with that LDS)
        static_assert(sizeof(T.long_ll) >= 288 * sizeof(tab_t) && sizeof(T.long_d) >= 32 * sizeof(tab_t), "an entry per symbol");
        if (!build_table<5, LL_ROOT>(H.lens, nlen, H.cnt_ll, H.sym_ll, T.long_ll, H.ol, T.ll, K_LITLEN, H.rs)) { err = ST_BAD_STREAM; break; }
        if (!build_table<1, D_ROOT>(H.lens + nlen, ndist, H.cnt_d, H.sym_d, T.long_d, H.ol, T.dt, K_DIST, H.rs + 2)) { err = ST_BAD_STREAM; break; }
        build_long<LL_ROOT>(H.cnt_ll, H.rs, T.long_ll, T.lim_ll, T.fb_ll);
        build_long<D_ROOT>(H.cnt_d, H.rs + 2, T.long_d, T.lim_d, T.fb_d);
        if (pos >= end) { err = ST_BAD_STREAM; break; }
        go = true;
        TCMI_STAMP(stamps, blk, 3);
    }
    wave_sync();
    if (lane == 0) { T.pos = pos; T.ntok = ntok; T.err = err; T.go = go && err == ST_OK ? 1u : 0u; T.last = last ? 1u : 0u; }
}

// The rounds of pass A, hand-scheduled (see the comment at their use).  Two insertion points for the kernels that put two literals into
// one token (one block per workgroup: files whose blocks hold thousands of literals): the look-up of the code behind a literal, in
// flight under the match lanes' distance look-up, and its resolution — this symbol a literal of <= 9 bits, the next code a root-table
// literal that starts in the same stretch and ends within the soft end: then the token carries both bytes and the lane moves on
// behind the second.  (For the bench file's blocks — two per workgroup, a thousand tokens each — the 22 instructions cost more than
// the 19 % of rounds they save: 141 -> 150 us; at 2.6 : 1 the rounds fall by 38 %.)
// The round's sections, in order (labels in the text below): LT the loop's head — a lane whose symbols cross into a new stretch of 2^shift
// bits notes {p, total} in its ring (LA1); every fourth round the lanes that have crossed since look their position up in their target's
// ring (LB*: a target that has stopped at or in front of the lane is replaced by the lane it met, or by the next one; equal positions:
// met — back to the meeting point, stop); LC1 one symbol: 64 bits of payload, the 9-bit root look-up (LLl: a longer literal / length
// code by range compare), LDeob an end-of-block code, LC3 the literal's token / the length's base and extra bits, PAIR_LOOK_, the
// 8-bit distance root look-up (LLd: a longer one), LC5 PAIR_RESOLVE_, the new position (LDover: past the end), LC6 the token's store
// into the lane's row of the scratch; LDend lanes at the payload's end without an end-of-block code; LX out.
#define TCMI_PAIR_LOOK "v_lshrrev_b32 v44, v50, v47\n" "v_and_b32 v44, 0x1ff, v44\n" "v_lshl_add_u32 v44, v44, 2, %[tabs]\n" "ds_read_b32 v44, v44\n"
#define TCMI_PAIR_RESOLVE "s_waitcnt lgkmcnt(0)\n" "v_and_b32 v40, v49, v44\n" "v_and_b32 v45, 15, v44\n" "v_add_u32 v46, v52, v45\n" "v_xor_b32 v42, %[p], v52\n" "v_lshrrev_b32 v42, %[shift], v42\n" "v_bfe_u32 v40, v40, 8, 1\n" "v_cmp_gt_u32 vcc, 10, v50\n" "v_cmp_eq_u32 s[86:87], 1, v40\n" "s_and_b64 vcc, vcc, s[86:87]\n" "v_cmp_eq_u32 s[86:87], 0, v42\n" "s_and_b64 vcc, vcc, s[86:87]\n" "v_cmp_le_u32 s[86:87], v46, %[wend]\n" "s_and_b64 vcc, vcc, s[86:87]\n" "v_bfe_u32 v40, v44, 16, 8\n" "v_lshl_or_b32 v40, v40, 8, v51\n" "v_or_b32 v40, 0x1000000, v40\n" "v_cndmask_b32 v51, v51, v40, vcc\n" "v_cndmask_b32 v52, v52, v46, vcc\n"
#define TCMI_PASS_A_ASM(PAIR_LOOK_, PAIR_RESOLVE_) \
                asm volatile( \
                    "s_mov_b64 s[92:93], exec\n" \
                    "LT%=:\n" \
                    "s_mov_b64 exec, %[run]\n" \
                    "s_cbranch_execz LX%=\n" \
                    "v_lshrrev_b32 v40, %[shift], %[p]\n" \
                    "v_cmp_ne_u32 vcc, v40, %[kprev]\n" \
                    "s_and_saveexec_b64 s[80:81], vcc\n" \
                    "s_cbranch_execz LA1%=\n" \
                    "v_mov_b32 %[kprev], v40\n" \
                    "v_and_b32 v41, 7, v40\n" \
                    "v_lshl_add_u32 v41, v41, 3, %[ringb]\n" \
                    "ds_write2_b32 v41, %[p], %[total] offset1:1\n" \
                    "v_mov_b32 %[crossp], %[p]\n" \
                    "v_mov_b32 %[crosst], %[total]\n" \
                    "LA1%=:\n" \
                    "s_mov_b64 exec, %[run]\n" \
                    "s_and_b32 s90, %[rounds], 3\n" \
                    "s_cmp_eq_u32 s90, 3\n" \
                    "s_cbranch_scc0 LC%=\n" \
                    "v_cmp_ne_u32 vcc, -1, %[crossp]\n" \
                    "s_and_saveexec_b64 s[80:81], vcc\n" \
                    "s_cbranch_execz LB9%=\n" \
                    "v_add_u32 v41, -1, %[lim]\n" \
                    "v_min_u32 v41, %[tgt], v41\n" \
                    "v_lshl_add_u32 v42, v41, 3, %[recbase]\n" \
                    "ds_read2_b32 v[44:45], v42 offset1:1\n" \
                    "v_lshrrev_b32 v40, %[shift], %[crossp]\n" \
                    "v_and_b32 v40, 7, v40\n" \
                    "v_lshlrev_b32 v40, 3, v40\n" \
                    "s_waitcnt lgkmcnt(0)\n" \
                    "v_and_b32 v43, 3, v44\n" \
                    "v_cmp_ne_u32 vcc, 0, v43\n" \
                    "v_cmp_ge_u32 s[86:87], %[crossp], v45\n" \
                    "s_and_b64 vcc, vcc, s[86:87]\n" \
                    "v_cmp_lt_u32 s[86:87], %[tgt], %[lim]\n" \
                    "s_and_b64 vcc, vcc, s[86:87]\n" \
                    "s_and_saveexec_b64 s[82:83], vcc\n" \
                    "v_cmp_eq_u32 vcc, 1, v43\n" \
                    "v_add_u32 %[tgt], 1, %[tgt]\n" \
                    "s_and_b64 exec, exec, vcc\n" \
                    "v_lshrrev_b32 %[tgt], 8, v44\n" \
                    "s_mov_b64 exec, s[82:83]\n" \
                    "v_cmp_lt_u32 vcc, %[tgt], %[lim]\n" \
                    "s_and_b64 exec, exec, vcc\n" \
                    "s_cbranch_execz LB8%=\n" \
                    "v_lshl_add_u32 v42, %[tgt], 6, v40\n" \
                    "v_add_u32 v42, %[ringbase], v42\n" \
                    "ds_read2_b32 v[44:45], v42 offset1:1\n" \
                    "s_waitcnt lgkmcnt(0)\n" \
                    "v_cmp_eq_u32 vcc, v44, %[crossp]\n" \
                    "s_and_b64 exec, exec, vcc\n" \
                    "s_cbranch_execz LB8%=\n" \
                    "v_mov_b32 %[midx], v45\n" \
                    "v_mov_b32 %[state], 1\n" \
                    "v_mov_b32 %[p], %[crossp]\n" \
                    "v_mov_b32 %[total], %[crosst]\n" \
                    "v_lshl_or_b32 v43, %[tgt], 8, 1\n" \
                    "ds_write2_b32 %[recb], v43, %[p] offset1:1\n" \
                    "s_andn2_b64 %[run], %[run], exec\n" \
                    "LB8%=:\n" \
                    "s_mov_b64 exec, s[80:81]\n" \
                    "v_mov_b32 %[crossp], -1\n" \
                    "LB9%=:\n" \
                    "s_mov_b64 exec, %[run]\n" \
                    "s_cbranch_execz LX%=\n" \
                    "LC%=:\n" \
                    "v_cmp_lt_u32 vcc, %[p], %[wend]\n" \
                    "s_xor_b64 s[86:87], vcc, exec\n" \
                    "s_cmp_lg_u64 s[86:87], 0\n" \
                    "s_cbranch_scc1 LDend%=\n" \
                    "LC1%=:\n" \
                    "v_lshrrev_b32 v40, 5, %[p]\n" \
                    "v_lshl_add_u32 v40, v40, 2, %[pay]\n" \
                    "ds_read2_b32 v[44:45], v40 offset1:1\n" \
                    "ds_read_b32 v46, v40 offset:8\n" \
                    "s_waitcnt lgkmcnt(0)\n" \
                    "v_alignbit_b32 v47, v45, v44, %[p]\n" \
                    "v_alignbit_b32 v48, v46, v45, %[p]\n" \
                    "v_and_b32 v40, 0x1ff, v47\n" \
                    "v_lshl_add_u32 v40, v40, 2, %[tabs]\n" \
                    "ds_read_b32 v49, v40\n" \
                    "s_waitcnt lgkmcnt(0)\n" \
                    "v_and_b32 v50, 15, v49\n" \
                    "v_cmp_eq_u32 vcc, 0, v50\n" \
                    "s_cbranch_vccnz LLl%=\n" \
                    "LC2%=:\n" \
                    "v_bfe_u32 v41, v49, 8, 3\n" \
                    "v_cmp_eq_u32 vcc, 4, v41\n" \
                    "s_cbranch_vccnz LDeob%=\n" \
                    "LC3%=:\n" \
                    "v_bfe_u32 v51, v49, 16, 8\n" \
                    "v_or_b32 v51, 0x80000000, v51\n" \
                    "v_add_u32 v52, %[p], v50\n" \
                    PAIR_LOOK_ \
                    "s_mov_b64 s[88:89], exec\n" \
                    "v_cmp_eq_u32 vcc, 2, v41\n" \
                    "s_and_b64 exec, exec, vcc\n" \
                    "s_cbranch_execz LC5%=\n" \
                    "v_bfe_u32 v53, v49, 11, 5\n" \
                    "v_alignbit_b32 v54, v48, v47, v53\n" \
                    "v_and_b32 v40, 0xff, v54\n" \
                    "v_lshl_add_u32 v40, v40, 2, %[tabs]\n" \
                    "ds_read_b32 v55, v40 offset:%[odt]\n" \
                    "v_lshrrev_b32 v42, v50, v47\n" \
                    "v_bfe_u32 v43, v49, 16, 4\n" \
                    "v_bfe_u32 v42, v42, 0, v43\n" \
                    "v_bfe_u32 v43, v49, 20, 9\n" \
                    "v_add_u32 v56, v43, v42\n" \
                    "s_waitcnt lgkmcnt(0)\n" \
                    "v_and_b32 v57, 15, v55\n" \
                    "v_cmp_eq_u32 vcc, 0, v57\n" \
                    "s_cbranch_vccnz LLd%=\n" \
                    "LC4%=:\n" \
                    "v_bfe_u32 v43, v55, 4, 4\n" \
                    "v_lshrrev_b32 v42, v57, v54\n" \
                    "v_bfe_u32 v42, v42, 0, v43\n" \
                    "v_lshrrev_b32 v40, 16, v55\n" \
                    "v_add_u32 v42, v42, v40\n" \
                    "v_add_u32 v42, -1, v42\n" \
                    "v_lshl_or_b32 v51, v42, 9, v56\n" \
                    "v_add3_u32 v52, %[p], v53, v57\n" \
                    "v_add_u32 v52, v52, v43\n" \
                    "LC5%=:\n" \
                    "s_and_b64 exec, s[88:89], %[run]\n" \
                    "s_cbranch_execz LT%=\n" \
                    PAIR_RESOLVE_ \
                    "v_mov_b32 %[p], v52\n" \
                    "v_cmp_gt_u32 vcc, %[p], %[end]\n" \
                    "s_cbranch_vccnz LDover%=\n" \
                    "LC6%=:\n" \
                    "s_mov_b64 s[80:81], exec\n" \
                    "v_cmp_ne_u32 vcc, 0, %[room]\n" \
                    "s_and_b64 exec, exec, vcc\n" \
                    "global_store_dword %[sptr], v51, off\n" \
                    "v_add_u32 %[room], -1, %[room]\n" \
                    "v_lshl_add_u64 %[sptr], %[sptr], 0, %[sstride]\n" \
                    "s_mov_b64 exec, s[80:81]\n" \
                    "v_add_u32 %[total], 1, %[total]\n" \
                    "s_add_u32 %[rounds], %[rounds], 1\n" \
                    "s_branch LT%=\n" \
                    "LDend%=:\n" \
                    "s_mov_b64 s[82:83], exec\n" \
                    "s_mov_b64 exec, s[86:87]\n" \
                    "v_mov_b32 %[state], 3\n" \
                    "v_mov_b32 v43, 3\n" \
                    "ds_write2_b32 %[recb], v43, %[p] offset1:1\n" \
                    "s_andn2_b64 %[run], %[run], exec\n" \
                    "s_andn2_b64 exec, s[82:83], s[86:87]\n" \
                    "s_cbranch_execz LT%=\n" \
                    "s_branch LC1%=\n" \
                    "LDeob%=:\n" \
                    "s_mov_b64 s[82:83], exec\n" \
                    "s_and_b64 exec, exec, vcc\n" \
                    "v_add_u32 %[p], %[p], v50\n" \
                    "v_add_u32 %[total], 1, %[total]\n" \
                    "v_mov_b32 %[state], 2\n" \
                    "v_mov_b32 v43, 2\n" \
                    "ds_write2_b32 %[recb], v43, %[p] offset1:1\n" \
                    "s_andn2_b64 %[run], %[run], exec\n" \
                    "s_andn2_b64 exec, s[82:83], exec\n" \
                    "s_cbranch_execz LT%=\n" \
                    "s_branch LC3%=\n" \
                    "LDover%=:\n" \
                    "s_mov_b64 s[82:83], exec\n" \
                    "s_and_b64 exec, exec, vcc\n" \
                    "v_mov_b32 %[state], 3\n" \
                    "v_mov_b32 v43, 3\n" \
                    "ds_write2_b32 %[recb], v43, %[p] offset1:1\n" \
                    "s_andn2_b64 %[run], %[run], exec\n" \
                    "s_andn2_b64 exec, s[82:83], exec\n" \
                    "s_cbranch_execz LT%=\n" \
                    "s_branch LC6%=\n" \
                    "LLl%=:\n" \
                    "s_mov_b64 s[84:85], exec\n" \
                    "s_and_b64 exec, exec, vcc\n" \
                    "v_bfrev_b32 v40, v47\n" \
                    "v_lshrrev_b32 v40, 17, v40\n" \
                    "v_add_u32 v41, %[oliml], %[tabs]\n" \
                    "ds_read2_b32 v[58:59], v41 offset1:1\n" \
                    "ds_read2_b32 v[60:61], v41 offset0:2 offset1:3\n" \
                    "ds_read2_b32 v[62:63], v41 offset0:4 offset1:5\n" \
                    "s_waitcnt lgkmcnt(0)\n" \
                    "v_sub_u32 v58, v40, v58\n" \
                    "v_sub_u32 v59, v40, v59\n" \
                    "v_sub_u32 v60, v40, v60\n" \
                    "v_sub_u32 v61, v40, v61\n" \
                    "v_sub_u32 v62, v40, v62\n" \
                    "v_sub_u32 v63, v40, v63\n" \
                    "v_ashrrev_i32 v58, 31, v58\n" \
                    "v_ashrrev_i32 v59, 31, v59\n" \
                    "v_ashrrev_i32 v60, 31, v60\n" \
                    "v_ashrrev_i32 v61, 31, v61\n" \
                    "v_ashrrev_i32 v62, 31, v62\n" \
                    "v_ashrrev_i32 v63, 31, v63\n" \
                    "v_add3_u32 v58, v58, v59, v60\n" \
                    "v_add3_u32 v61, v61, v62, v63\n" \
                    "v_add3_u32 v42, v58, v61, 6\n" \
                    "v_min_u32 v41, 5, v42\n" \
                    "v_lshl_add_u32 v41, v41, 2, %[tabs]\n" \
                    "ds_read_b32 v43, v41 offset:%[ofbll]\n" \
                    "v_sub_u32 v41, 5, v42\n" \
                    "v_lshrrev_b32 v41, v41, v40\n" \
                    "s_waitcnt lgkmcnt(0)\n" \
                    "v_and_b32 v40, 0xffff, v43\n" \
                    "v_cmp_ge_u32 vcc, v41, v40\n" \
                    "v_cmp_gt_u32 s[86:87], 6, v42\n" \
                    "s_and_b64 vcc, vcc, s[86:87]\n" \
                    "v_sub_u32 v41, v41, v40\n" \
                    "v_lshrrev_b32 v40, 16, v43\n" \
                    "v_add_u32 v41, v41, v40\n" \
                    "v_and_b32 v41, 0x1ff, v41\n" \
                    "v_lshl_add_u32 v41, v41, 2, %[tabs]\n" \
                    "ds_read_b32 v49, v41 offset:%[olongll]\n" \
                    "s_waitcnt lgkmcnt(0)\n" \
                    "v_and_b32 v50, 15, v49\n" \
                    "v_cmp_ne_u32 s[86:87], 0, v50\n" \
                    "s_and_b64 vcc, vcc, s[86:87]\n" \
                    "s_andn2_b64 exec, exec, vcc\n" \
                    "s_cbranch_execz LLl9%=\n" \
                    "v_mov_b32 %[state], 3\n" \
                    "v_mov_b32 v43, 3\n" \
                    "ds_write2_b32 %[recb], v43, %[p] offset1:1\n" \
                    "s_andn2_b64 %[run], %[run], exec\n" \
                    "LLl9%=:\n" \
                    "s_and_b64 exec, s[84:85], %[run]\n" \
                    "s_cbranch_execz LT%=\n" \
                    "s_branch LC2%=\n" \
                    "LLd%=:\n" \
                    "s_mov_b64 s[84:85], exec\n" \
                    "s_and_b64 exec, exec, vcc\n" \
                    "v_bfrev_b32 v40, v54\n" \
                    "v_lshrrev_b32 v40, 17, v40\n" \
                    "v_add_u32 v41, %[olimd], %[tabs]\n" \
                    "ds_read2_b32 v[58:59], v41 offset1:1\n" \
                    "ds_read2_b32 v[60:61], v41 offset0:2 offset1:3\n" \
                    "ds_read2_b32 v[62:63], v41 offset0:4 offset1:5\n" \
                    "ds_read_b32 v42, v41 offset:24\n" \
                    "s_waitcnt lgkmcnt(0)\n" \
                    "v_sub_u32 v58, v40, v58\n" \
                    "v_sub_u32 v59, v40, v59\n" \
                    "v_sub_u32 v60, v40, v60\n" \
                    "v_sub_u32 v61, v40, v61\n" \
                    "v_sub_u32 v62, v40, v62\n" \
                    "v_sub_u32 v63, v40, v63\n" \
                    "v_sub_u32 v42, v40, v42\n" \
                    "v_ashrrev_i32 v58, 31, v58\n" \
                    "v_ashrrev_i32 v59, 31, v59\n" \
                    "v_ashrrev_i32 v60, 31, v60\n" \
                    "v_ashrrev_i32 v61, 31, v61\n" \
                    "v_ashrrev_i32 v62, 31, v62\n" \
                    "v_ashrrev_i32 v63, 31, v63\n" \
                    "v_ashrrev_i32 v42, 31, v42\n" \
                    "v_add3_u32 v58, v58, v59, v60\n" \
                    "v_add3_u32 v61, v61, v62, v63\n" \
                    "v_add3_u32 v42, v58, v61, v42\n" \
                    "v_add_u32 v42, 7, v42\n" \
                    "v_min_u32 v41, 6, v42\n" \
                    "v_lshl_add_u32 v41, v41, 2, %[tabs]\n" \
                    "ds_read_b32 v43, v41 offset:%[ofbd]\n" \
                    "v_sub_u32 v41, 6, v42\n" \
                    "v_lshrrev_b32 v41, v41, v40\n" \
                    "s_waitcnt lgkmcnt(0)\n" \
                    "v_and_b32 v40, 0xffff, v43\n" \
                    "v_cmp_ge_u32 vcc, v41, v40\n" \
                    "v_cmp_gt_u32 s[86:87], 7, v42\n" \
                    "s_and_b64 vcc, vcc, s[86:87]\n" \
                    "v_sub_u32 v41, v41, v40\n" \
                    "v_lshrrev_b32 v40, 16, v43\n" \
                    "v_add_u32 v41, v41, v40\n" \
                    "v_and_b32 v41, 31, v41\n" \
                    "v_lshl_add_u32 v41, v41, 2, %[tabs]\n" \
                    "ds_read_b32 v55, v41 offset:%[olongd]\n" \
                    "s_waitcnt lgkmcnt(0)\n" \
                    "v_and_b32 v57, 15, v55\n" \
                    "v_cmp_ne_u32 s[86:87], 0, v57\n" \
                    "s_and_b64 vcc, vcc, s[86:87]\n" \
                    "s_andn2_b64 exec, exec, vcc\n" \
                    "s_cbranch_execz LLd9%=\n" \
                    "v_mov_b32 %[state], 3\n" \
                    "v_mov_b32 v43, 3\n" \
                    "ds_write2_b32 %[recb], v43, %[p] offset1:1\n" \
                    "s_andn2_b64 %[run], %[run], exec\n" \
                    "LLd9%=:\n" \
                    "s_and_b64 exec, s[84:85], %[run]\n" \
                    "s_cbranch_execz LC5%=\n" \
                    "s_branch LC4%=\n" \
                    "LX%=:\n" \
                    "s_mov_b64 exec, s[92:93]\n" \
                    : [p] "+v"(p), [total] "+v"(total), [tgt] "+v"(tgt_abs), [midx] "+v"(midx), [kprev] "+v"(kprev), [state] "+v"(state), \
                      [room] "+v"(room), [crossp] "+v"(crossp), [crosst] "+v"(crosst), [sptr] "+v"(sptr), [run] "+s"(run), [rounds] "+s"(rounds) \
                    : [tabs] "v"(tabs), [pay] "v"(payb), [end] "v"(b_end), [wend] "v"(b_soft), [shift] "v"(shift), [ringb] "v"(ringb), [recb] "v"(recb), [lim] "v"(lim), \
                      [ringbase] "s"(ringbase), [recbase] "s"(recbase), [sstride] "s"(sstride), [odt] "n"(offsetof(BlkTabs, dt)), [olongll] "n"(offsetof(BlkTabs, long_ll)), \
                      [olongd] "n"(offsetof(BlkTabs, long_d)), [oliml] "n"(offsetof(BlkTabs, lim_ll)), [ofbll] "n"(offsetof(BlkTabs, fb_ll)), \
                      [olimd] "n"(offsetof(BlkTabs, lim_d)), [ofbd] "n"(offsetof(BlkTabs, fb_d)) \
                    : "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", \
                      "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63", "s80", "s81", "s82", "s83", "s84", "s85", "s86", "s87", \
                      "s88", "s89", "s90", "s92", "s93", "vcc", "scc", "memory");

// WIN (one block per workgroup): the payload is staged a window at a time.  A block of a file that compresses 2 - 4 : 1 has 16 - 26 KB of
// payload; staged whole, four workgroups fit a CU and a BAM's blocks take four rounds and a half.  With a window of 6 KB pass A runs
// over the symbols that START in the window, the chain's last lane says where the next window begins, and the tables stay.
template <int NB, bool WIN>
__global__ __launch_bounds__(64 * NB) __attribute__((amdgpu_waves_per_eu(TCMI_SYM_WAVES, TCMI_SYM_WAVES))) void bgzf_symbols(SymArgs a)
{
    static_assert(!WIN || NB == 1, "a window per wavefront");
    constexpr int SYM_BLOCKS = NB, SYM_LANES = 64 / NB;
    constexpr bool PAIRS = NB == 1;                 // two literals in one token: the kernels of one block per workgroup (payloads beyond 4 KB)
    static_assert(NB == 2 || NB == 1, "a block's lanes: two rows of 16, or the wavefront");
    __shared__ SymLds<NB> L;
    extern __shared__ __attribute__((aligned(8))) uint32_t pay_all[];   // per block: its compressed payload, from the dword that holds its first byte on
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int blk0 = a.first_block + (int)blockIdx.x * SYM_BLOCKS;
    const int blk = blk0 + wave;                    // this wavefront's block (header, tables)
    const bool have = blk < a.n_blocks;
    BlkTabs &T = L.b[wave];
    uint32_t *const pay_lds = pay_all + (size_t)wave * (WIN ? a.win_dwords : a.pay_dwords);
    const uint32_t *pay = pay_lds;                  // (WIN: moved so that pay[dword of the payload] hits the staged window)
    BlockDesc d = {};
    if (have) d = a.blocks[blk];
    const uint32_t *const gsrc = a.file32 + (d.cin >> 2);
    uint32_t *const toks = a.tokens + d.tok;
    const uint32_t base_bit = (uint32_t)(d.cin & 3u) * 8u;
    const uint32_t end = base_bit + d.clen * 8u;                    // first bit behind the payload
    // ---- the payload into LDS (+ 6 dwords: a lane looks up to 48 bits past the end; the file buffer has the slack) ----
    if (have) {
        if (a.stamps && lane < 16) a.stamps[(size_t)blk * 16 + lane] = 0;
        TCMI_STAMP(a.stamps, blk, 0);
        if constexpr (!WIN) {
            const uint32_t n = min(a.pay_dwords, (end + 31u) / 32u + 6u);
            for (uint32_t i = (uint32_t)lane; i < n; i += 64) pay_lds[i] = gsrc[i];
        }
    }
    if (lane == 0) { T.pos = base_bit; T.end = end; T.ntok = 0; T.err = ST_OK; T.go = 0; T.last = 0; }
    wave_sync();
    if (have) TCMI_STAMP(a.stamps, blk, 1);
    bool last = !have;
    bool hdr_due = true;                            // WIN: the next thing at T.pos is a deflate header (else: more symbols of the stream)
    uint32_t soft_end = end;                        // WIN: first bit behind the symbols this window's pass A takes
    for (;;) {
        if constexpr (WIN) {
            // ---- the window: from the dword of T.pos on (a header fits in well under a window; so does a symbol behind the soft end)
            if (have && uni(T.err) == ST_OK && (!last || !hdr_due)) {
                const uint32_t wfirst = uni(T.pos) >> 5, total_dw = (end + 31u) / 32u + 6u;
                const uint32_t n = min(a.win_dwords, total_dw - min(total_dw, wfirst));
                wave_sync();
                {   // (8 bytes a lane, four loads in flight; the window starts on any dword of the file: unaligned access mode)
                    const uint32_t n2 = (n + 1u) >> 1;
                    uint2 *const dst2 = reinterpret_cast<uint2 *>(pay_lds);
                    const uint32_t *const src = gsrc + wfirst;
                    for (uint32_t i = (uint32_t)lane; i < n2; i += 256) {
                        uint2 v[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) if (i + 64u * k < n2) __builtin_memcpy(&v[k], src + 2u * (i + 64u * k), 8);
#pragma unroll
                        for (int k = 0; k < 4; ++k) if (i + 64u * k < n2) dst2[i + 64u * k] = v[k];
                    }
                }
                wave_sync();
                pay = pay_lds - wfirst;
                soft_end = min(end, (wfirst + a.win_dwords - 6u) * 32u);
            }
        }
        // ---- every wavefront: its block's next header and tables ------------------------------------------------------------------
        if (have && uni(T.err) == ST_OK && (!last || (WIN && !hdr_due))) {         // (WIN, !hdr_due: the stream's symbols go on in the new window)
            if (!WIN || hdr_due) block_header(T, L.h[wave], pay, base_bit, toks, d.tok_cap, last, a.stamps, blk, WIN);
        } else if (lane == 0) T.go = 0;
        __syncthreads();
        uint32_t any = 0;
#pragma unroll
        for (int k = 0; k < NB; ++k) any |= L.b[k].go;
        if (uni(any) == 0) {
            if (WIN && have && uni(T.err) == ST_OK && !last) continue;     // (a stored block became tokens: the header behind it is next)
            break;                                  // (all streams finished or failed)
        }
        if constexpr (WIN) hdr_due = false;
        if (wave == 0) {
            // ---- wavefront 0: the symbols of all NB blocks, 64 / NB lanes each ---------------------------------------------------
            const int b = lane / SYM_LANES, c = lane % SYM_LANES, lane0 = lane - c;       // block, lane in the block, the block's first lane
            BlkTabs &B = L.b[b];
            const uint32_t *const bp = WIN ? pay : pay_all + (size_t)b * a.pay_dwords;
            const bool on = B.go != 0;
            const uint32_t b_end = B.end, start = B.pos;
            const uint32_t b_soft = WIN ? soft_end : b_end;     // where the lanes stop taking symbols (WIN: the window's end)
            const BlockDesc bd = blk0 + b < a.n_blocks ? a.blocks[blk0 + b] : BlockDesc{};
            uint32_t *const btok = a.tokens + bd.tok;
            const uint32_t bcap = bd.tok_cap;
            const uint32_t lane_cap = bcap / (uint32_t)SYM_LANES / max(a.scratch_div, 1u);     // tokens a lane may park in the scratch half (scratch_div: tests force pass B)
            // A lane's k-th parked token lies at scratch[k * SYM_LANES]: the lanes of a block decode one symbol a round each, so the
            // stores of a round fall into consecutive words (4-byte stores into a region of its own per lane cost a memory transaction
            // each: 115 MB of writes per BAM for 4.4 MB of tokens).
            uint32_t *const scratch = btok + bcap + (uint32_t)c;

            const uint32_t chunk = on ? (b_soft - min(b_soft, start) + (uint32_t)SYM_LANES - 1u) / (uint32_t)SYM_LANES : 1u;      // >= 1
            // stretches of >= 64 bits (a symbol takes <= 48: none is skipped), about chunk / 4: a lane trails its target by about
            // a chunk, RING stretches are kept
            const uint32_t shift = (uint32_t)max(6, 30 - (int)__builtin_clz(chunk | 1u) - (int)a.shift_bias);
            // One literal / length / end-of-block code at bit p; a length is followed by its distance.  A literal of at most nine bits
            // takes the next code along if that is a root-table literal too, starts in the same stretch and ends within the soft end:
            // a rule of the position alone, so that pass B and the hand-scheduled rounds below cut the stream into the same tokens.
            auto symbol = [&](uint32_t &p, uint32_t &tok) __attribute__((always_inline)) -> int {
                uint32_t lo, hi;
                peek64(bp, p, lo, hi);
                uint32_t e = B.ll[lo & ((1u << LL_ROOT) - 1u)];
                if (__builtin_expect(__ballot((e & 15u) == 0) != 0, 0)) {
                    const uint32_t e2 = long_lookup<LL_ROOT>(B.lim_ll, B.fb_ll, B.long_ll, lo);
                    if ((e & 15u) == 0) e = e2;
                }
                if ((e & 15u) == 0) return SY_BAD;
                if (e & E_LIT) {
                    const uint32_t p0 = p, nb1 = e & 15u;
                    p += nb1;
                    tok = TOK_LIT | ((e >> 16) & 0xFFu);
                    if (PAIRS && nb1 < 10u) {
                        const uint32_t e2 = B.ll[(lo >> nb1) & ((1u << LL_ROOT) - 1u)];
                        const uint32_t p3 = p + (e2 & 15u);
                        if ((e2 & E_LIT) && ((p ^ p0) >> shift) == 0u && p3 <= b_soft) { tok |= TOK_LIT2 | (((e2 >> 16) & 0xFFu) << 8); p = p3; }
                    }
                    return SY_LIT;
                }
                if (e & E_EOB) { p += e & 15u; return SY_EOB; }
                const uint32_t k = (e >> 11) & 31u;                 // code + extra bits of the length
                const uint32_t d32 = __builtin_amdgcn_alignbit(hi, lo, k);
                uint32_t f = B.dt[d32 & ((1u << D_ROOT) - 1u)];
                if (__builtin_expect(__ballot((f & 15u) == 0) != 0, 0)) {
                    const uint32_t f2 = long_lookup<D_ROOT>(B.lim_d, B.fb_d, B.long_d, d32);
                    if ((f & 15u) == 0) f = f2;
                }
                if ((f & 15u) == 0) return SY_BAD;
                const uint32_t nd = f & 15u, eb2 = (f >> 4) & 15u;
                p += k + nd + eb2;
                const uint32_t nb = e & 15u, eb = (e >> 16) & 15u;
                const uint32_t len = ((e >> 20) & 0x1FFu) + ((lo >> nb) & ((1u << eb) - 1u));
                const uint32_t dist = (f >> 16) + ((d32 >> nd) & ((1u << eb2) - 1u));
                tok = len | ((dist - 1u) << 9);
                return SY_MATCH;
            };

            // ---- pass A: every lane decodes from its own start until it meets the lane in front; the tokens go to its scratch ----
            // Meeting points are looked for where a lane's symbols cross into a new stretch of 2^shift bits: the lane notes its
            // first symbol start p in the stretch (and how many symbols it had decoded by then) in a ring of its own, and looks
            // p up in the ring of its target — the nearest lane in front that is still decoding, or the lane that one met.  Equal
            // positions are one trajectory from there on: the lane stops, its target's symbols from that one on are the true ones.
            const uint32_t s_c = start + (uint32_t)c * chunk;
            enum { RUN = 0, MERGED = 1, EOB = 2, DEAD = 3 };
            uint32_t state = on && s_c < b_soft ? RUN : DEAD;
            uint32_t tgt = (uint32_t)c + 1u, total = 0, midx = 0;
            uint32_t p = min(s_c, b_soft);
            uint32_t kprev = 0xFFFFFFFFu;
            bool spilled = false;                   // more symbols than the scratch holds: pass B decodes this block again
            uint32_t rounds = 0;
#pragma unroll
            for (int k = 0; k < RING; ++k) L.a.ring[lane][k] = make_uint2(0xFFFFFFFFu, 0u);
            L.a.rec[lane] = make_uint2(state, p);
            wave_sync();
            // The rounds, hand-scheduled (TCMI_PASS_A_ASM: ~85 instructions a round; the compiler's version of the same loop took ~180,
            // half of them bookkeeping of which lanes are in which branch — tools/spec_inflate_proto.py and tools/sym_balance_sim.py
            // are the scheme in Python).  A lane's look at its target's ring waits for the next round that is a multiple of four (the
            // lane goes on decoding meanwhile; if it has met its target, it steps back to the meeting point), and a lane's target is
            // kept as a lane of the wavefront.
            {
                uint32_t tgt_abs = (uint32_t)lane0 + tgt, room = lane_cap, crossp = 0xFFFFFFFFu, crosst = 0;
                uint64_t sptr = reinterpret_cast<uint64_t>(scratch);
                const uint64_t sstride = (uint64_t)SYM_LANES * 4u;
                const uint32_t tabs = (uint32_t)reinterpret_cast<uintptr_t>(&B), payb = (uint32_t)reinterpret_cast<uintptr_t>(bp);
                const uint32_t ringbase = (uint32_t)reinterpret_cast<uintptr_t>(&L.a.ring[0][0]), recbase = (uint32_t)reinterpret_cast<uintptr_t>(&L.a.rec[0]);
                const uint32_t ringb = ringbase + (uint32_t)lane * (RING * 8), recb = recbase + (uint32_t)lane * 8u;
                const uint32_t lim = (uint32_t)lane0 + (uint32_t)SYM_LANES;
                unsigned long long run = __ballot(state == RUN);
                static_assert(LL_ROOT == 9 && D_ROOT == 8 && RING == 8, "masks and counts below");
                if constexpr (PAIRS) { TCMI_PASS_A_ASM(TCMI_PAIR_LOOK, TCMI_PAIR_RESOLVE) } else { TCMI_PASS_A_ASM(, ) }
                tgt = tgt_abs - (uint32_t)lane0;
                spilled = total > lane_cap;
            }
            TCMI_STAMP(a.stamps, blk0, 4);
            TCMI_STAMP_ADD(a.stamps, blk0, 8, rounds);
            // ---- per block the chain of lanes that hold the true symbols: lane 0 from `start`, then whoever it met, ... ----------
            uint32_t before = 0;                    // symbols a lane decoded in front of its true start: they do not count
            bool alive = on && c == 0;
            uint32_t eob_pos = 0, berr = ST_OK;
            bool more = false;                      // WIN: the stream goes on behind this window (no end-of-block code yet)
            for (int bb = 0; bb < SYM_BLOCKS; ++bb) {
                if (uni(L.b[bb].go) == 0) continue;
                uint32_t cc = (uint32_t)bb * SYM_LANES;
                for (;;) {
                    const uint32_t st = (uint32_t)__builtin_amdgcn_readlane((int)state, (int)cc);
                    if (st == MERGED) {
                        const uint32_t t = (uint32_t)bb * SYM_LANES + (uint32_t)__builtin_amdgcn_readlane((int)tgt, (int)cc);
                        const uint32_t mi = (uint32_t)__builtin_amdgcn_readlane((int)midx, (int)cc);
                        if ((uint32_t)lane == t) { alive = true; before = mi; }
                        cc = t;
                    } else {
                        const uint32_t pp = (uint32_t)__builtin_amdgcn_readlane((int)p, (int)cc);
                        if (b == bb) {
                            if (st == EOB) eob_pos = pp;
                            else if (WIN && st == DEAD && pp >= b_soft && pp <= b_end && b_soft < b_end) { eob_pos = pp; more = true; }   // the window's end: on from there
                            else berr = ST_BAD_STREAM;
                        }
                        break;
                    }
                }
            }
            uint32_t cnt = 0;
            if (alive) {
                cnt = total - before;
                if (state == EOB) --cnt;            // (the end-of-block code is a symbol, not a token)
            }
            // exclusive sum over the block's lanes -> every lane's place among the block's tokens
            const uint32_t incl = group_scan_add<NB>(cnt);
            const uint32_t all = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((lane0 + SYM_LANES - 1) << 2), (int)incl);
            const uint32_t ntok0 = B.ntok;
            if (on && berr == ST_OK && ntok0 + all > bcap) berr = ST_BAD_STREAM;
            // a lane that parked more than its scratch holds: the whole block goes through pass B
            const unsigned long long spill_mask = __ballot(alive && spilled);
            const bool block_redo = ((spill_mask >> lane0) & (NB == 1 ? ~0ull : (1ull << (SYM_LANES & 63)) - 1ull)) != 0;
            TCMI_STAMP(a.stamps, blk0, 5);
            // The true tokens to their places, in order, behind those the block has already.  They lie where the lanes parked them: lane
            // j's k-th at scratch[k][j], of which [before_j, before_j + cnt_j) are true and belong at excl_j onwards.  The lanes of the
            // block take the OUTPUT tokens in turn (lane c: c, c + SYM_LANES, ..): every lane follows the table {where lane j's tokens
            // end, before_j - excl_j} through LDS — the owner of a lane's next token is the same lane or a later one —, reads the token
            // from the parked rows (this workgroup wrote them a moment ago: L2) and the stores of a turn are consecutive words.
            // (Round 4 left the tokens parked and gave bgzf_copy a list of 32 pieces: its lanes then fetched a batch of 64 tokens from
            // 64 rows — 170 MB of 64-byte sectors per BAM for 4.4 MB of tokens, from HBM: the rows of the 4 000 blocks in flight do
            // not fit the L2s.  Before that every lane moved its own tokens: a store per token and lane into 32 places.)
            L.a.ring[lane][0] = make_uint2(incl, before - (incl - cnt));
            uint32_t rows_max = alive && on && berr == ST_OK ? before + cnt : 0u;      // the parked rows that hold true tokens (the wavefront's: uniform turns below)
#pragma unroll
            for (int dd = 32; dd >= 1; dd >>= 1) rows_max = max(rows_max, (uint32_t)__shfl_xor((int)rows_max, dd, 64));
            wave_sync();
            if (on && berr == ST_OK) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // (the parked tokens are this wavefront's own stores)
                if (!block_redo && all <= a.gather_max) {
                    constexpr int GV = TCMI_SYM_MOVE;
                    const uint32_t *const rows = btok + bcap;
                    uint32_t *const dst = btok + ntok0;
                    uint32_t owner = 0;
                    uint2 e = L.a.ring[lane0][0];
                    for (uint32_t i0 = (uint32_t)c; i0 < all; i0 += GV * SYM_LANES) {      // (GV loads in flight: the loop is all latency)
                        uint32_t at[GV], t[GV];
#pragma unroll
                        for (int k = 0; k < GV; ++k) {
                            const uint32_t i = min(i0 + (uint32_t)(k * SYM_LANES), all - 1u);
                            while (e.x <= i && owner + 1u < (uint32_t)SYM_LANES) { ++owner; e = L.a.ring[lane0 + (int)owner][0]; }
                            at[k] = (i + e.y) * (uint32_t)SYM_LANES + owner;
                        }
#pragma unroll
                        for (int k = 0; k < GV; ++k) t[k] = rows[at[k]];
#pragma unroll
                        for (int k = 0; k < GV; ++k) if (i0 + (uint32_t)(k * SYM_LANES) < all) dst[i0 + (uint32_t)(k * SYM_LANES)] = t[k];
                    }
                } else if (!block_redo) {
                    // A block of many tokens (a file that compresses like real data: thousands per block, its parked rows 50 KB and
                    // more — with every block of the chip's round in flight they are in no L2 any more, and a lane that follows ONE
                    // owner reads one word of every row: sixteen times the bytes).  Here the rows are read as they were written — row
                    // k + r, every lane its own word: whole sectors, each once — R rows at a time, all their loads in flight; a lane's R tokens are
                    // consecutive in the output, so it stores them as four 16-byte words (word-aligned; the ends of its true range word
                    // by word).
                    constexpr int R = TCMI_SYM_ROWS;
                    const uint32_t *const mine = btok + bcap + (uint32_t)c;
                    uint32_t *const dst = btok + ntok0 + (incl - cnt);              // this lane's first true token goes here
                    const uint32_t lo = before, hi = before + cnt;
                    const uint32_t kmax = rows_max;
                    const uint32_t last_row = lane_cap ? lane_cap - 1u : 0u;
                    for (uint32_t k0 = 0; k0 < kmax; k0 += R) {
                        uint32_t t[R];
#pragma unroll
                        for (int r = 0; r < R; ++r) t[r] = mine[(size_t)min(k0 + (uint32_t)r, last_row) * SYM_LANES];
                        if (k0 >= lo && k0 + R <= hi) {
                            // (dst is word-aligned only: the 16-byte store goes through a type that says so)
                            struct __attribute__((packed, aligned(4))) W4 { uint32_t w[4]; };
                            W4 *q = reinterpret_cast<W4 *>(dst + (k0 - lo));
#pragma unroll
                            for (int r = 0; r < R; r += 4) q[r / 4] = W4{{t[r], t[r + 1], t[r + 2], t[r + 3]}};
                        } else {
#pragma unroll
                            for (int r = 0; r < R; ++r) if (k0 + r >= lo && k0 + r < hi) dst[k0 + r - lo] = t[r];
                        }
                    }
                } else {
                    // ---- pass B: the true ranges once more, tokens straight to their places -----------------------------------
                    // (the position of a lane's true start is not kept: decode from the lane's own start and drop `before` symbols)
                    uint32_t *const dst = btok + ntok0 + (incl - cnt);
                    uint32_t pp = min(s_c, b_soft);
                    for (uint32_t i = 0; alive && i < before + cnt; ++i) {
                        uint32_t tok = 0;
                        (void)symbol(pp, tok);
                        if (i >= before) dst[i - before] = tok;
                    }
                }
            }
            TCMI_STAMP(a.stamps, blk0, 6);
            if (on && c == 0) { B.ntok = ntok0 + all; B.pos = eob_pos; B.err = berr; }
            if constexpr (WIN) hdr_due = uni(__ballot(more) != 0 ? 1u : 0u) == 0u;       // (an end-of-block code was reached: a header comes next)
        }
        __syncthreads();
    }
    if (have && lane == 0) {
        a.n_tok[blk] = T.ntok;
        a.status[blk] = T.err;
    }
}

} // namespace

// Chooses the variant — blocks per workgroup, payloads staged whole or a window at a time —, launches it and says whether its tokens
// may carry two literals (bgzf_symbols<1, *> writes such tokens: bgzf_copy must then be a variant that reads them).
int tcmi_bgzf_symbols_launch(tcmi_ctx *ctx, const tcmi_bgzf_decode_args &g, size_t b_first, size_t nb, uint64_t *stamps, bool report, bool *two_literals)
{
    SymArgs sa;
    sa.stamps = stamps;
    sa.file32 = reinterpret_cast<const uint32_t *>(g.d_file);
    sa.blocks = static_cast<const BlockDesc *>(g.d_desc);
    sa.tokens = g.d_tok - g.tok_base; sa.n_tok = g.d_ntok; sa.status = g.d_stat; sa.n_blocks = (int32_t)(b_first + nb); sa.first_block = (int32_t)b_first;
    sa.pay_dwords = g.pay_dwords;
    sa.gather_max = 2048u;
    sa.scratch_div = (uint32_t)std::max(g.scratch_div, 1);
    // (measured on one 4 187-block file, kernel alone: 4 blocks per workgroup 372 us, 2: 285 us, 1: 325 us; on the harder file —
    //  4 611 blocks of 10.7 KB — 1 634 / 1 036 / 698 us: with larger payloads more lanes per block pay.  The variant of four is gone.)
    const size_t pay = (size_t)g.pay_dwords * 4;
    const int per_wg = pay <= 4096 ? 2 : 1;
    // payloads of more than 16 KB (files that compress less than ~4 : 1) are staged a window of 5 KB at a time, bgzf_symbols<1, true>:
    // 2.5 : 1 (26 KB a block): 2 766 -> 1 875 us per 1M-read file in round 3 (8 KB windows); at 6 : 1 (11 KB, eight workgroups per CU
    // staged whole) windows cost more than they bring (413 -> 580 us): every window is a pass of its own (ring set-up, chain, tokens
    // moved to their places).  Round 4, same file: windows of 16 / 12 / 8 / 6 / 5 / 4 / 3 KB 1 959 / 1 826 / 1 436 / 1 395 / 1 348 /
    // 1 381 / 1 448 us — the smaller the window the more workgroups a CU holds (12 at 5 KB), the more passes a block takes.
    static const int win_env = std::getenv("TCMI_SYM_WINDOW") ? std::atoi(std::getenv("TCMI_SYM_WINDOW")) : -1;      // (tests, A/B: 0 = never, else the window's bytes)
    const size_t win_bytes = per_wg == 1 ? (win_env >= 0 ? (size_t)win_env : pay > 16384 ? 5120u : 0u) : 0u;
    const bool windowed = win_bytes >= 2048 && win_bytes + 24 < pay;
    sa.win_dwords = windowed ? (uint32_t)((win_bytes / 4 + 6 + 1) & ~(size_t)1) : 0u;    // (even: the window loader stores 8 bytes a lane)
    // a window's chunks are short (5 KB over 64 lanes: 640 bits): with stretches of chunk / 4 .. chunk / 2 bits a lane decodes a third of
    // a chunk into its neighbour's before it can meet it; half as long there (2.5 : 1: 1 258 -> 1 200 us; the bench file, whole payloads: 142 -> 163)
    sa.shift_bias = windowed ? 1u : 0u;
    const size_t dyn = windowed ? (size_t)sa.win_dwords * 4 : (size_t)g.pay_dwords * 4 * per_wg;
    static const bool attr_once = [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(bgzf_symbols<2, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(160 * 1024 - sizeof(SymLds<2>)));
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(bgzf_symbols<1, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(160 * 1024 - sizeof(SymLds<1>)));
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(bgzf_symbols<1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(160 * 1024 - sizeof(SymLds<1>)));
        return true;
    }();
    (void)attr_once;
    if (report) {                               // (diagnostic) how many workgroups a compute unit really holds
        int occ = 0;
        if (per_wg == 2) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, reinterpret_cast<const void *>(bgzf_symbols<2, false>), 128, dyn);
        else if (windowed) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, reinterpret_cast<const void *>(bgzf_symbols<1, true>), 64, dyn);
        else (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, reinterpret_cast<const void *>(bgzf_symbols<1, false>), 64, dyn);
        std::fprintf(stderr, "[tcmi inflate] %zu blocks, payload %zu B + slack; bgzf_symbols<%d%s>: %zu B of LDS per workgroup, %d workgroups per CU\n",
                     nb, pay, per_wg, windowed ? ", windowed" : "", dyn + (per_wg == 2 ? sizeof(SymLds<2>) : sizeof(SymLds<1>)), occ);
    }
    tcmi_prof_begin(ctx, TCMI_K_INFLATE);
    if (per_wg == 2) hipLaunchKernelGGL((bgzf_symbols<2, false>), dim3((unsigned)((nb + 1) / 2)), dim3(128), dyn, ctx->stream, sa);
    else if (windowed) hipLaunchKernelGGL((bgzf_symbols<1, true>), dim3((unsigned)nb), dim3(64), dyn, ctx->stream, sa);
    else hipLaunchKernelGGL((bgzf_symbols<1, false>), dim3((unsigned)nb), dim3(64), dyn, ctx->stream, sa);
    tcmi_prof_end(ctx, TCMI_K_INFLATE);
    TCMI_HIP(ctx, hipGetLastError());
    *two_literals = per_wg == 1;
    return TCMI_OK;
}
