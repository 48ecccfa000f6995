// pack_bits.h — DEVICE: the bit work both packers' plane kernels share: where the packed read set goes (PackOut), 4-bit BAM codes to
// {lo, hi} bit planes (classify8, fetch32, pair_planes), the drop plane's two sources of bits (the base-quality floor, the primer mask
// with the mate join's clip) and one projected read's walk over its CIGAR (pack_read).  pack_device.hip includes it once, inside its
// unnamed namespace, behind what it needs from there (PB, NIB, PackTotals): one translation unit, so that classify_view and pack_read keep
// all their callers and every kernel the machine code it had (tools/isa_diff.sh; three translation units did not give that).
struct PackOut {
    uint32_t *lenoff;               // [n_kept]
    uint32_t *seq;                  // [word_cap]
    tcmi_fast_chunk *chunks;        // [chunk_cap]
    uint32_t *covrun;               // [n_kept]: the runs of a chunk start at its first read's index
    uint32_t *events;               // [event_cap]
    uint32_t word_cap, chunk_cap, event_cap;
    uint32_t *slack;                // 64 words behind the last array
};

__device__ inline void push_event(const PackOut &o, PackTotals *tot, uint32_t w)
{
    const uint32_t slot = atomicAdd(&tot->n_events, 1u);
    if (slot < o.event_cap) o.events[slot] = w;
}

// Any boolean function of three words in one instruction (v_bitop3_b32): TT(f) is its truth table, bit (a << 2 | b << 1 | c).  These
// kernels are bound by vector issue, and the compiler finds only some of the three-input forms by itself.
template <typename F> constexpr uint32_t truth_table(F f)
{
    uint32_t t = 0;
    for (uint32_t i = 0; i < 8; ++i) t |= (f((i >> 2) & 1u, (i >> 1) & 1u, i & 1u) & 1u) << i;
    return t;
}
#define BITOP3(a_, b_, c_, ...) ((uint32_t)__builtin_amdgcn_bitop3_b32((a_), (b_), (c_), truth_table([](uint32_t a, uint32_t b, uint32_t c) { return (__VA_ARGS__); })))

// eight 4-bit BAM codes (base k in nibble k) -> one bit per base: C|T, G|T, "is one of A C G T"
__device__ inline void classify8(uint32_t n, uint32_t &lo, uint32_t &hi, uint32_t &ok)
{
    // (bits 0, 4, .. 28 of n, n >> 1, n >> 2, n >> 3 are a base's four code bits; the other bits are masked out of `ok` and so of all three)
    const uint32_t b = n >> 1, c = n >> 2, d = n >> 3;
    const uint32_t one3 = BITOP3(n, b, c, (a ^ b ^ c) & ~(a & b & c)), none3 = BITOP3(n, b, c, ~(a | b | c));
    ok = BITOP3(one3, none3, d, c ? b : a) & NIB;               // exactly one bit set: A=1 C=2 G=4 T=8
    lo = BITOP3(b, d, ok, (a | b) & c);
    hi = BITOP3(c, d, ok, (a | b) & c);
}
__device__ inline uint32_t squeeze8(uint32_t t)                 // bits 0,4,..,28 -> bits 0..7
{
    t = (t | (t >> 3)) & 0x03030303u;
    t = (t | (t >> 6)) & 0x000F000Fu;
    return (t | (t >> 12)) & 0xFFu;
}

// bases [yy, yy + nb) of a read (nb <= 32) as bit planes; bases at or beyond l_seq are "not A/C/G/T"
__device__ inline void fetch32(const uint8_t *seq, int32_t l_seq, int32_t yy, int nb, uint32_t &lo, uint32_t &hi, uint32_t &ok)
{
    lo = hi = ok = 0;
    const int have = min(nb, l_seq - yy);
    if (have <= 0) return;
    const uintptr_t a = reinterpret_cast<uintptr_t>(seq + (yy >> 1));
    const uint32_t *q = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)(a & 3) * 8u;
    uint32_t d[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) d[k] = q[k];
    uint32_t w[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const uint32_t b = sh ? __builtin_amdgcn_alignbit(d[k + 1], d[k], sh) : d[k];
        w[k] = ((b & 0x0F0F0F0Fu) << 4) | ((b >> 4) & 0x0F0F0F0Fu);   // BAM keeps the first base of a byte in the high nibble
    }
    const bool odd = yy & 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t n = odd ? __builtin_amdgcn_alignbit(w[k + 1], w[k], 4) : w[k];
        uint32_t l, h, v;
        classify8(n, l, h, v);
        lo |= squeeze8(l) << (8 * k);
        hi |= squeeze8(h) << (8 * k);
        ok |= squeeze8(v) << (8 * k);
    }
    const uint32_t mask = have >= 32 ? 0xFFFFFFFFu : ((1u << have) - 1u);
    lo &= mask; hi &= mask; ok &= mask;
}

// 32 consecutive bases of a read that lies on the reference as it is ([H][S]M[S][H]): one unaligned 16-byte load (+ the byte behind
// it for a read whose first aligned base sits in a low nibble) -> the pair {C|T, G|T} and the "is A/C/G/T" plane.
// p: the byte that holds base y (= y0 + 32 q), odd: y is odd, have: bases of the pair the read really has (< 32: masked)
__device__ inline void pair_planes(const uint8_t *p, bool odd, int have, uint32_t &lo, uint32_t &hi, uint32_t &ok)
{
    uint32_t d[5];
    __builtin_memcpy(d, p, 16);                                 // (any byte address: unaligned access mode, one global_load_dwordx4)
    d[4] = p[16];                                               // (what lies behind a read's SEQ — its QUAL, the arrays' slack — is masked below)
    uint32_t w[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) w[k] = BITOP3(d[k] << 4, d[k] >> 4, 0xF0F0F0F0u, c ? a : b);        // BAM keeps the first base of a byte in the high nibble
    // The four words' planes (bits at 0, 4, .. 28: base 8 k + i of word k at bit 4 i) are squeezed TOGETHER: two bits per byte
    // within each word, the four words interleaved into one (byte b: bases 8 k + 2 b + e at bits 2 k + e), then the bytes'
    // 2-bit fields transposed with two masked swaps — 19 instructions a plane where four 3-step squeezes took 39, and this
    // kernel is bound by vector issue.
    uint32_t ul = 0, uh = 0, uv = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t n = odd ? __builtin_amdgcn_alignbit(w[k + 1], w[k], 4) : w[k];
        uint32_t l, h, v;
        classify8(n, l, h, v);
        ul |= BITOP3(l, l >> 3, 0x03030303u, (a | b) & c) << (2 * k);
        uh |= BITOP3(h, h >> 3, 0x03030303u, (a | b) & c) << (2 * k);
        uv |= BITOP3(v, v >> 3, 0x03030303u, (a | b) & c) << (2 * k);
    }
    auto swap_fields = [](uint32_t x, int s, uint32_t m) { const uint32_t t = BITOP3(x >> s, x, m, (a ^ b) & c); return BITOP3(x, t, t << s, a ^ b ^ c); };
    lo = swap_fields(swap_fields(ul, 12, 0x0000F0F0u), 6, 0x00CC00CCu);
    hi = swap_fields(swap_fields(uh, 12, 0x0000F0F0u), 6, 0x00CC00CCu);
    ok = swap_fields(swap_fields(uv, 12, 0x0000F0F0u), 6, 0x00CC00CCu);
    const uint32_t mask = have >= 32 ? 0xFFFFFFFFu : have > 0 ? ((1u << have) - 1u) : 0u;
    lo &= mask; hi &= mask; ok &= mask;
}

// ---- the base-quality floor (tcmi_ctx_set_min_base_quality; BQ variants of the plane kernels only) ---------------------------------
// A token whose quality is below the floor is SKIPPED (pysam's pileup_base_qual_skip): its bit is set in the read set's third plane,
// "drop" — one word per {lo, hi} pair, in an array of its own indexed by pair —, its lo / hi bits are cleared and it pushes no event
// word; tally_planes_drop_kernel counts the plane and takes it out of the coverage.
// bit i: byte i of the 32 QUAL bytes at p (any address) is below q (1 .. 255).  Unsigned bytes: 0xFF, "no QUAL", is below nothing.
__device__ inline uint32_t qual_below32(const uint8_t *p, uint32_t q)
{
    uint32_t d[8];
    __builtin_memcpy(d, p, 32);
    const uint32_t H = 0x80808080u, qq = q * 0x01010101u;
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t x = d[k];
        const uint32_t z = (x | H) - (qq & ~H);                  // bit 7 of a byte: its low seven bits are >= q's (no borrow between bytes)
        const uint32_t lt = ((~x & qq) | (~(x ^ qq) & ~z)) & H;  // x < q: the top bits say so, or they are equal and the low bits do
        m |= ((((lt >> 7) * 0x01020408u) >> 24) & 0xFu) << (4 * k);      // (the four bits gathered by one multiply: no two partial products meet)
    }
    return m;
}
// the skipped ones among the nb (<= 32) query bases from y on: below the floor, or at / beyond l_seq (quality 0)
__device__ inline uint32_t dropped32(const uint8_t *qual, int32_t l_seq, int32_t y, int nb, uint32_t q)
{
    const uint32_t nbm = nb >= 32 ? 0xFFFFFFFFu : ((1u << nb) - 1u);
    const int have = min(nb, l_seq - y);
    if (have <= 0) return nbm;
    const uint32_t hm = have >= 32 ? 0xFFFFFFFFu : ((1u << have) - 1u);
    return (qual_below32(qual + y, q) | ~hm) & nbm;             // (the load ends < 32 bytes behind the record: the stream's slack)
}

// ---- the primer mask (tcmi_ctx_set_primers; the BQ variants only) -------------------------------------------------------------------
// A second source of bits for the drop plane, chosen by column and read end instead of by QUAL byte.  Per read, once: two binary
// searches of the compiled segment lists (primer_table.h) give the masked head length and tail length, clamped to the read's columns
// (<= 1023) and packed into one word, head | tail << 10; the lanes that make the pairs turn it into bits.
using PrimerTab = tcmi_primer_tab;
// Where the searches read the table.  A search is a chain of dependent loads, about log2(n) + 2 per list: some 18 probes per read for
// an ARTIC-like scheme of a hundred amplicons.  A probe that hits L2 costs 180 - 225 cycles, one of LDS about 50, and a workgroup's 256
// reads walk the same few entries; staging the table costs the workgroup one coalesced load and one barrier.  So a workgroup stages a
// table of up to PT_LDS segments (3 KiB: the kernels keep their workgroups per CU) and searches larger ones where they lie.
constexpr int PT_LDS = 256;                 // (the search itself: pack_device.h's seg_find)
// a read of `len` columns (1 .. 1023) whose first lies at p
__device__ inline uint32_t mask_word(const int32_t *t, int32_t n_head, int32_t n_tail, int32_t p, int32_t len)
{
    const int32_t q = p + len - 1;
    const int32_t he = seg_find(t, n_head, p, p), ts = seg_find(t + 3 * n_head, n_tail, q, q + 1);
    return (uint32_t)min(max(he - p, 0), len) | ((uint32_t)min(max(q + 1 - ts, 0), len) << 10);
}
__device__ inline void stage_table(const PrimerTab &pt, int32_t *s_tab)
{
    const int n3 = 3 * (pt.n_head + pt.n_tail);
    if (n3 <= 3 * PT_LDS) for (int i = threadIdx.x; i < n3; i += PB) s_tab[i] = pt.seg[i];
}
__device__ inline uint32_t mask_word_of(const PrimerTab &pt, const int32_t *s_tab, int32_t p, int32_t len)
{
    if (pt.n_head + pt.n_tail == 0) return 0u;
    if (pt.n_head + pt.n_tail <= PT_LDS) return mask_word(s_tab, pt.n_head, pt.n_tail, p, len);
    return mask_word(pt.seg, pt.n_head, pt.n_tail, p, len);
}
// the mate join's clip (mate_join.hip; clip == nullptr: the setting is off) raises the head part of a read's mask word: the read's
// first clip[record] columns are its mate's — merged AFTER the read was asked whether the primer table masks it (n_masked)
__device__ inline uint32_t clip_merge(uint32_t mw, const uint32_t *clip, uint64_t record, uint32_t len)
{
    if (!clip) return mw;
    return (mw & ~1023u) | min(max(mw & 1023u, clip[record]), len);
}
// one ballot over the lanes that are here and one atomic per wavefront that holds a masked read (as filter_view counts)
__device__ inline void count_masked(bool masked, PackTotals *tot)
{
    const unsigned long long m = __ballot(masked);
    if (masked && (int)(threadIdx.x & 63) == (int)__builtin_ctzll(m)) atomicAdd(&tot->n_masked, (uint32_t)__popcll(m));
}
__device__ inline uint32_t low_bits(int n) { return n <= 0 ? 0u : n >= 32 ? 0xFFFFFFFFu : (1u << n) - 1u; }
// the masked ones among the nb (<= 32) columns from c0 on, of a read of `len` columns under the mask word mw
__device__ inline uint32_t masked32(uint32_t mw, int len, int c0, int nb)
{
    const int head = (int)(mw & 1023u), keep_end = len - (int)(mw >> 10);
    return (low_bits(head - c0) | ~low_bits(keep_end - c0)) & low_bits(nb);
}
// the skipped tokens of nb matched bases: query bases from y on, on columns from c0 on — the floor (Q = 0: none, and then a query
// index at or beyond l_seq is NOT skipped) or the mask
__device__ inline uint32_t skipped32(const uint8_t *qual, int32_t l_seq, int32_t y, int nb, uint32_t Q, uint32_t mw, int len, int c0)
{
    uint32_t d = Q ? dropped32(qual, l_seq, y, nb, Q) : 0u;
    if (mw) d |= masked32(mw, len, c0, nb);
    return d;
}

// one PROJECTED read (anything but [H][S]M[S][H]) -> its plane pairs (out: 2 * ceil(len / 32) words, then the zero pair) and its event words
// BQ: and its drop words (dout: one per pair, then the zero word), under the floor Q — a D / N token is tested with the quality of
// the next query base (the query index at which the op starts), the I mark belongs to the token in front of the insertion — and under
// the read's primer mask mw (mask_word), column by column: a D / N op that crosses the mask's edge loses only its masked columns
template <bool BQ>
__device__ inline void pack_read(const ReadView &v, const PackOut &o, PackTotals *tot, uint32_t info, int32_t gpos, uint32_t *out, uint32_t *dout, uint32_t Q,
                                 [[maybe_unused]] uint32_t mw)
{
    const int len = (int)(info & 1023u), npair = (len + 31) >> 5;
    const uint8_t *qual = v.seq + ((size_t)v.l_seq + 1) / 2;
    {
        // Walk the CIGAR: matched bases land on their reference offset (bit-field copies into the pair being built), D / N
        // leave empty positions, and the tokens that are not plain bases become events: X for a deleted base
        // whose token is exactly "*", I on the last reference base before an insertion (also "*+..": I but not X).
        int q_cur = 0;
        uint32_t lo = 0, hi = 0, ok = 0;
        uint32_t dr = 0;                            // (BQ) the pair's skipped tokens: they are in `ok` too — no OTHER event for them
        auto flush_to = [&](int q_new) {            // store the pairs [q_cur, q_new), all but the first of them empty
            while (q_cur < q_new && q_cur < npair) {
                const int nb = min(32, len - 32 * q_cur);
                *reinterpret_cast<uint2 *>(out + 2 * q_cur) = make_uint2(lo, hi);
                if constexpr (BQ) { dout[q_cur] = dr; dr = 0; }
                uint32_t miss = (nb >= 32 ? 0xFFFFFFFFu : ((1u << nb) - 1u)) & ~ok;
                while (miss) {
                    const int b = __builtin_ctz(miss);
                    push_event(o, tot, (uint32_t)(gpos + 32 * q_cur + b) | TCMI_F_EV_OTHER);
                    miss &= miss - 1;
                }
                lo = hi = ok = 0;
                ++q_cur;
            }
        };
        int x = 0, y = 0;
        for (uint32_t k = 0; k < v.n_cigar && x < len; ++k) {
            const uint32_t c = ld_u32(v.cigar + 4 * (size_t)k), op = c & 0xFu;
            const int oplen = (int)(c >> 4);
            if (consumes_ref(op)) {
                const bool ins = oplen > 0 && ins_after(v.cigar, v.n_cigar, k);
                bool skip_last = false;             // (BQ) the op's last token is skipped: no I mark
                if (is_match(op)) {
                    int t = 0;
                    while (t < oplen) {
                        const int q = (x + t) >> 5, b0 = (x + t) & 31, nb = min(32 - b0, oplen - t);
                        flush_to(q);
                        uint32_t l, h, g;
                        fetch32(v.seq, v.l_seq, y + t, nb, l, h, g);
                        if constexpr (BQ) {
                            const uint32_t d = skipped32(qual, v.l_seq, y + t, nb, Q, mw, len, x + t);
                            l &= ~d; h &= ~d; g |= d;
                            dr |= d << b0;
                            skip_last = (d >> (nb - 1)) & 1u;
                        }
                        lo |= l << b0; hi |= h << b0; ok |= g << b0;
                        t += nb;
                    }
                } else {
                    if constexpr (BQ) {
                        // the floor skips every column of the op or none; the mask skips the op's masked columns: no OTHER event, no
                        // X event and no coverage there, and no I mark when the op's last column is skipped
                        const bool below = Q && (y < v.l_seq ? byte_at(qual + y) : 0u) < Q;     // (qual_at written out: the call changes the two BQ kernels' code)
                        const int head = (int)(mw & 1023u), keep_end = len - (int)(mw >> 10);
                        const int x1 = min(x + oplen, len);
                        if (below || x < head || x1 > keep_end) {
                            for (int t = 0; x + t < x1;) {
                                const int q = (x + t) >> 5, b0 = (x + t) & 31, nb = min(32 - b0, x1 - x - t);
                                flush_to(q);
                                const uint32_t m = (below ? low_bits(nb) : masked32(mw, len, x + t, nb)) << b0;
                                dr |= m; ok |= m;
                                t += nb;
                            }
                        }
                        auto gone = [&](int c) { return below || c < head || c >= keep_end; };
                        skip_last = gone(x + oplen - 1);
                        if (op == 2) {
                            const int nx = ins ? oplen - 1 : oplen;
                            for (int t = 0; t < nx; ++t) if (!gone(x + t)) push_event(o, tot, (uint32_t)(gpos + x + t) | TCMI_F_EV_X);
                        }
                    } else if (op == 2) {
                        const int nx = ins ? oplen - 1 : oplen;
                        for (int t = 0; t < nx; ++t) push_event(o, tot, (uint32_t)(gpos + x + t) | TCMI_F_EV_X);
                    }
                }
                if (ins && !skip_last) push_event(o, tot, (uint32_t)(gpos + x + oplen - 1) | TCMI_F_EV_I);
                x += oplen;
            }
            if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) y += oplen;     // (consumes_query, written out: the call changes pk_place's code)
        }
        flush_to(npair);
    }
    *reinterpret_cast<uint2 *>(out + 2 * npair) = make_uint2(0u, 0u);
    if constexpr (BQ) dout[npair] = 0u;
}

// places of the LDS list "read t, pair q" a plane kernel's workgroup keeps for its PB reads (planes_body, place_body): a read's pairs,
// its zero pair, and the second one that ends it on 16 bytes
constexpr int PL_SLOTS = PB * (TCMI_D_MAXLEN / 32 + 2);
