// pack_caps.h — what the device packer (pack_device.hip) and the code that feeds it (bam_device.hip) must agree on before a kernel runs:
// the flags a packer declines with, the capacities the one-sync packer is queued from, the pinned buffer its report fills, and the
// arrays each packer takes from the context's arena.  Plain C++: no HIP header, so a program of the tests builds it alone
// (tests/pack_caps_main.cpp).  tcmi_internal.h includes it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "readset_layout.h"

// ---- why a packer declined: PackTotals.flags, *why of tcmi_pack_on_device / tcmi_pack_fused_finish, the stat "one_sync_last_decline_flags"
enum { PKF_LONG = 1, PKF_FARPOS = 2, PKF_BADREAD = 4, PKF_EVENT_OVF = 8, PKF_CHUNK_OVF = 16, PKF_HEADER_OVF = 32, PKF_WORD_OVF = 64,
       PKF_MULTIREF = 128, PKF_SLOT_OVF = 1u << 13 /* a kept read ends past its contig's slot (tcmi_ctx_set_layout) */ };
constexpr uint32_t PKF_CHAIN = 256, PKF_STAT = 512, PKF_REC_OVF = 2048;       // (the one-sync path's: pk_index, pk_place)

// ---- chunks, events and plane words: the rule both packers size their read set by ----------------------------------------------------
constexpr int PK_BLOCK = 256;                    // lanes per workgroup of the packers' kernels (pack_device.hip: PB)
constexpr int PK_CMAX = 1024;                    // most reads one pk_pack workgroup takes
constexpr int64_t PK_LONG_CHUNK = 2048;          // reads per workgroup the rule aims for without balancing
// plane words around the reads' own: the zero pair in front of the first read, and what the last stage's last 16-byte load takes along
constexpr uint32_t PK_WORD_SLACK = 2 + 16;
constexpr uint64_t PK_WORD_MOST = 0xF0000000ull; // (word offsets are 32 bits)
constexpr int64_t PK_REC_MOST = 0x7FFFFFF0ll;

// what a packer sizes its read set and pk_pack's launch by: records (kept reads), plane words, chunks, events; pk_pack's grid and — from
// an exact count only: from a capacity the kernel works it out itself, dev_slots > 0 — its reads per workgroup
struct PkCaps { int64_t rec_cap; uint64_t word_cap; uint32_t chunk_cap, event_cap; int64_t n_wg, reads_per_wg; };
// n: the kept reads — exact (the host has read the count back), or a capacity: then the grid is at least the workgroups the
// reads-per-workgroup rule leaves for ANY number of kept reads up to n.  slots: the tally kernel's resident workgroups; balance: long
// chunks, but a multiple of `slots` of them, as the host packer cuts them; reach: positions the reads may reach.
static inline PkCaps pk_chunk_rule(int64_t n, uint64_t word_cap, bool exact, int64_t slots, bool balance, int64_t reach)
{
    PkCaps c = {n, word_cap, 0, 0, 0, 0};
    const int64_t full = (n + PK_CMAX - 1) / PK_CMAX;
    if (exact) c.reads_per_wg = std::min<int64_t>(balance ? tcmi_balanced_chunk(n, slots) : PK_LONG_CHUNK, PK_CMAX);
    if (exact) c.n_wg = (n + c.reads_per_wg - 1) / c.reads_per_wg;
    else c.n_wg = balance ? std::max<int64_t>(tcmi_balance_rounds(n, slots) * slots, full) : full + (n + PK_LONG_CHUNK - 1) / PK_LONG_CHUNK;
    // every workgroup opens at least one chunk; more when a window or a lane's 255-read budget runs out
    c.chunk_cap = (uint32_t)std::min<int64_t>(n, 4 * c.n_wg + reach / 128 + 64);
    c.event_cap = (uint32_t)std::min<int64_t>(PK_REC_MOST, std::max<int64_t>(1 << 20, n / 2));
    return c;
}

// ---- the one-sync packer's capacities: what its arrays are sized for before anybody has seen the file ---------------------------------
// (a file beyond one of them takes the several-kernel path; tests/capacity_files.py writes one per rung and restates the rules)
// records of a stream of `inflated` bytes: a record takes at least 36 of them; the arena is reserved for records of >= 64 bytes
// (block_size + 32 fixed bytes + name + CIGAR + SEQ + QUAL of a 15-base read) — it cannot grow under live data
static inline int64_t pk_most_records(uint64_t inflated) { return (int64_t)(inflated / 36 + 16); }
static inline int64_t pk_guess_records(uint64_t inflated) { return std::min<int64_t>(pk_most_records(inflated), (int64_t)(inflated / 64 + 1024)); }
// hint: the mean size of the file's first records as the host saw them (< 36: none); safe_caps: sized as the arena was reserved, not
// from the hint; len_bound: positions the reads may reach.  rec_cap beyond PK_REC_MOST, word_cap beyond PK_WORD_MOST: not for this packer.
static inline PkCaps pk_one_sync_caps(uint64_t inflated, uint32_t hint, bool safe_caps, int64_t len_bound, int64_t slots, bool balance)
{
    int64_t rec = pk_guess_records(inflated);
    if (hint >= 36 && !safe_caps) rec = std::min<int64_t>(rec, (int64_t)(inflated / hint) * 5 / 4 + 8192);     // (+ 25 %)
    // words: a read of len positions takes <= len / 16 + 7 words, and a read without long deletions / skips has len <= l_seq, each base
    // of which takes 1.5 bytes of the stream (others overflow the capacity: PKF_WORD_OVF, the other path)
    return pk_chunk_rule(rec, inflated / 24 + 8ull * (uint64_t)rec + 64, false, slots, balance, len_bound);
}
// did the totals fit?  -> the PKF_*_OVF flags of what did not
static inline uint32_t pk_beyond_caps(const PkCaps &c, uint64_t n_rec, uint64_t n_words, uint32_t n_chunks, uint32_t n_events)
{
    return (n_rec > (uint64_t)c.rec_cap ? PKF_REC_OVF : 0u) | (n_words + PK_WORD_SLACK > c.word_cap ? (uint32_t)PKF_WORD_OVF : 0u) |
           (n_chunks > c.chunk_cap ? (uint32_t)PKF_CHUNK_OVF : 0u) | (n_events > c.event_cap ? (uint32_t)PKF_EVENT_OVF : 0u);
}

// ---- the pinned buffer the packers' totals come back in, as byte offsets -----------------------------------------------------------------
// PackTotals | blk_alg [n_blocks] | blk_end [n_blocks] | stat [n_blocks] | the mate join's four counters, the duplicate rule's four behind
// them  (pk_report fills it; the several-kernel packer copies its totals and counters to the same places, n_blocks = 0)
constexpr size_t PK_TOTALS_BYTES = 104;          // sizeof(PackTotals) (pack_device.hip)
struct ReportPin {
    size_t alg, end, stat, mate, dup, bytes;
    explicit ReportPin(int64_t nb) : alg(tcmi_align256(PK_TOTALS_BYTES)), end(alg + tcmi_align256((size_t)nb * 8)), stat(end + tcmi_align256((size_t)nb * 4)),
                                     mate(stat + tcmi_align256((size_t)nb * 4)), dup(mate + 32), bytes(mate + 256) {}
};

// ---- the packers' arena scratch ----------------------------------------------------------------------------------------------------------
// A packer's arrays, listed ONCE, in the order they are taken: bytes[i] of array i (0: not taken under these settings).  `end` sums
// them as the arena would hand them out (tcmi_arena_take: every piece starts on 256 bytes), for the reservation and for the check in
// front of a take; `take` takes them.  Some arrays are taken later than others — a count comes back from the device in between —: both
// passes go over a range [from, to) of the list.
static inline size_t tcmi_mate_slots(size_t rec_cap) { size_t s = 1024; while (s < 2 * rec_cap) s <<= 1; return s; }
// the mate join's table {tag << 32 | record + 1} [slots] and, behind it, its four counters: one memset zeroes both
static inline size_t tcmi_mate_table_bytes(size_t rec_cap) { return tcmi_mate_slots(rec_cap) * 8 + 256; }
// the duplicate rule's table (dedup.hip): {tag << 32 | leader + 1} [slots] | best [slots], 8 bytes each | its four counters | the
// templates per slot [slots], 4 bytes each: one memset zeroes all of it
static inline size_t tcmi_dup_table_bytes(size_t rec_cap) { return tcmi_align256(tcmi_mate_slots(rec_cap) * 20 + 32); }
constexpr size_t TCMI_DUP_END_BYTES = 16;       // sizeof(tcmi_dup_end) (dedup_rule.h)

template <int N> struct PkScratch {
    size_t bytes[N] = {};
    void *p[N] = {};
    void set(int i, size_t elem, size_t count) { bytes[i] = elem * count; }
    size_t end(size_t used, int from = 0, int to = N) const
    {
        for (int i = from; i < to; ++i)
            if (bytes[i]) used = tcmi_align256(used) + bytes[i];
        return used;
    }
    template <class Take> void take(Take &&arena_take, int from = 0, int to = N)
    {
        for (int i = from; i < to; ++i) p[i] = bytes[i] ? arena_take(bytes[i]) : nullptr;
    }
    template <class T> T *at(int i) const { return static_cast<T *>(p[i]); }
};

// The several-kernel packer (tcmi_pack_on_device): 24 bytes a record (+ 4 and the record index's 8 from a stream, + the mate join's, + the
// duplicate rule's: the join's, mate_idx[], ends[], slot_of[], dup[] and its own table) and
// 20 per 256 of them while it classifies; 24 per KEPT read once the host knows how many there are.
enum { SK_REC_OFF,                                                              // a stream's record index (bam_device.hip: decode_on_device)
       SK_INFO, SK_RD_SEQ, SK_RD_POS, SK_BLK_SUM, SK_BLK_ALG, SK_BLK_END, SK_TOT, SK_GEN_IDX,   // pk_classify, pk_scan
       SK_MATE_TABLE, SK_CLIP,                                                  // the mate join
       SK_MATE_IDX, SK_DUP_ENDS, SK_DUP_SLOT, SK_DUP, SK_DUP_TABLE,             // the duplicate rule (the join's two as well)
       SK_C_IDX, SK_C_POS, SK_C_INFO, SK_C_WOFF, SK_C_SEQ,                      // pk_scatter: the kept reads, compacted
       SK_N };
static inline void pk_several_kept(PkScratch<SK_N> &s, int64_t nf)
{
    for (int i : {SK_C_IDX, SK_C_POS, SK_C_INFO, SK_C_WOFF}) s.set(i, 4, (size_t)nf);
    s.set(SK_C_SEQ, 8, (size_t)nf);
}
// the duplicate rule's arrays for `cap` records, from list index `first` (SK_MATE_IDX / OS_MATE_IDX) on
template <int N> static inline void pk_dedup_scratch(PkScratch<N> &s, int first, size_t cap)
{
    s.set(first, 4, cap + 1); s.set(first + 1, TCMI_DUP_END_BYTES, cap + 1); s.set(first + 2, 4, cap + 1); s.set(first + 3, 1, cap + 1);
    s.set(first + 4, 1, tcmi_dup_table_bytes(cap));
}
// n records (every one of them kept, until pk_several_kept says how many are); mode: 0 flat arrays, 1 a stream; mate: the join's
// arrays (the mate rule or the duplicate rule is on); dedup: the duplicate rule's
static inline PkScratch<SK_N> pk_several_scratch(int64_t n, int mode, bool mate, bool dedup = false)
{
    PkScratch<SK_N> s;
    const size_t n1 = (size_t)std::max<int64_t>(n, 1), blk1 = (size_t)std::max<int64_t>((n + PK_BLOCK - 1) / PK_BLOCK, 1);
    if (mode == 1) s.set(SK_REC_OFF, 1, tcmi_align256((size_t)n * 8 + 8));
    s.set(SK_INFO, 4, n1); s.set(SK_RD_SEQ, 8, n1); s.set(SK_RD_POS, 4, n1);
    s.set(SK_BLK_SUM, 8, blk1); s.set(SK_BLK_ALG, 8, blk1); s.set(SK_BLK_END, 4, blk1);
    s.set(SK_TOT, PK_TOTALS_BYTES, 1);
    if (mode == 1) s.set(SK_GEN_IDX, 4, n1);
    if ((mate || dedup) && n > 0) { s.set(SK_MATE_TABLE, 1, tcmi_mate_table_bytes((size_t)n)); s.set(SK_CLIP, 4, (size_t)n + 1); }
    if (dedup && n > 0) pk_dedup_scratch(s, SK_MATE_IDX, (size_t)n);
    pk_several_kept(s, n);
    return s;
}

// The one-sync packer (tcmi_pack_fused_enqueue): 52 bytes a record of the capacity (+ the mate join's, + the duplicate rule's) and 32 a BGZF block (+ 24 when
// pk_prefix makes the blocks' prefix sums).
enum { OS_AGG, OS_FN, OS_REC_BASE, OS_RREC, OS_BLK_ALG, OS_BLK_END, OS_TOT, OS_PRE, OS_REC_OFF, OS_C_IDX, OS_C_POS, OS_C_INFO, OS_C_WOFF, OS_C_SEQ,
       OS_GEN_IDX, OS_MATE_TABLE, OS_CLIP, OS_MATE_IDX, OS_DUP_ENDS, OS_DUP_SLOT, OS_DUP, OS_DUP_TABLE, OS_N };
// (every workgroup adds up what lies in front of its block: a few thousand words for a 1M-read file, but quadratic in the blocks — at
//  67 000 blocks, a 4 GiB stream, it was 40 % of these kernels' time: from 16 384 blocks on three small scan launches do it;
//  option "prefix_kernels": > 0 always, < 0 never)
static inline bool pk_prefix_on(int option, int64_t nb) { return option > 0 || (option == 0 && nb >= 16384); }
static inline size_t pk_prefix_words(int64_t nb) { return tcmi_align256(((size_t)nb + 1) * 8) / 8; }     // of each of pk_prefix's three arrays
static inline PkScratch<OS_N> pk_one_sync_scratch(int64_t rec_cap, int64_t nb, bool mate, bool prefix, bool dedup = false)
{
    PkScratch<OS_N> s;
    const size_t cap = (size_t)rec_cap, b = (size_t)nb;
    s.set(OS_AGG, 8, b); s.set(OS_FN, 8, b); s.set(OS_REC_BASE, 4, b);
    s.set(OS_RREC, 16, cap);
    s.set(OS_BLK_ALG, 8, b); s.set(OS_BLK_END, 4, b);
    s.set(OS_TOT, PK_TOTALS_BYTES, 1);
    if (prefix) s.set(OS_PRE, 8, 3 * pk_prefix_words(nb));
    s.set(OS_REC_OFF, 8, cap + 1);
    for (int i : {OS_C_IDX, OS_C_POS, OS_C_INFO, OS_C_WOFF}) s.set(i, 4, cap);
    s.set(OS_C_SEQ, 8, cap);
    s.set(OS_GEN_IDX, 4, cap);
    if (mate || dedup) { s.set(OS_MATE_TABLE, 1, tcmi_mate_table_bytes(cap)); s.set(OS_CLIP, 4, cap + 1); }
    if (dedup) pk_dedup_scratch(s, OS_MATE_IDX, cap);
    return s;
}
