// readset_layout.h — the packed read set as the tally kernels take it, and the geometry of its chunks.  Plain C++: no HIP header, so
// the host packer (host_pack.cpp) and a program around it build without one.  tcmi_internal.h includes it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

static inline size_t tcmi_align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }     // the pieces of device buffers start on 256 bytes

// ---- several contigs on one coordinate axis (tcmi_ctx_set_layout) --------------------------------------------------
// Reference t's reads pile up at pos + shift[t]; shift[t] < 0: they do not pile up (a reference the caller has no record of);
// a kept read must end at or before end[t] = shift[t] + slot_len[t].  No layout (n() == 0): reference 0 at 0, nothing else.
// The one rule of the host packer (host_pack.cpp) and the host insert sweep (insert_tokens.cpp); the kernels read the same
// table on the device (pack_device.h: shift_of).
struct tcmi_layout {
    std::vector<int64_t> shift, end;
    int32_t n() const { return (int32_t)shift.size(); }
    int64_t shift_of(int32_t tid) const
    {
        if (shift.empty()) return tid == 0 ? 0 : -1;
        return tid >= 0 && tid < n() ? shift[(size_t)tid] : -1;
    }
    int64_t end_of(int32_t tid) const { return shift.empty() ? INT64_MAX : end[(size_t)tid]; }
};

// ---- device read layout -------------------------------------------------------------
// Only reads that pile up (mapped, tid == 0, pos >= 0, reference span > 0)
// are kept, in two sets:
//
//  * ALIGNED set (tally_planes.hip) — every read of every BASELINE config.  A read whose CIGAR is one run
//    of match ops (M / = / X, optionally flanked by S / H clips) is taken as it is; any other CIGAR is
//    PROJECTED onto the reference while it is packed: matched bases land on their reference offset,
//    deleted / skipped positions stay empty, inserted and clipped bases are dropped, and the tokens that
//    are not plain bases ("*", "..+n..") become EVENT words (position | kind) that the tail blocks of the
//    same launch count.  Per entry ONE packed header word (position - window start | len << 10 | pair
//    offset from the stage's first word << 20) and the bases as codes A=0 C=1 G=2 T=3 (anything else 0),
//    32 bases per pair of words {lo plane, hi plane}, one zero pair in front of every read and behind the
//    last of a chunk: 4 + 8*ceil(l/32) + 8 bytes, 52 for a 150-bp read.
//    "Anything else" (N, IUPAC, '=', base beyond SEQ, deleted / skipped positions) is exactly what
//    indexing.py:115-132 puts in no class; those positions are listed as OTHER event words (they
//    count toward coverage but toward no class).
//    Consecutive reads are grouped into CHUNKS (window <= TCMI_F_MAXW grid words of 8 positions,
//    <= 255 reads per lane); one workgroup tallies one chunk in STAGES of <= sub_reads reads.
//    Packed on the DEVICE from the BAM-native arrays (pack_device.hip: sorted input, entries of
//    <= TCMI_D_MAXLEN positions) or on the HOST (host_pack.cpp: anything, long reads in pieces of
//    TCMI_F_SEG positions, re-sorted).
//  * GENERAL set (CIGAR-walk kernel, tally.hip): what the aligned path does not take (positions >= 2^29,
//    reads with indels under option project_reads = 0, or everything under option tally_variant = 1;
//    the tests use these to cross-check independent implementations), in ROUNDS of TCMI_ROUND reads with
//    per-round offset tables, raw 4-bit codes.
//
// The algorithmic bytes of SURVEY 8-d are 12 + 4*n_cigar + ceil(l/2) per read: 91 for a 150-bp read.
#define TCMI_ROUND 256
#ifndef TCMI_F_BLOCK
#define TCMI_F_BLOCK 256           // lanes per workgroup of the fast kernel (256 or 512; 256 measured faster)
#endif
#define TCMI_F_MAXW 96             // max grid words (8 positions each) in a chunk window
#define TCMI_F_MAXSPAN 600         // longest aligned read the fast kernel takes in one piece
#define TCMI_F_SEG 512             // projected reads longer than this are cut into pieces of this many positions
#define TCMI_D_MAXLEN 512          // longest entry the device packer takes (a window holds MAXW * 8 = 768 positions)
#ifndef TCMI_F_SEQCAP
#define TCMI_F_SEQCAP 6144         // LDS words for staged bases
#endif
#define TCMI_F_MAXSTAGE 8          // stages per chunk
#ifndef TCMI_P_NPL
#define TCMI_P_NPL 8               // counter planes per lane: a lane counts <= 2^NPL - 1 reads per chunk
#endif
#ifndef TCMI_P_WAVES
#define TCMI_P_WAVES 4             // workgroups per CU the kernel's register budget is set for
#endif
#ifndef TCMI_P_SUB
#define TCMI_P_SUB 512             // max reads staged in LDS at a time
#endif
// event word = reference position | kind; kinds may be combined
#define TCMI_F_EVPOS   (1u << 29)  // positions must stay below this for the fast path
#define TCMI_F_EV_OTHER (1u << 29) // a covered position whose token is no A/C/G/T base: was counted as T by subtraction
#define TCMI_F_EV_X     (1u << 30) // token "*"
#define TCMI_F_EV_I     (1u << 31) // token carries an insertion

struct tcmi_fast_chunk {           // 80 bytes
    int64_t read0;                 // first read (index into f_pos / f_lenoff)
    int64_t word0;                 // first word of the chunk's base stream (multiple of 4)
    int32_t n_reads;
    int32_t P0;                    // window start, multiple of 8
    int32_t Wn;                    // window length in grid words
    int32_t sub_reads;             // reads per stage (<= TCMI_P_SUB)
    int32_t stage_end[TCMI_F_MAXSTAGE];   // word offset (from word0) one past stage i, trailing pad included;
                                          // stage i starts at stage_end[i-1] - pad (0 for i = 0)
    // the chunk's coverage as runs of reads with equal (position, length), words of d_fcovrun:
    // position - P0 | len << 10 | (reads in the run, <= 4095) << 20
    int64_t run0;
    int32_t n_runs;
    int32_t reserved_;
};

// ---- chunk geometry: the host's one copy (the host packer, the device packer's launch code); pk_pack keeps device twins -------------
// Reads in the longest chunk the balancing rule aims for: TCMI_F_MAXSTAGE stages of ~ 400 reads (5 000x / 150 bp).
constexpr int64_t TCMI_F_LONGEST = (int64_t)TCMI_F_MAXSTAGE * 400;
// Long chunks (the spread / reduce epilogue is paid once per chunk), but k * slots of them for `slots` resident workgroups — with 2 315
// chunks on 1 024 slots the third round of workgroups ran a quarter full.  -> k, and the reads per chunk that give k * slots chunks.
static inline int64_t tcmi_balance_rounds(int64_t nf, int64_t slots)
{
    return std::max<int64_t>(1, (nf + slots * TCMI_F_LONGEST - 1) / (slots * TCMI_F_LONGEST));
}
static inline int64_t tcmi_balanced_chunk(int64_t nf, int64_t slots)
{
    const int64_t k = tcmi_balance_rounds(nf, slots);
    return std::max<int64_t>(64, (nf + k * slots - 1) / (k * slots));
}
// words of one read of `len` positions in the base stream, trailing zero pair included
static inline int64_t tcmi_read_words(int64_t len) { return 2 * ((len + 31) / 32) + 2; }
// Lanes own 32 positions: the kernel splits a stage over S = TCMI_F_BLOCK / ceil(window / 32) depth slices (it keeps at least two
// lane groups).
static inline int64_t tcmi_stage_slices(int64_t words) { return TCMI_F_BLOCK / std::max<int64_t>(2, (words * 8 + 31) / 32); }
// Stage size for a window of `words` grid words and reads of <= maxnw grid words: the kernel's inner loop takes bodies of 8 reads per
// lane and one of 4, so a stage of S * 4 * m reads wastes none.  Fill the stage buffer (2 = the zero pair in front of a chunk's first
// read); stage_cap > 0 bounds it (experiments).
static inline int64_t tcmi_stage_reads(int64_t words, int64_t maxnw, int64_t stage_cap)
{
    const int64_t S = tcmi_stage_slices(words);
    int64_t cap = std::min<int64_t>(TCMI_P_SUB, (TCMI_F_SEQCAP - 16 - 2) / tcmi_read_words(maxnw * 8));
    if (stage_cap > 0) cap = std::min<int64_t>(cap, std::max<int64_t>(stage_cap, S * 4));
    int64_t sub = S * 4 * std::max<int64_t>(1, cap / (S * 4));
    if (sub > cap) sub = std::max<int64_t>(S, cap / S * S);
    return sub;
}
// reads of a chunk: whole stages, <= 2^planes - 1 reads per lane, at most balanced_cap
static inline int64_t tcmi_chunk_reads(int64_t sub, int64_t words, int64_t n_stages, int64_t balanced_cap)
{
    const int64_t S = tcmi_stage_slices(words);
    const int64_t whole = std::max<int64_t>(sub, std::min<int64_t>(((1 << TCMI_P_NPL) - 1) * S, n_stages * sub) / sub * sub);
    return std::min(whole, balanced_cap);
}
