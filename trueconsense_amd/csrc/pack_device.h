// pack_device.h — DEVICE (.hip files only): one read as every kernel that goes to the reads themselves sees it, whether it lies in the
// flat arrays of struct tcmi_reads or in the inflated BAM stream (SAM spec §4.2) — the packers (pack_device.hip), the insert-candidate
// kernels (ins_entries.hip), the long-read tally (tally.hip: tally_stream_kernel) and the counting kernels (amplicon_reads.hip,
// strand_counts.hip, link_counts.hip; their host side and their frame: stream_count.h) — and the wave join, which the packer uses too.
// What only the packers use stays in pack_device.hip.
#pragma once
#include "cigar_rule.h"
#include "tcmi_internal.h"

namespace {

using PackSrc = tcmi_pack_src;

// the decoded stream a read set left in its context's arena, as a record source (the caller has checked arena_epoch)
inline PackSrc stream_src(const tcmi_readset *rs)
{
    PackSrc s = {};
    s.stream = rs->d_stream; s.rec_off = rs->d_rec_off; s.mode = 1; s.n = rs->n_reads;
    tcmi_rules_args(s, rs->rules);              // (the filter and the floor the read set was built under)
    return s;
}

struct ReadView {
    int32_t tid, pos, l_seq;
    uint32_t flag, n_cigar;
    uint32_t mapq;              // (flat arrays carry none: 255)
    const uint8_t *cigar;       // n_cigar little-endian words, not necessarily aligned
    const uint8_t *seq;         // ceil(l_seq / 2) bytes
    bool bad;                   // inconsistent offsets / lengths
    bool broken;                // ... of a BAM record (any record, mapped or not: the file is not a BAM file then)
};

__device__ inline uint32_t ld_u32(const uint8_t *p)
{
    uint32_t w;                                 // (the record fields of a BAM stream sit at any byte offset: one unaligned dword load)
    __builtin_memcpy(&w, p, 4);
    return w;
}

// a record of the inflated BAM stream, `rec` at its block_size field (any byte address)
__device__ inline ReadView view_rec(const uint8_t *rec)
{
    ReadView v;
    v.bad = false;
    v.broken = false;
    const uint8_t *r = rec + 4;                             // behind block_size
    // the fixed fields in two loads at the record's own (any) byte address — unaligned access mode; twelve aligned dword loads
    // and funnel shifts kept the kernel waiting on the address unit: every lane's record lies in a cache line of its own
    uint32_t h[6];                                         // block_size, refID, pos, l_read_name|mapq|bin, n_cigar_op|flag, l_seq
    __builtin_memcpy(h, r - 4, 16);
    __builtin_memcpy(h + 4, r + 12, 8);
    v.tid = (int32_t)h[1];
    v.pos = (int32_t)h[2];
    const uint32_t w2 = h[3], w3 = h[4];
    const uint32_t l_name = w2 & 0xFFu;
    v.mapq = (w2 >> 8) & 0xFFu;
    v.n_cigar = w3 & 0xFFFFu;
    v.flag = w3 >> 16;
    v.l_seq = (int32_t)h[5];
    // The record walk only checked block_size itself: the variable-length fields must fit into it (what bam_reader.cpp's
    // "alignment record fields overrun block_size" refuses) — a forged l_seq or n_cigar_op would otherwise send the kernels
    // that follow the CIGAR and the bases far behind the record, or behind the stream.
    const uint32_t block_size = h[0];
    const uint64_t need = 32ull + l_name + 4ull * v.n_cigar + ((uint64_t)(uint32_t)v.l_seq + 1) / 2 + (uint64_t)(uint32_t)v.l_seq;
    v.bad = v.l_seq < 0 || l_name == 0 || need > block_size;
    v.broken = v.bad;
    if (v.bad) v.n_cigar = 0;
    v.cigar = r + 32 + l_name;
    v.seq = v.cigar + 4 * (size_t)v.n_cigar;
    return v;
}

__device__ inline ReadView view(const PackSrc &s, int64_t i)
{
    ReadView v;
    v.bad = false;
    v.broken = false;
    if (s.mode == 0) {
        v.tid = s.tid ? s.tid[i] : 0;
        v.pos = s.pos[i];
        v.l_seq = s.l_qseq[i];
        v.flag = s.flag[i];
        v.mapq = 255u;
        const uint64_t c0 = s.cigar_off[i], c1 = s.cigar_off[i + 1], q0 = s.seq_off[i], q1 = s.seq_off[i + 1];
        v.bad = c1 < c0 || c1 - c0 > 65535u || q1 < q0 || v.l_seq < 0 || (int64_t)(q1 - q0) < ((int64_t)v.l_seq + 1) / 2;
        v.n_cigar = v.bad ? 0u : (uint32_t)(c1 - c0);
        v.cigar = reinterpret_cast<const uint8_t *>(s.cigar + c0);
        v.seq = s.seq + q0;
    } else v = view_rec(s.stream + s.rec_off[i]);
    return v;
}

// the read filter (tcmi_ctx_set_read_filter): a record that fails is ignored wherever an unmapped one is
__device__ inline bool filter_on(const tcmi_filter_words &f) { return (f.flags | f.min_mapq) != 0u; }
__device__ inline bool passes(const tcmi_filter_words &f, const ReadView &v)
{
    return (v.flag & f.flags & 0xFFFFu) == (f.flags >> 16) && v.mapq >= f.min_mapq;
}

__device__ inline uint32_t nib_at(const uint8_t *seq, int32_t q)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(seq + (q >> 1));
    const uint32_t w = *reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3) >> ((a & 3) * 8);
    return (q & 1) ? (w & 15u) : ((w >> 4) & 15u);
}
__device__ inline uint32_t byte_at(const uint8_t *p)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    return (*reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3) >> ((a & 3) * 8)) & 0xFFu;
}

// CIGAR operations (SAM spec §1.4: M 0, I 1, D 2, N 3, S 4, H 5, P 6, = 7, X 8); the host twins of these and of ins_after: cigar_host.h
__device__ inline bool consumes_ref(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }
__device__ inline bool is_match(uint32_t op) { return op == 0 || op == 7 || op == 8; }
__device__ inline bool consumes_query(uint32_t op) { return op == 0 || op == 1 || op == 4 || op == 7 || op == 8; }

// where reference `tid` starts on the one coordinate axis: without a contig layout reference 0 at the uniform shift (batched uploads),
// with one its table entry (a handful of words, read through the scalar cache); < 0: the read does not pile up
__device__ inline int32_t shift_of(const PackSrc &s, int32_t tid)
{
    if (s.n_lay == 0) return tid == 0 ? s.pos_shift : -1;
    return tid >= 0 && tid < s.n_lay ? s.lay[tid] : -1;
}

// htslib resolve_cigar2's peek at the last reference base of op k: is an insertion reported there?
__device__ inline bool ins_after(const uint8_t *cg, uint32_t n, uint32_t k)
{
    if (k + 1 >= n) return false;
    const uint32_t c2 = ld_u32(cg + 4 * (size_t)(k + 1)), op2 = c2 & 0xFu;
    uint32_t tot = 0;
    if (op2 == 1) {
        tot = c2 >> 4;
        for (uint32_t j = k + 2; j < n; ++j) {
            const uint32_t c = ld_u32(cg + 4 * (size_t)j), o = c & 0xFu;
            if (o == 1) tot += c >> 4;
            else if (o != 6) break;
        }
    } else if (op2 == 6 && k + 2 < n) {
        for (uint32_t j = k + 2; j < n; ++j) {
            const uint32_t c = ld_u32(cg + 4 * (size_t)j), o = c & 0xFu;
            if (o == 1) tot += c >> 4;
            else if (consumes_ref(o)) break;
        }
    }
    return tot > 0;
}

// ---- THE wave join ------------------------------------------------------------------------------------------------------------------
// The lanes of a wavefront whose `todo` is set, grouped by equal key: per distinct key ONE call f(lead, lk, same) — lead the group's
// lowest lane, lk its key, same whether this lane is of the group — that every lane of the wavefront makes together, so f may ballot and
// shuffle; what it adds or stores, it does on lane `lead` alone.  One pass per distinct key: a sorted BAM puts a wavefront's 64 records
// on one or two.  THE RULE: every lane of the wavefront calls wave_join, with todo = false when it has nothing — the ballots and the
// shuffle see all 64 lanes; so the loop around a call has a bound that is uniform over the wavefront.
template <class K, class F> __device__ inline void wave_join(bool todo, K key, F f)
{
    for (;;) {
        const unsigned long long m = __ballot(todo);
        if (!m) break;
        const int lead = (int)__builtin_ctzll(m);
        const K lk = __shfl(key, lead, 64);
        const bool same = todo && key == lk;
        f(lead, lk, same);
        if (same) todo = false;
    }
}

// ---- what the kernels that walk the records where they lie share (tally.hip: tally_stream_kernel; amplicon_reads.hip; strand_counts.hip;
// link_counts.hip) ----
// the columns of the one axis lie in [0, 2^29): what a counting call can be asked for (stream_count.h) and where a walk ends (stream_walk.h)
constexpr int64_t WALK_MAX_COL = 1 << 29;

// the reference span of a read: the sum of its reference-consuming ops (unaligned dword loads, no base is read)
__device__ inline int64_t ref_span(const ReadView &v)
{
    int64_t span = 0;
    for (uint32_t k = 0; k < v.n_cigar; ++k) {
        const uint32_t c = ld_u32(v.cigar + 4 * (size_t)k);
        if (consumes_ref(c & 0xFu)) span += c >> 4;
    }
    return span;
}

// Record i of a stream source: true exactly when the device packer keeps it, with its first and last column [p, q] on the one axis.
// THE kept-record rule outside the packer: mapped, through the read filter the set was built under, consistent, on a reference that
// piles up, with a reference span and a query total below 2^29 (cigar_rule.h; the packer refuses the file over a record beyond that, so
// this copy only keeps a kernel that is asked all the same away from it).  The packer's own copy is pack_device.hip's classify_view (one walk that also decides `simple`, at
// pk_index's register ceiling): a rule changed here is changed there, and the other way round.
__device__ inline bool kept_span(const PackSrc &s, int64_t i, ReadView &v, int64_t &p, int64_t &q)
{
    v = view_rec(s.stream + s.rec_off[i]);
    if ((v.flag & 0x4u) || !passes(s.flt, v) || v.bad || v.pos < 0) return false;
    const int32_t shift = shift_of(s, v.tid);
    if (shift < 0) return false;
    int64_t span = 0;
    int32_t yr = TCMI_CIGAR_YR0;    // min(Yq - 2^29, 0)
    for (uint32_t k = 0; k < v.n_cigar; ++k) {
        tcmi_cigar_step(span, yr, ld_u32(v.cigar + 4 * (size_t)k));
    }
    if (span <= 0 || tcmi_cigar_malformed(span, yr)) return false;
    p = (int64_t)v.pos + shift;
    q = p + span - 1;
    return true;
}

// the lookup in a compiled primer segment list (primer_table.h; t: a[n] | b[n] | v[n]): the value of the segment that holds x, or `none`
// (host twin: primer_table.cpp's tcmi_pseg_find)
__device__ inline int32_t seg_find(const int32_t *t, int32_t n, int32_t x, int32_t none)
{
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (t[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo > 0 && x < t[n + lo - 1] ? t[2 * n + lo - 1] : none;
}

// leaves of the token rule: the count matrix's plane of a one-letter SEQ nibble (A 1, C 2, G 4, T 8), and the quality of query index
// qi — 0 at or beyond l_seq (QUAL lies behind SEQ; the first form is for a kernel that holds the pointer across a loop)
__device__ inline int base_plane(uint32_t nib)
{
    const int b = __ffs(nib) - 1;
    return b == 0 ? TCMI_A : b == 1 ? TCMI_C : b == 2 ? TCMI_G : TCMI_T;
}
__device__ inline uint32_t qual_at(const uint8_t *qual, int32_t l_seq, int32_t qi) { return qi < l_seq ? byte_at(qual + qi) : 0u; }
__device__ inline uint32_t qual_at(const ReadView &v, int32_t qi) { return qual_at(v.seq + ((size_t)v.l_seq + 1) / 2, v.l_seq, qi); }

} // namespace
