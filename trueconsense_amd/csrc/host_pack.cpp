// host_pack.cpp — HOST: the stages of host_pack.h.  No HIP header, no context.
#include "host_pack.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <functional>
#include <thread>

#include "cigar_host.h"

using namespace tcmi_cigar;

namespace {

typedef tcmi_host_sel Sel;
typedef tcmi_host_gsel GSel;
typedef tcmi_host_slice Slice;

// BAM byte (two 4-bit codes, first base in the high nibble) -> two one-hot class nibbles in
// linear order (first base in the low nibble); codes other than A/C/G/T become 0.
struct SwapLut {
    uint8_t t[256];
    SwapLut()
    {
        auto oh = [](unsigned c) -> unsigned { return (c == 1 || c == 2 || c == 4 || c == 8) ? c : 0; };
        for (unsigned b = 0; b < 256; ++b) t[b] = (uint8_t)(oh(b >> 4) | (oh(b & 15) << 4));
    }
};
const SwapLut kSwap;

inline unsigned one_hot_at(const uint8_t *src, int64_t q)      // base q of a BAM SEQ as a one-hot class nibble (no A/C/G/T: 0)
{
    const unsigned code = (q & 1) ? (src[q >> 1] & 15u) : (src[q >> 1] >> 4);
    return (code == 1 || code == 2 || code == 4 || code == 8) ? code : 0;
}

int refuse(tcmi_host_packed &P, int code, const char *text)
{
    std::snprintf(P.msg, sizeof P.msg, "%s", text);
    return code;
}

// ---- select ------------------------------------------------------------------------------------------------------------------
struct SelectJob {
    const tcmi_reads *const *batch; int32_t n_batch; int64_t stride;
    const tcmi_layout &lay; const tcmi_host_pack_opts &opt;
    int n_cls;
};

void fail(Slice &P, int code, const char *fmt, long long x, long long y, long long z)
{
    P.err = code;
    std::snprintf(P.msg, sizeof P.msg, fmt, x, y, z);
}

// slice t of BAM bi: its reads that pile up, classified, into the slice's own lists
void classify_slice(const SelectJob &J, Slice &P, int32_t bi, int t)
{
    const tcmi_reads *r = J.batch[bi];
    const tcmi_layout &lay = J.lay;
    const int64_t off0 = (int64_t)bi * J.stride;
    const int64_t i0 = r->n_reads * t / J.n_cls, i1 = r->n_reads * (t + 1) / J.n_cls;
    for (int64_t i = i0; i < i1; ++i) {
        int64_t span;
        // Reads on a second or later reference: the reference implementation piles them up keyed by position only, so they
        // collide with the first reference's columns and its BuildIndex fails (indexing.py:137-151).  They never
        // pile up here, and an upload that meets a mapped one fails with TCMI_E_UNSUPPORTED instead of tallying it onto
        // reference 0's coordinates.
        if (!lay.n() && r->tid && r->tid[i] > 0 && !(r->flag[i] & 0x4))
            return fail(P, TCMI_E_UNSUPPORTED, "read %lld is mapped to reference %lld: only single-reference alignments are supported "
                                               "(the reference implementation keys columns by position only and fails on these)%.0lld", i, r->tid[i], 0);
        const int32_t tid = r->tid ? r->tid[i] : 0;
        if (lay.n() && lay.shift_of(tid) < 0 && tid >= 0 && !(r->flag[i] & 0x4) && r->pos[i] >= 0) ++P.n_dropped;
        if (!tcmi_host_piles_up(r, i, &span, lay)) continue;
        const int64_t off = off0 + (lay.n() ? lay.shift_of(tid) : 0);
        if (lay.n() && off + r->pos[i] + span > lay.end_of(tid))
            return fail(P, TCMI_E_UNSUPPORTED, "read %lld on reference %lld ends past the end of its contig's slot (at %lld)", i, tid, r->pos[i] + span);
        if (lay.n() && r->pos[i] + span > P.ref_ext[(size_t)tid]) P.ref_ext[(size_t)tid] = r->pos[i] + span;
        const uint32_t *cg = r->cigar + r->cigar_off[i];
        const int64_t nc = (int64_t)(r->cigar_off[i + 1] - r->cigar_off[i]);
        if (nc > 65535) return fail(P, TCMI_E_UNSUPPORTED, "read %lld has %lld CIGAR ops (> 65535)%.0lld", i, nc, 0);
        // The CIGAR rule (cigar_rule.h), where the device packer's classify_view raises PKF_BADREAD: a read that would be kept with a
        // query total of 2^29 or more is no alignment — the walks that follow index SEQ and QUAL by that total.
        {
            const tcmi_cigar_sums sums = tcmi_cigar_walk([cg](uint32_t k) { return cg[k]; }, (uint32_t)nc);
            if (tcmi_cigar_malformed(sums))
                return fail(P, TCMI_E_FORMAT, "read %lld is malformed: its CIGAR consumes %lld query bases (2^29 or more; the reference span is %lld)",
                            i, sums.yq, sums.span);
        }
        const int64_t lq = r->l_qseq[i];
        if (lq < 0) return fail(P, TCMI_E_ARG, "read %lld has negative l_qseq%.0lld%.0lld", i, 0, 0);
        const int64_t nbytes = (int64_t)(r->seq_off[i + 1] - r->seq_off[i]);
        if (nbytes < (lq + 1) / 2) return fail(P, TCMI_E_ARG, "read %lld: seq bytes %lld < ceil(l_qseq/2)%.0lld", i, nbytes, 0);
        if (J.n_batch > 1 && r->pos[i] + span > J.stride)
            return fail(P, TCMI_E_ARG, "read %lld of a batched BAM ends at %lld, beyond the batch stride %lld", i, r->pos[i] + span, J.stride);
        if (span > INT32_MAX || off + r->pos[i] + span > INT32_MAX - 4096)
            return fail(P, TCMI_E_UNSUPPORTED, "read %lld ends beyond 2^31%.0lld%.0lld", i, 0, 0);
        P.alg += 12 + 4 * nc + (lq + 1) / 2;
        if (off + r->pos[i] + span > P.max_end) P.max_end = off + r->pos[i] + span;
        int64_t y0, len;
        const bool fast = J.opt.use_fast && off + r->pos[i] + span < TCMI_F_EVPOS;
        if (fast && aligned_shape(cg, nc, TCMI_F_MAXSPAN, &y0, &len)) P.fsel.push_back({r, i, off, y0, len, 0, false});
        else if (fast && J.opt.project_reads) {
            // any CIGAR, projected onto the reference; a long read in pieces (the count matrix is a sum over
            // positions, so cutting a read changes nothing)
            for (int64_t seg = 0; seg < span; seg += TCMI_F_SEG)
                P.fsel.push_back({r, i, off, 0, std::min<int64_t>(TCMI_F_SEG, span - seg), seg, true});
            if (span > TCMI_F_SEG) P.any_cut = true;
        }
        else { P.gsel.push_back({r, i, off}); P.g_cig += nc; P.g_seqw += (lq + 7) / 8; }
    }
}

void classify_thread(const SelectJob &J, std::vector<Slice> &slices, int t)
{
    for (int32_t bi = 0; bi < J.n_batch; ++bi) classify_slice(J, slices[(size_t)bi * (size_t)J.n_cls + (size_t)t], bi, t);
}

// ---- plan_chunks -------------------------------------------------------------------------------------------------------------
struct Window { int64_t read0, n, lo, hi, maxnw; };     // the chunk that is being filled: its reads, positions [lo, hi), longest read in grid words

void close_chunk(const Window &w, int stage_cap, std::vector<tcmi_fast_chunk> &chunks)
{
    tcmi_fast_chunk c;
    std::memset(&c, 0, sizeof c);
    c.read0 = w.read0;
    c.n_reads = (int32_t)w.n;
    c.P0 = (int32_t)w.lo;
    c.Wn = (int32_t)((w.hi - w.lo + 7) / 8);
    c.sub_reads = (int32_t)tcmi_stage_reads(c.Wn, w.maxnw, stage_cap);
    chunks.push_back(c);
}

// ---- pack_aligned ------------------------------------------------------------------------------------------------------------
const int64_t kPrefix = 2;          // zero words in front of a chunk's first read

// A projected read's piece into one-hot nibbles at dst.  Walk the CIGAR once: matched bases land on their reference offset, D / N
// leave zero nibbles (coverage only), and the tokens that are not plain bases become events: X for a deleted base
// whose token is exactly "*", I on the last reference base before an insertion (also "*+..": I but not X).
void project_piece(const Sel &s, int64_t rpos, uint8_t *dst, std::vector<uint32_t> &ev)
{
    const tcmi_reads *r = s.r;
    const uint8_t *src = r->seq + r->seq_off[s.i];
    const int64_t lq = r->l_qseq[s.i];
    const uint32_t *cg = r->cigar + r->cigar_off[s.i];
    const int64_t nc = (int64_t)(r->cigar_off[s.i + 1] - r->cigar_off[s.i]);
    // x = offset in the read's reference span, relative to this piece [0, s.len)
    int64_t x = -s.seg, y = 0;
    for (int64_t k = 0; k < nc && x < s.len; ++k) {
        const unsigned op = cg[k] & 0xF;
        const int64_t len = cg[k] >> 4;
        if (consumes_ref(op)) {
            const bool ins = len > 0 && ins_after(cg, nc, k);
            const int64_t t0 = std::max<int64_t>(0, -x), t1 = std::min(len, s.len - x);   // part inside the piece
            if (is_match(op)) {
                for (int64_t t = t0; t < t1; ++t) {
                    const int64_t q = y + t;
                    if (q >= lq) break;
                    dst[(x + t) >> 1] |= (uint8_t)(one_hot_at(src, q) << (((x + t) & 1) * 4));
                }
            } else if (op == 2) {
                for (int64_t t = t0; t < std::min(t1, ins ? len - 1 : len); ++t)
                    ev.push_back((uint32_t)(rpos + x + t) | TCMI_F_EV_X);
            }
            if (ins && x + len - 1 >= 0 && x + len - 1 < s.len) ev.push_back((uint32_t)(rpos + x + len - 1) | TCMI_F_EV_I);
            x += len;
        }
        if (consumes_query(op)) y += len;
    }
}

// An aligned read's bases [y0, y0 + len) into one-hot nibbles at dst, as far as SEQ has them.
void copy_aligned(const Sel &s, uint8_t *dst)
{
    const uint8_t *src = s.r->seq + s.r->seq_off[s.i];
    const int64_t have = std::max<int64_t>(0, std::min(s.len, (int64_t)s.r->l_qseq[s.i] - s.y0));   // bases present in SEQ
    if ((s.y0 & 1) == 0) {
        const uint8_t *b = src + (s.y0 >> 1);
        const int64_t full = have >> 1;
        for (int64_t k = 0; k < full; ++k) dst[k] = kSwap.t[b[k]];
        if (have & 1) dst[full] = (uint8_t)(kSwap.t[b[full]] & 0x0F);
    } else {
        for (int64_t k = 0; k < have; ++k) dst[k >> 1] |= (uint8_t)(one_hot_at(src, s.y0 + k) << ((k & 1) * 4));
    }
}

// bases that are no A/C/G/T: rare, found a word at a time
void other_events(const uint32_t *w, int64_t nw, int64_t len, int64_t rpos, std::vector<uint32_t> &ev)
{
    for (int64_t k = 0; k < nw; ++k) {
        const uint32_t v = w[k];
        uint32_t nz = (v | (v >> 1) | (v >> 2) | (v >> 3)) & 0x11111111u;   // 1 per non-zero nibble
        const int64_t in_read = std::min<int64_t>(8, len - 8 * k);
        const uint32_t want = in_read >= 8 ? 0x11111111u : (0x11111111u >> (4 * (8 - in_read)));
        uint32_t miss = want & ~nz;
        while (miss) {
            const int bit = __builtin_ctz(miss);
            ev.push_back((uint32_t)(rpos + 8 * k + bit / 4) | TCMI_F_EV_OTHER);
            miss &= miss - 1;
        }
    }
}

inline uint32_t squeeze(uint32_t x)                 // bits 0,4,..,28 -> bits 0..7
{
    x = (x | (x >> 3)) & 0x03030303u;
    x = (x | (x >> 6)) & 0x000F000Fu;
    return (x | (x >> 12)) & 0xFFu;
}

// one-hot nibbles -> codes A=0 C=1 G=2 T=3 (class-less = 0) as {lo plane, hi plane} per 32 bases
void to_planes(const uint32_t *w, int64_t nw, int64_t len, uint32_t *out)
{
    for (int64_t q = 0; q < (len + 31) / 32; ++q) {
        uint32_t lo = 0, hi = 0;
        for (int64_t k = 0; k < 4 && 4 * q + k < nw; ++k) {
            const uint32_t v = w[4 * q + k];
            lo |= squeeze(((v >> 1) | (v >> 3)) & 0x11111111u) << (8 * k);   // C or T
            hi |= squeeze(((v >> 2) | (v >> 3)) & 0x11111111u) << (8 * k);   // G or T
        }
        out[2 * q] = lo;
        out[2 * q + 1] = hi;
    }
}

// thread t of n_threads packs its share of the chunks: headers, bases and stage_end[] at their final places, events and coverage runs
// into its own lists (run0 relative to `runs`: made global once the threads' lists are joined)
void pack_chunk_range(tcmi_host_packed &P, int t, int n_threads, std::vector<uint32_t> &ev, std::vector<uint32_t> &runs, std::atomic<bool> &overflow)
{
    std::vector<tcmi_fast_chunk> &chunks = P.chunks;
    uint32_t *f_seq = P.f_seq;
    std::vector<uint32_t> scratch;                                        // a read's nibbles before they become planes
    const size_t c0 = chunks.size() * (size_t)t / (size_t)n_threads, c1 = chunks.size() * (size_t)(t + 1) / (size_t)n_threads;
    for (size_t ci = c0; ci < c1; ++ci) {
        tcmi_fast_chunk &c = chunks[ci];
        const size_t c_end = ci + 1 < chunks.size() ? (size_t)chunks[ci + 1].word0 : P.f_words;
        std::memset(&f_seq[(size_t)c.word0], 0, (c_end - (size_t)c.word0) * 4);      // pads and alignment gaps stay zero
        size_t cursor = (size_t)c.word0 + (size_t)kPrefix;
        size_t stage_begin = (size_t)c.word0;
        c.run0 = (int64_t)runs.size();
        uint32_t run_key = 0xFFFFFFFFu;
        for (int64_t j = c.read0; j < c.read0 + c.n_reads; ++j) {
            const Sel &s = P.fsel[(size_t)j];
            const int64_t rpos = s.r->pos[s.i] + s.off + s.seg;      // reference position of the entry's first base
            const int64_t nw = (s.len + 7) / 8;
            const size_t base = cursor;
            // ONE packed word per read — position relative to the window | len << 10 | pair offset from
            // the stage's first word << 20 (a stage starts on the zero pair in front of its first read)
            // (10 + 10 + 12 bits: the chunker keeps windows <= 768 positions, entries <= 600 positions and
            // stages <= 6144 words; checked, not assumed)
            if (rpos - c.P0 > 1023 || s.len > 1023 || (base - stage_begin) / 2 > 4095) overflow.store(true);
            P.f_lenoff[(size_t)j] = (uint32_t)(rpos - c.P0) | ((uint32_t)s.len << 10) | ((uint32_t)((base - stage_begin) / 2) << 20);
            // coverage: reads of equal (position, length) follow each other in a sorted BAM — one run word per
            // group instead of per-read bookkeeping in the kernel
            const uint32_t key = (uint32_t)(rpos - c.P0) | ((uint32_t)s.len << 10);
            if (key == run_key && (runs.back() >> 20) < 4095u) runs.back() += 1u << 20;
            else { runs.push_back(key | (1u << 20)); run_key = key; }
            cursor += (size_t)tcmi_read_words(s.len);
            scratch.assign((size_t)nw + 1, 0u);
            if (s.projected) project_piece(s, rpos, reinterpret_cast<uint8_t *>(scratch.data()), ev);
            else copy_aligned(s, reinterpret_cast<uint8_t *>(scratch.data()));
            other_events(scratch.data(), nw, s.len, rpos, ev);
            to_planes(scratch.data(), nw, s.len, &f_seq[base]);
            if ((j - c.read0 + 1) % c.sub_reads == 0 || j + 1 == c.read0 + c.n_reads) {
                c.stage_end[(j - c.read0) / c.sub_reads] = (int32_t)(cursor - (size_t)c.word0);
                stage_begin = cursor - 2;                        // the next stage starts on this read's zero pair
            }
        }
        c.n_runs = (int32_t)((int64_t)runs.size() - c.run0);
    }
}

} // namespace

size_t tcmi_host_packed::bytes() const
{
    size_t b = fsel.capacity() * sizeof(Sel) + gsel.capacity() * sizeof(GSel) + chunks.capacity() * sizeof(tcmi_fast_chunk) +
               (f_lenoff.capacity() + f_event.capacity() + f_covrun.capacity() + f_seq_cap) * 4 +
               (g_pos.capacity() + g_lseq.capacity() + g_meta.capacity() + g_cigar.capacity() + g_seq.capacity()) * 4 +
               (g_round_cig.capacity() + g_round_seq.capacity()) * 8;
    for (const Slice &s : slices) b += s.fsel.capacity() * sizeof(Sel) + s.gsel.capacity() * sizeof(GSel);
    return b;
}

int tcmi_host_check_reads(const tcmi_reads *r, const char **msg)
{
    *msg = nullptr;
    if (!r) *msg = "reads is NULL";
    else if (r->n_reads < 0) *msg = "n_reads < 0";
    else if (r->n_reads > 0 && (!r->pos || !r->flag || !r->l_qseq || !r->cigar_off || !r->seq_off)) *msg = "reads has NULL arrays";
    return *msg ? TCMI_E_ARG : TCMI_OK;
}

bool tcmi_host_piles_up(const tcmi_reads *r, int64_t i, int64_t *span, const tcmi_layout &lay)
{
    if (r->flag[i] & 0x4) return false;
    if (lay.shift_of(r->tid ? r->tid[i] : 0) < 0) return false;
    if (r->pos[i] < 0) return false;
    *span = ref_span(r->cigar + r->cigar_off[i], (int64_t)(r->cigar_off[i + 1] - r->cigar_off[i]));
    return *span > 0;
}

int tcmi_host_select(const tcmi_reads *const *batch, int32_t n_batch, int64_t stride, const tcmi_layout &lay, const tcmi_host_pack_opts &opt,
                     tcmi_host_packed *out)
{
    tcmi_host_packed &P = *out;
    P.fsel.clear();
    P.gsel.clear();
    P.n_reads_in = P.alg = P.max_end = P.n_dropped = P.g_cig = P.g_seqw = 0;
    P.ref_ext.assign((size_t)lay.n(), 0);
    P.msg[0] = 0;
    for (int32_t b = 0; b < n_batch; ++b) {
        const char *text;
        if (const int rc = tcmi_host_check_reads(batch[b], &text)) return refuse(P, rc, text);
        P.n_reads_in += batch[b]->n_reads;
    }
    // every BAM's reads in `host_threads` contiguous slices, each into its own lists, joined in order afterwards
    const int n_cls = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)opt.host_threads, 64, P.n_reads_in / 65536 + 1}));
    P.slices.resize((size_t)n_batch * (size_t)n_cls);
    for (Slice &S : P.slices) {
        S.fsel.clear(); S.gsel.clear();
        S.g_cig = S.g_seqw = S.alg = S.max_end = S.n_dropped = 0;
        S.any_cut = false; S.err = TCMI_OK;
        S.ref_ext.assign((size_t)lay.n(), 0);
    }
    const SelectJob J = {batch, n_batch, stride, lay, opt, n_cls};
    {
        std::vector<std::thread> th;
        for (int t = 1; t < n_cls; ++t) th.emplace_back(classify_thread, std::cref(J), std::ref(P.slices), t);
        classify_thread(J, P.slices, 0);
        for (auto &x : th) x.join();
    }
    size_t nfs = 0, ngs = 0;
    for (const Slice &S : P.slices) {
        if (S.err) return refuse(P, S.err, S.msg);
        nfs += S.fsel.size(); ngs += S.gsel.size();
    }
    P.fsel.reserve(nfs); P.gsel.reserve(ngs);
    bool any_cut = false;
    for (const Slice &S : P.slices) {
        P.fsel.insert(P.fsel.end(), S.fsel.begin(), S.fsel.end());
        P.gsel.insert(P.gsel.end(), S.gsel.begin(), S.gsel.end());
        P.g_cig += S.g_cig; P.g_seqw += S.g_seqw; P.alg += S.alg; P.max_end = std::max(P.max_end, S.max_end); any_cut |= S.any_cut;
        P.n_dropped += S.n_dropped;
        for (size_t t = 0; t < S.ref_ext.size(); ++t) P.ref_ext[t] = std::max(P.ref_ext[t], S.ref_ext[t]);
    }
    if (any_cut)                                // pieces of long reads start further right than the reads that follow them
        std::stable_sort(P.fsel.begin(), P.fsel.end(), [](const Sel &a, const Sel &b) {
            return a.r->pos[a.i] + a.off + a.seg < b.r->pos[b.i] + b.off + b.seg;
        });
    return TCMI_OK;
}

// Chunks: consecutive entries while their window stays within TCMI_F_MAXW grid words and their number within tcmi_chunk_reads; then
// the base stream's sizes, chunk by chunk: [pad] read [pad] read [pad] ... each chunk 16-byte aligned.
void tcmi_host_plan_chunks(const tcmi_host_pack_opts &opt, tcmi_host_packed *out)
{
    tcmi_host_packed &P = *out;
    const int64_t nf = (int64_t)P.fsel.size();
    // chunk_stages = 0: long chunks (up to TCMI_F_MAXSTAGE stages), but capped so that the launch has k * slots chunks
    const int n_stages = opt.chunk_stages > 0 ? std::min(opt.chunk_stages, TCMI_F_MAXSTAGE) : TCMI_F_MAXSTAGE;
    const int64_t balanced_cap = opt.chunk_stages == 0 && opt.balance ? tcmi_balanced_chunk(nf, opt.slots) : INT64_MAX;
    P.chunks.clear();
    Window w = {0, 0, 0, 0, 0};
    for (int64_t j = 0; j < nf; ++j) {
        const Sel &s = P.fsel[(size_t)j];
        const int64_t p = s.r->pos[s.i] + s.off + s.seg, e = p + s.len;
        const int64_t lo = p & ~(int64_t)7, nw = (s.len + 7) / 8;
        if (w.n > 0) {
            const int64_t nlo = std::min(w.lo, lo), nhi = std::max(w.hi, e), nmax = std::max(w.maxnw, nw);
            const int64_t words = (nhi - nlo + 7) / 8;
            if (words > TCMI_F_MAXW || w.n >= tcmi_chunk_reads(tcmi_stage_reads(words, nmax, opt.stage_cap), words, n_stages, balanced_cap)) {
                close_chunk(w, opt.stage_cap, P.chunks);
                w.n = 0;
            } else { w.lo = nlo; w.hi = nhi; w.maxnw = nmax; }
        }
        if (w.n == 0) { w.read0 = j; w.lo = lo; w.hi = e; w.maxnw = nw; }
        ++w.n;
    }
    if (w.n > 0) close_chunk(w, opt.stage_cap, P.chunks);
    size_t total = 0;
    for (tcmi_fast_chunk &c : P.chunks) {
        total = (total + 3) & ~(size_t)3;
        c.word0 = (int64_t)total;
        total += (size_t)kPrefix;
        for (int64_t j = c.read0; j < c.read0 + c.n_reads; ++j) total += (size_t)tcmi_read_words(P.fsel[(size_t)j].len);
    }
    total = (total + 3) & ~(size_t)3;
    if (P.f_seq_cap < total + 4) {
        delete[] P.f_seq;
        P.f_seq = nullptr;
        P.f_seq_cap = 0;
        P.f_seq = new uint32_t[total + 4 + total / 16];
        P.f_seq_cap = total + 4 + total / 16;
    }
    P.f_words = total;
}

// The planned chunks packed by `host_threads` threads, their events and coverage runs joined in chunk order.
int tcmi_host_pack_aligned(const tcmi_host_pack_opts &opt, tcmi_host_packed *out)
{
    tcmi_host_packed &P = *out;
    P.f_lenoff.resize(P.fsel.size());
    P.f_event.clear();
    P.f_covrun.clear();
    const int n_threads = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)opt.host_threads, (int64_t)P.chunks.size(), 64}));
    std::vector<std::vector<uint32_t>> ev_parts((size_t)n_threads), run_parts((size_t)n_threads);
    std::atomic<bool> overflow{false};
    if (n_threads == 1) pack_chunk_range(P, 0, 1, ev_parts[0], run_parts[0], overflow);
    else {
        std::vector<std::thread> th;
        for (int t = 0; t < n_threads; ++t)
            th.emplace_back(pack_chunk_range, std::ref(P), t, n_threads, std::ref(ev_parts[(size_t)t]), std::ref(run_parts[(size_t)t]), std::ref(overflow));
        for (auto &x : th) x.join();
    }
    if (overflow.load()) return refuse(P, TCMI_E_UNSUPPORTED, "internal: a packed read header field overflowed (window / length / stage offset)");
    for (auto &part : ev_parts) P.f_event.insert(P.f_event.end(), part.begin(), part.end());
    for (int t = 0; t < n_threads; ++t) {                    // thread t packed the chunks [c0, c1): shift their run offsets
        const size_t c0 = P.chunks.size() * (size_t)t / (size_t)n_threads, c1 = P.chunks.size() * (size_t)(t + 1) / (size_t)n_threads;
        for (size_t ci = c0; ci < c1; ++ci) P.chunks[ci].run0 += (int64_t)P.f_covrun.size();
        P.f_covrun.insert(P.f_covrun.end(), run_parts[(size_t)t].begin(), run_parts[(size_t)t].end());
    }
    return TCMI_OK;
}

// The general set: rounds of TCMI_ROUND reads with per-round offset tables, raw codes.
void tcmi_host_pack_general(tcmi_host_packed *out)
{
    tcmi_host_packed &P = *out;
    const int64_t ng = (int64_t)P.gsel.size();
    P.n_rounds = (ng + TCMI_ROUND - 1) / TCMI_ROUND;
    P.g_pos.resize((size_t)ng); P.g_lseq.resize((size_t)ng); P.g_meta.resize((size_t)ng);
    P.g_cigar.resize((size_t)P.g_cig + 1); P.g_seq.resize((size_t)P.g_seqw + 1);
    P.g_round_cig.resize((size_t)P.n_rounds + 1); P.g_round_seq.resize((size_t)P.n_rounds + 1);
    int64_t co = 0, so = 0;
    for (int64_t j = 0; j < ng; ++j) {
        const tcmi_reads *r = P.gsel[(size_t)j].r;
        const int64_t i = P.gsel[(size_t)j].i;
        if (j % TCMI_ROUND == 0) { P.g_round_cig[(size_t)(j / TCMI_ROUND)] = co; P.g_round_seq[(size_t)(j / TCMI_ROUND)] = so; }
        const int64_t nc = (int64_t)(r->cigar_off[i + 1] - r->cigar_off[i]);
        const int64_t lq = r->l_qseq[i];
        P.g_pos[(size_t)j] = (int32_t)(r->pos[i] + P.gsel[(size_t)j].off);
        P.g_lseq[(size_t)j] = (int32_t)lq;
        P.g_meta[(size_t)j] = ((uint32_t)r->flag[i] << 16) | (uint32_t)nc;
        std::memcpy(&P.g_cigar[(size_t)co], r->cigar + r->cigar_off[i], (size_t)nc * 4);
        co += nc;
        const uint8_t *s = r->seq + r->seq_off[i];
        const int64_t nw = (lq + 7) / 8, nb = (lq + 1) / 2;
        uint8_t *dst = reinterpret_cast<uint8_t *>(&P.g_seq[(size_t)so]);
        for (int64_t b = 0; b < nb; ++b) dst[b] = (uint8_t)((s[b] << 4) | (s[b] >> 4));   // linear nibble order
        if (lq & 1) dst[nb - 1] &= 0x0F;                                                   // pad nibble = 0
        for (int64_t b = nb; b < nw * 4; ++b) dst[b] = 0;
        so += nw;
    }
    P.g_round_cig[(size_t)P.n_rounds] = co;
    P.g_round_seq[(size_t)P.n_rounds] = so;
}
