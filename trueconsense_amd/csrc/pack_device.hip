// pack_device.hip — DEVICE: BAM-native reads -> the bit-plane layout tally_planes.hip consumes.
//
// What the reference does per pileup token in Python (indexing.py:100-139: pileup membership, the token of every covered position,
// parse_query_sequences' classification) is decided here per READ by HIP kernels, straight from what a BAM holds (SAM spec §4.2: pos,
// flag, l_seq, CIGAR words, 4-bit SEQ; pack_device.h: one read as the kernels see it).  Two chains of kernels fill the same read set.
//
// The several-kernel packer (tcmi_pack_on_device): the flat arrays of struct tcmi_reads copied to the device as they are, or an inflated
// BAM stream with its record index (bam_device.hip: files the one-sync packer declines); the host reads the totals back twice.
//   pk_classify   one lane per read: does it pile up, reference span, CIGAR shape ([H][S]M[S][H] reads are taken as they
//                 are, anything else is projected onto the reference), words it will occupy; per-workgroup sums for the scan
//   pk_scan       exclusive scan of the per-workgroup sums (one workgroup)
//   pk_scatter    compacted index of every kept read + its word offset (block scan + the scanned sums)
//   pk_pack       one workgroup per run of consecutive kept reads: cuts it into chunks (window <= 768 positions, <= 255 reads per lane,
//                 <= 8 stages that fill the tally kernel's LDS stage buffer), writes the chunk records, ONE packed header word per read
//                 and the coverage runs (reads of equal position and length)
//   pk_planes     one lane per 32 bases: the bases as {lo, hi} bit planes — 4-bit codes classified eight at a time with SWAR bit tricks
//                 (one-hot test, C|T and G|T planes, bit squeeze); a projected read has its CIGAR walked by its own lane (M/=/X copy
//                 bit fields, D -> X events, insertions -> I events on the base before, every covered position without an A/C/G/T
//                 base -> OTHER event)
// The one-sync packer (tcmi_pack_fused_enqueue, _report, _finish): an inflated BAM stream as bgzf_copy left it, one workgroup per BGZF
// block, queued from CAPACITIES so that the host waits once per file (the comment above pk_index says why it has this shape).
//   pk_prefix     (files of very many blocks) prefix sums of the blocks' counts
//   pk_index      the block's records: their place in the record index, classification as in pk_classify, the record chain across it
//   pk_place      the chain check, the kept reads' entries and bit planes (pk_scatter's and pk_planes' work) at their final places
//   pk_pack       as above, from the counts pk_place left on the device
//   pk_report     totals and per-block verdicts into pinned host memory, behind whatever the caller queued behind the packer
//
// Where it all lies — ONE translation unit (classify_view and pack_read keep all their callers: split three ways, pk_classify, pk_index and
// pk_place_bq came out with other machine code), its device code in headers that this file includes once each:
//   pack_caps.h       (plain C++, no HIP: tcmi_internal.h includes it) the PKF_* flags, the one-sync packer's capacities and the "did the
//                     totals fit" test, the chunk rule both packers size by, the pinned report's offsets, each packer's arena scratch as a list
//   this file         what every kernel here shares (PackTotals, words_of, block_scan2, filter_view, classify_view), pk_pack, pk_mask_long,
//                     pk_report and the host code: the helpers both packers call, then the packers
//   pack_bits.h       PackOut, codes -> bit planes, the floor, the primer mask, pack_read
//   pack_several.h    pk_classify, pk_scan, pk_scatter, pk_planes(_bq)
//   pack_one_sync.h   pk_prefix, pk_index, pk_place(_bq)
//
// HBM-streaming byte / bit work: no MFMA.  Input 91 B + 20 B of offsets per 150-bp read, output 52 B.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tally_common.h"
#include "bgzf_device.h"
#include "pack_device.h"

namespace {

constexpr int PB = 256;                          // lanes per workgroup of every kernel here
constexpr uint32_t NIB = 0x11111111u;

// does the record carry a CG:B aux field (the real CIGAR of a read with more than 65 535 operations, SAM spec §4.2.2)?
__device__ inline bool has_cg_tag(const uint8_t *aux, const uint8_t *end)
{
    for (int guard = 0; guard < 4096 && aux + 3 <= end; ++guard) {
        const uint32_t t0 = byte_at(aux), t1 = byte_at(aux + 1), ty = byte_at(aux + 2);
        if (t0 == 'C' && t1 == 'G' && ty == 'B') return true;
        aux += 3;
        if (ty == 'A' || ty == 'c' || ty == 'C') aux += 1;
        else if (ty == 's' || ty == 'S') aux += 2;
        else if (ty == 'i' || ty == 'I' || ty == 'f') aux += 4;
        else if (ty == 'Z' || ty == 'H') { while (aux < end && byte_at(aux)) ++aux; ++aux; }
        else if (ty == 'B' && aux + 5 <= end) {
            const uint32_t st = byte_at(aux), cnt = ld_u32(aux + 1);
            const uint32_t sz = (st == 'c' || st == 'C') ? 1u : (st == 's' || st == 'S') ? 2u : 4u;
            if (cnt > (1u << 28)) return false;
            aux += 5 + (size_t)cnt * sz;
        } else return false;
    }
    return false;
}

// per-read word of pk_classify: len (10 bits, <= TCMI_D_MAXLEN) | projected << 10 | kept << 11 | y0 << 12
constexpr uint32_t INFO_PROJ = 1u << 10, INFO_KEPT = 1u << 11;

struct PackTotals {                 // device scalars, copied back to the host
    unsigned long long alg_bytes;
    unsigned long long n_kept, n_words;
    int32_t max_end;
    uint32_t flags;
    uint32_t n_chunks, n_events, n_runs;
    uint32_t word_cursor;
    uint32_t max_len;               // longest reference span of a kept read
    uint32_t n_gen;                 // reads left to the stream-walking tally kernel (longer than TCMI_D_MAXLEN positions)
    unsigned long long n_rec;       // pk_place: alignment records of the decoded range
    // pk_place, a block range: where its first record starts / where the first record behind it starts, as offsets into the range's
    // stream + 1 (0: no record starts in the range / the chain was never fixed) — tcmi_readset_range_anchors
    unsigned long long range_first, range_next;
    unsigned long long slot_ovf;    // a contig layout: (read index + 1) << 24 | reference of the last kept read that ends past its slot (0: none)
    unsigned long long n_dropped;   // a contig layout: mapped reads on references without a slot
    uint32_t n_filtered;            // a read filter: records that failed it (records are fewer than 2^31: PKF_REC_OVF)
    uint32_t n_masked;              // a primer table: kept reads with a non-empty head or tail mask (in what was the struct's tail padding)
};
static_assert(sizeof(PackTotals) == PK_TOTALS_BYTES, "n_masked sits in the tail padding: pk_report copies the struct as before");
static_assert(PB == PK_BLOCK, "pack_caps.h sizes the per-workgroup scratch of pk_classify");

// words a read takes in the plane stream: its pairs, the zero pair behind them, and — for an even number of pairs — one more zero pair,
// so that every read ends on a 16-byte boundary: the reads then lie in ONE contiguous run (a read's place is 2 + the scanned sum of
// the words in front of it, known before any chunk is cut), and the zero pair that closes a read is the one a chunk that starts with
// the next read needs in front of it — 16-byte aligned, as the tally kernel's loads want a chunk's first word.
__device__ inline uint32_t words_of(uint32_t len) { return (2u * ((len + 31u) >> 5) + 2u + 3u) & ~3u; }

// inclusive scan of a pair over the workgroup (PB lanes)
__device__ inline uint2 block_scan2(uint2 v, uint2 *wave_tot /* LDS [PB / 64] */)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t ox = (uint32_t)__shfl_up((int)v.x, d, 64), oy = (uint32_t)__shfl_up((int)v.y, d, 64);
        if (lane >= d) { v.x += ox; v.y += oy; }
    }
    __syncthreads();
    if (lane == 63) wave_tot[wave] = v;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < PB / 64; ++w)
        if (w < wave) { v.x += wave_tot[w].x; v.y += wave_tot[w].y; }
    return v;
}

// ---- 1: classify ----------------------------------------------------------------------------------------------
// what one read is to the packer: its per-read word (0: not kept), the words it takes in the plane stream, its SURVEY §8-d bytes,
// its end; `longread`: left to tally_stream_kernel (a device-decoded stream only; from flat arrays PKF_LONG is raised instead)
struct Classified { uint32_t word, nwords, len; unsigned long long alg; int32_t end; bool longread, slot_ovf; };

// The read filter, where a record enters the packer: a record that fails is marked unmapped — from here on it is ignored wherever a
// record with FLAG 0x4 is — and counted: one ballot over the lanes that are here and one atomic per wavefront that holds any (the lanes
// of a wavefront's tail are not here: the lowest failing lane adds).  Without a filter (both words 0) every record passes: no atomic.
// pk_classify asks filter_on first (uniform) and skips the compares too; pk_index, which sits at the scalar-register ceiling, does
// not — the branch around these few instructions cost it two more vector registers than the instructions themselves.
__device__ inline void filter_view(ReadView &v, const tcmi_filter_words &flt, PackTotals *tot)
{
    const bool failed = !passes(flt, v);
    const unsigned long long m = __ballot(failed);
    if (failed) {
        v.flag |= 0x4u;
        if ((int)(threadIdx.x & 63) == (int)__builtin_ctzll(m)) atomicAdd(&tot->n_filtered, (uint32_t)__popcll(m));
    }
}

__device__ inline int32_t slot_end_of(const PackSrc &s, int32_t tid) { return s.n_lay == 0 ? 0x7FFFFFFF : s.lay[s.n_lay + tid]; }

// the kept reads' max end per reference (a contig layout): called by every lane of the wavefront; one atomic per reference the
// wavefront holds reads of (one or two in a sorted file)
__device__ inline void ref_extent_max(int32_t *ext, int32_t t, int32_t e)
{
    wave_join(t >= 0 && e > 0, t, [&](int lead, int32_t lt, bool same) {
        int32_t v = same ? e : 0;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
        if ((int)(threadIdx.x & 63) == lead) atomicMax(ext + lt, v);
    });
}

// `shift`: where the read's reference starts on the axis (< 0: not piled up), `slot_end`: where its slot ends, `layout`: a contig
// layout is set (reads on other references are not an error then).  The read filter: the callers hand a failing record in with FLAG
// 0x4 set (filter_view) — it is ignored in the three places below, and in pk_classify's `dropped`, exactly as an unmapped record is
// The kernels that count in the stream afterwards ask pack_device.h's kept_span which records are kept here: the two hold the same rule,
// the CIGAR rule included (cigar_rule.h: a record that would be kept with a query total Yq >= 2^29 is malformed) — it raises PKF_BADREAD
// and is NOT kept, neither packed nor a long read: on the one-sync path pk_place, pk_pack and the tally are queued behind pk_index
// before the host reads the flags, and they must find nothing of such a record to walk (their query index has 32 bits).
__device__ inline Classified classify_view(const ReadView &v, int32_t mode, int32_t shift, int32_t slot_end, bool layout, const uint8_t *rec,
                                           bool stream_long_ok, PackTotals *tot)
{
    Classified c = {0u, 0u, 0u, 0ull, 0, false, false};
    const int32_t pos_shift = shift;
    bool kept = !(v.flag & 0x4u) && shift >= 0 && v.pos >= 0 && !v.bad;
    if (v.broken || (v.bad && !(v.flag & 0x4u) && shift >= 0 && v.pos >= 0)) atomicOr(&tot->flags, (uint32_t)PKF_BADREAD);
    if (!layout && !(v.flag & 0x4u) && v.tid > 0) atomicOr(&tot->flags, (uint32_t)PKF_MULTIREF);   // (the host packer words the error)
    if (!kept) return c;
    // one walk over the CIGAR: reference span and query total (cigar_rule.h), and is it [H]*[S]* (M|=|X)+ [S]*[H]* ?
    int64_t span = 0, m = 0, y0 = 0;
    int32_t yr = TCMI_CIGAR_YR0;    // min(Yq - 2^29, 0)
    int ph = 0;                     // 0 start / leading H, 1 leading S, 2 match run, 3 trailing S, 4 trailing H
    bool simple = true;
    for (uint32_t k = 0; k < v.n_cigar; ++k) {
        const uint32_t cw = ld_u32(v.cigar + 4 * (size_t)k), op = cw & 0xFu, len = cw >> 4;
        tcmi_cigar_step(span, yr, cw);
        if (op == 5) { if (ph >= 2) ph = 4; else if (ph == 1) simple = false; }
        else if (op == 4) { if (ph <= 1) { ph = 1; y0 += len; } else if (ph <= 3) ph = 3; else simple = false; }
        else if (is_match(op)) { if (ph <= 2) { ph = 2; m += len; } else simple = false; }
        else simple = false;
    }
    simple = simple && ph >= 2 && m > 0 && y0 < (1 << 20);
    if (mode == 1 && v.n_cigar == 2 && v.l_seq > 0) {   // <l_seq>S<n>N + a CG:B tag: the real CIGAR lives in the tag (SAM spec §4.2.2)
        const uint32_t c0 = ld_u32(v.cigar), c1 = ld_u32(v.cigar + 4);
        if ((c0 & 0xFu) == 4 && (c0 >> 4) == (uint32_t)v.l_seq && (c1 & 0xFu) == 3) {
            if (has_cg_tag(v.seq + ((size_t)v.l_seq + 1) / 2 + (size_t)v.l_seq, rec + 4 + ld_u32(rec)))
                atomicOr(&tot->flags, (uint32_t)PKF_BADREAD);   // (the host reader words the refusal)
        }
    }
    if (span <= 0) return c;
    if (tcmi_cigar_malformed(span, yr)) { atomicOr(&tot->flags, (uint32_t)PKF_BADREAD); return c; }
    const int64_t end = (int64_t)v.pos + pos_shift + span;
    const int64_t len = simple ? m : span;
    if (end >= (int64_t)TCMI_F_EVPOS) { atomicOr(&tot->flags, (uint32_t)PKF_FARPOS); return c; }
    if (end > (int64_t)slot_end) { atomicOr(&tot->flags, (uint32_t)PKF_SLOT_OVF); c.slot_ovf = true; return c; }      // (never tallied into the next slot)
    c.alg = (unsigned long long)(12 + 4 * (int64_t)v.n_cigar + ((int64_t)v.l_seq + 1) / 2);
    c.end = (int32_t)end;
    if (len > TCMI_D_MAXLEN) {
        // A read that spans more positions than a chunk's window (long-read platforms).  From the flat arrays: the host
        // packer cuts it into pieces.  In a device-decoded stream: it stays out of the packed set and is walked where it
        // lies, CIGAR op by CIGAR op, by tally_stream_kernel (one wavefront per such read).
        if (mode == 1 && stream_long_ok) c.longread = true;
        else { atomicOr(&tot->flags, (uint32_t)PKF_LONG); c.alg = 0; c.end = 0; }
        return c;
    }
    c.word = (uint32_t)len | (simple ? 0u : INFO_PROJ) | INFO_KEPT | (simple ? (uint32_t)y0 << 12 : 0u);
    c.nwords = words_of((uint32_t)len);
    c.len = (uint32_t)len;
    return c;
}

#include "pack_bits.h"
#include "pack_several.h"

// ---- pack: chunks, header words, coverage runs (both packers) ----------------------------------------------------------------------
// dev_slots > 0 (the one-sync path: nobody has read the totals back): n_kept and n_words are taken from `tot`, and the reads per
// workgroup are worked out here as tcmi_pack_on_device does on the host (dev_slots = the tally kernel's resident workgroups, or
// 1 << 30: no balancing); the grid was sized from the capacity, workgroups beyond the reads leave at once.
__global__ __launch_bounds__(PB) void pk_pack(PackOut o, const int32_t *c_pos, const uint32_t *c_info, const uint32_t *c_woff,
                                              uint32_t n_kept, uint32_t n_words, int reads_per_wg, int n_stages, int stage_cap, PackTotals *tot,
                                              int64_t dev_slots)
{
    if (dev_slots > 0) {
        n_kept = (uint32_t)min(tot->n_kept, (unsigned long long)0xFFFFFFF0u);
        // A file beyond the record or word capacity: pk_place left the entries of the blocks without room unwritten, and the kept
        // reads may outnumber c_pos / c_info / c_woff, lenoff and covrun.  No chunk is cut from such entries — the tally kernel that
        // tcmi_bamfile_step has queued behind this one takes a chunk's word0, P0 and run0 on trust — and nothing is stored past an
        // array's end; the host declines the file after its wait.  (The two bits are pk_index's and pk_place's, launches ago.)
        if (tot->flags & (PKF_REC_OVF | (uint32_t)PKF_WORD_OVF)) n_kept = 0u;
        n_words = (uint32_t)min(tot->n_words, (unsigned long long)o.word_cap - (unsigned long long)PK_WORD_SLACK);
        int64_t C = PK_LONG_CHUNK;                              // (the twin of pack_caps.h's pk_chunk_rule, readset_layout.h's tcmi_balanced_chunk: one shared function changes this kernel's code)
        if (dev_slots < (1ll << 30)) {
            const int64_t nf = n_kept;
            const int64_t k = max((int64_t)1, (nf + dev_slots * TCMI_F_LONGEST - 1) / (dev_slots * TCMI_F_LONGEST));
            C = max((int64_t)64, (nf + k * dev_slots - 1) / (k * dev_slots));
        }
        reads_per_wg = (int)min(C, (int64_t)PK_CMAX);
    }
    __shared__ int32_t s_pos[PK_CMAX];
    __shared__ uint32_t s_woff[PK_CMAX + 1];
    __shared__ uint16_t s_len[PK_CMAX];
    __shared__ uint16_t s_run[PK_CMAX + 1];     // chunk-relative index of every run's first read
    __shared__ int s_red[3][PB / 64];
    __shared__ int s_scan[PB / 64];
    __shared__ uint32_t s_slot[1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (blockIdx.x == 0 && tid < 64) {                          // what the last stage's last 16-byte load takes along, and the blob's slack
        if (tid < 16) o.seq[2u + n_words + tid] = 0u;
        o.slack[tid] = 0u;
    }
    const uint32_t r0 = (uint32_t)blockIdx.x * (uint32_t)reads_per_wg;
    if ((unsigned long long)blockIdx.x * (unsigned long long)reads_per_wg >= n_kept) return;     // (a grid sized from the capacity)
    const int n = (int)min((uint32_t)reads_per_wg, n_kept - r0);
    for (int t = tid; t < n; t += PB) {
        s_pos[t] = c_pos[r0 + t];
        s_len[t] = (uint16_t)(c_info[r0 + t] & 1023u);
        s_woff[t] = c_woff[r0 + t];
    }
    if (tid == 0) s_woff[n] = r0 + n < n_kept ? c_woff[r0 + n] : n_words;
    __syncthreads();

    int cur = 0;
    while (cur < n) {                                            // uniform: one chunk per turn
        const int P0 = s_pos[cur] & ~7;
        // the chunk's reads: the longest prefix of [cur, n) inside a window of MAXPOS positions that starts at P0
        int viol = n;
        for (int t = cur + 1 + tid; t < n; t += PB) {
            const int rel = s_pos[t] - P0;
            if (rel < 0 || rel + (int)s_len[t] > MAXPOS) { viol = t; break; }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) viol = min(viol, __shfl_xor(viol, d, 64));
        if (lane == 0) s_red[0][wave] = viol;
        __syncthreads();
        int e1 = s_red[0][0];
#pragma unroll
        for (int w = 1; w < PB / 64; ++w) e1 = min(e1, s_red[0][w]);
        int mend = 0, mlen = 0;
        for (int t = cur + tid; t < e1; t += PB) {
            mend = max(mend, s_pos[t] - P0 + (int)s_len[t]);
            mlen = max(mlen, (int)s_len[t]);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { mend = max(mend, __shfl_xor(mend, d, 64)); mlen = max(mlen, __shfl_xor(mlen, d, 64)); }
        if (lane == 0) { s_red[1][wave] = mend; s_red[2][wave] = mlen; }
        __syncthreads();
        mend = s_red[1][0]; mlen = s_red[2][0];
#pragma unroll
        for (int w = 1; w < PB / 64; ++w) { mend = max(mend, s_red[1][w]); mlen = max(mlen, s_red[2][w]); }
        // stage and chunk sizes exactly as the tally kernel will derive them from (Wn, sub_reads): the twins of readset_layout.h's
        // tcmi_stage_reads and tcmi_chunk_reads
        const int Wn = (mend + 7) >> 3;
        const int S = FB / max(2, (Wn * 8 + 31) >> 5);
        int cap = min((int)TCMI_P_SUB, (TCMI_F_SEQCAP - 16 - 2) / (int)words_of((uint32_t)mlen));
        if (stage_cap > 0) cap = min(cap, max(stage_cap, S * 4));
        int sub = S * 4 * max(1, cap / (S * 4));
        if (sub > cap) sub = max(S, cap / S * S);
        const int whole = max(sub, min(((1 << TCMI_P_NPL) - 1) * S, n_stages * sub) / sub * sub);
        const int nc = min(e1 - cur, whole);
        if (tid == 0) s_slot[0] = atomicAdd(&tot->n_chunks, 1u);
        // ---- coverage runs: reads of equal (position, length) follow each other in a sorted BAM ---------------------
        int n_runs = 0;
        for (int t0 = 0; t0 < nc; t0 += PB) {
            const int t = t0 + tid;
            bool start = false;
            if (t < nc) {
                const int j = cur + t;
                start = t == 0 || (t & 2047) == 0 || s_pos[j] != s_pos[j - 1] || s_len[j] != s_len[j - 1];
            }
            const int incl = block_scan_incl(start ? 1 : 0, s_scan);    // (two barriers inside: s_slot is visible after them)
            if (start) s_run[n_runs + incl - 1] = (uint16_t)t;
            __syncthreads();
            n_runs += s_scan[0] + s_scan[1] + s_scan[2] + s_scan[3];
            __syncthreads();
        }
        static_assert(PB / 64 == 4, "run count sums four wave totals");
        if (tid == 0) s_run[n_runs] = (uint16_t)nc;
        __syncthreads();
        // the chunk's words: from the zero pair that closes the read in front of its first one (the stream's own first pair for read 0)
        const uint32_t ci = s_slot[0], w0 = s_woff[cur];
        const bool fits = ci < o.chunk_cap;
        if (!fits && tid == 0) atomicOr(&tot->flags, (uint32_t)PKF_CHUNK_OVF);
        if (fits) {
            const uint32_t g0 = r0 + (uint32_t)cur;             // compacted index of the chunk's first read
            for (int k = tid; k < n_runs; k += PB) {
                const int t = s_run[k], cnt = (int)s_run[k + 1] - t, j = cur + t;
                o.covrun[g0 + k] = (uint32_t)(s_pos[j] - P0) | ((uint32_t)s_len[j] << 10) | ((uint32_t)cnt << 20);
            }
            if (tid == 0) {
                tcmi_fast_chunk c;
                c.read0 = g0; c.word0 = w0; c.n_reads = nc; c.P0 = P0; c.Wn = Wn; c.sub_reads = sub;
                for (int st = 0; st < TCMI_F_MAXSTAGE; ++st) {
                    const int last = min(nc, (st + 1) * sub);
                    c.stage_end[st] = st * sub < nc ? (int32_t)(2u + s_woff[cur + last] - s_woff[cur]) : 0;
                }
                c.run0 = g0; c.n_runs = n_runs; c.reserved_ = 0;
                o.chunks[ci] = c;
                atomicAdd(&tot->n_runs, (uint32_t)n_runs);
                if (w0 == 0u) { o.seq[0] = 0u; o.seq[1] = 0u; }  // the zero pair in front of the very first read (the others: pk_planes)
            }
        }
        // ---- per read: the header word, and where its planes go (pk_planes writes them, one lane per 32 bases) ----------------
        {
            const uint32_t g0 = r0 + (uint32_t)cur;
            for (int t = tid; t < nc; t += PB) {
                const int j = cur + t, st = t / sub;
                const uint32_t base = 2u + s_woff[j] - s_woff[cur];                          // words from word0
                const uint32_t sb = st == 0 ? 0u : s_woff[cur + st * sub] - s_woff[cur];     // the stage starts on the zero pair in front of its first read
                const uint32_t rel = (uint32_t)(s_pos[j] - P0), len = s_len[j], poff = (base - sb) >> 1;
                if (fits) {
                    if (rel > 1023u || len > 1023u || poff > 4095u) atomicOr(&tot->flags, (uint32_t)PKF_HEADER_OVF);
                    o.lenoff[g0 + t] = rel | (len << 10) | (poff << 20);
                }
            }
        }
        cur += nc;
        __syncthreads();
    }
}

#include "pack_one_sync.h"

// The long reads of a stream (left to tally_stream_kernel, which masks them tally by tally) with a non-empty head or tail mask, counted
// once for tcmi_readset_primers: a few workgroups stride over the tot->n_gen records the classifying kernel listed; one lane per read
// adds up its CIGAR's reference length.  Launched only under a table.
__global__ __launch_bounds__(PB) void pk_mask_long(PackSrc s, const uint32_t *gen_idx, PackTotals *tot, PrimerTab pt)
{
    const uint32_t n = tot->n_gen;
    for (uint32_t i0 = blockIdx.x * PB; i0 < n; i0 += gridDim.x * PB) {        // (uniform: every lane of a wavefront reaches the ballot)
        const uint32_t i = i0 + threadIdx.x;
        bool masked = false;
        if (i < n) {
            const ReadView v = view(s, (int64_t)gen_idx[i]);
            int32_t span = 0;
            for (uint32_t k = 0; k < v.n_cigar; ++k) {
                const uint32_t cw = ld_u32(v.cigar + 4 * (size_t)k);
                if (consumes_ref(cw & 0xFu)) span += (int32_t)(cw >> 4);
            }
            const int32_t p = v.pos + shift_of(s, v.tid), q = p + span - 1;
            masked = seg_find(pt.seg, pt.n_head, p, p) > p || seg_find(pt.seg + 3 * pt.n_head, pt.n_tail, q, q + 1) <= q;
        }
        count_masked(masked, tot);
    }
}

} // namespace

// ---- host side ------------------------------------------------------------------------------------------------------------
// a read set's allocation: from the context's pool of freed read sets when one of about this size lies there
static char *take_blob(tcmi_ctx *ctx, tcmi_readset *rs, size_t want)
{
    for (size_t k = 0; k < ctx->blob_pool.size(); ++k)
        if (ctx->blob_pool[k].bytes >= want && ctx->blob_pool[k].bytes <= want + want / 2 + (1 << 20)) {
            char *blob = ctx->blob_pool[k].p;
            rs->blob_bytes = ctx->blob_pool[k].bytes;
            ctx->blob_pool.erase(ctx->blob_pool.begin() + (long)k);
            return blob;
        }
    char *blob = nullptr;
    if (hipMalloc((void **)&blob, want + want / 16) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    rs->blob_bytes = want + want / 16;
    return blob;
}

// one allocation for everything the tally kernel reads: headers | planes | chunk records | runs | events, and 256 bytes of slack
// behind the last array (pk_pack zeroes them); under a base-quality floor or a primer table (drop != nullptr) the drop plane behind the slack: one word
// per pair of the plane stream, *drop_bytes of them — the caller zeroes it in front of its plane kernel, inside the pack bracket
// (zero_drop): the pair in front of the first read and the stream's slack stay zero, the packers write every other word
static int carve_blob(tcmi_ctx *ctx, tcmi_readset *rs, size_t n_reads, uint32_t word_cap, uint32_t chunk_cap, uint32_t event_cap, PackOut *o, uint32_t **drop,
                      size_t *drop_bytes)
{
    const size_t b_len = tcmi_align256(n_reads * 4), b_seq = tcmi_align256((size_t)word_cap * 4), b_run = b_len,
                 b_chk = tcmi_align256((size_t)chunk_cap * sizeof(tcmi_fast_chunk)), b_ev = tcmi_align256((size_t)event_cap * 4);
    const size_t b_drop = drop ? tcmi_align256(((size_t)word_cap / 2 + 1) * 4) : 0;
    const size_t want = b_len + b_seq + b_chk + b_run + b_ev + 256 + b_drop;
    char *blob = take_blob(ctx, rs, want);
    if (!blob) return tcmi_fail(ctx, TCMI_E_NOMEM, "hipMalloc(%zu) for the packed read set failed", want + want / 16);
    rs->d_blob = blob;
    o->lenoff = (uint32_t *)blob;
    o->seq = (uint32_t *)(blob + b_len);
    o->chunks = (tcmi_fast_chunk *)(blob + b_len + b_seq);
    o->covrun = (uint32_t *)(blob + b_len + b_seq + b_chk);
    o->events = (uint32_t *)(blob + b_len + b_seq + b_chk + b_run);
    o->word_cap = word_cap; o->chunk_cap = chunk_cap; o->event_cap = event_cap;
    o->slack = reinterpret_cast<uint32_t *>(blob + b_len + b_seq + b_chk + b_run + b_ev);
    if (drop) { *drop = reinterpret_cast<uint32_t *>(blob + b_len + b_seq + b_chk + b_run + b_ev + 256); *drop_bytes = b_drop; }
    return TCMI_OK;
}

// (queued like the launches beside it: an error is what hipGetLastError says behind the bracket's end — nothing returns from inside it)
static void zero_drop(tcmi_ctx *ctx, uint32_t *drop, size_t bytes)
{
    if (drop) (void)hipMemsetAsync(drop, 0, bytes, ctx->stream);
}

static void point_at_blob(tcmi_readset *rs, const PackOut &o, uint32_t *drop)       // (the several-kernel packer: only once it has succeeded)
{
    rs->d_flenoff = o.lenoff; rs->d_fseq = o.seq; rs->d_fchunk = o.chunks; rs->d_fcovrun = o.covrun; rs->d_fevent = o.events; rs->d_fdrop = drop;
}

// what the packed set takes of its allocation
static int64_t packed_bytes(const PackTotals &tot)
{
    return (int64_t)tot.n_kept * 4 + ((int64_t)tot.n_words + 4) * 4 + (int64_t)tot.n_chunks * (int64_t)sizeof(tcmi_fast_chunk) + (int64_t)tot.n_runs * 4 +
           (int64_t)tot.n_events * 4;
}

// ---- what both packers do on the host, once each ------------------------------------------------------------------------------------------
// The plane rules a read set was built under (its record: tcmi_read_rules): the base-quality floor, the primer table, the mate rule —
// the caller points pt.clip at the join's array once it has one —, the duplicate rule, which raises the same clip[] (join: either of
// the two is on, the join runs), and whether they give the read set a drop plane and the BQ plane kernel.
struct PlaneRules { uint32_t min_bq; PrimerTab pt; bool mate, drop_on, dedup, join; };
static PlaneRules plane_rules(const tcmi_readset *rs)
{
    PlaneRules r = {(uint32_t)rs->rules.min_bq, tcmi_primer_args(rs->rules.primers), rs->rules.mate != 0, false, false, false};
    r.dedup = rs->rules.dedup != 0;
    r.join = r.mate || r.dedup;
    r.drop_on = r.min_bq || r.pt.seg || r.join;
    return r;
}

// how the context wants chunks cut: stages per chunk, and whether pk_pack's workgroups take long chunks but a multiple of the tally
// kernel's resident workgroups (`slots`) of them, as the host packer does (pack_caps.h: pk_chunk_rule)
struct ChunkOpts { int n_stages; bool balance; int64_t slots; };
static ChunkOpts chunk_opts(const tcmi_ctx *ctx)
{
    return {ctx->chunk_stages > 0 ? std::min(ctx->chunk_stages, TCMI_F_MAXSTAGE) : TCMI_F_MAXSTAGE, ctx->chunk_stages == 0 && ctx->balance_chunks,
            (int64_t)ctx->n_cu * ctx->wg_per_cu};
}

// arrays [from, to) of a packer's scratch list from the arena; false, and nothing taken: the reservation does not hold them
template <int N> static bool take_scratch(tcmi_ctx *ctx, PkScratch<N> &s, int from, int to)
{
    if (s.end(ctx->dev_arena.used, from, to) > ctx->dev_arena.cap) return false;
    s.take([ctx](size_t bytes) { return tcmi_arena_take(ctx, bytes); }, from, to);
    return true;
}

// the stream and its record index stay in the arena until this context's next upload: whatever walks the records later (the long reads'
// tally, the mate join's clip, the record-stream counts) finds them through the read set
static void keep_stream(tcmi_ctx *ctx, tcmi_readset *rs, const uint8_t *stream, const uint64_t *rec_off)
{
    rs->d_stream = stream; rs->d_rec_off = rec_off; rs->arena_epoch = ctx->arena_epoch;
}

// the mate join's four counters out of the pinned buffer (behind a wait of the host for whatever brought them there)
static void take_mate_counts(tcmi_ctx *ctx, tcmi_readset *rs, const char *h_pin, const ReportPin &pin)
{
    const unsigned long long *h_cnt = reinterpret_cast<const unsigned long long *>(h_pin + pin.mate);
    for (int k = 0; k < 4; ++k) { rs->mate_stat[k] = (int64_t)h_cnt[k]; ctx->stat_mate[k] += rs->mate_stat[k]; }
    if (!rs->rules.dedup) return;
    const unsigned long long *h_dup = reinterpret_cast<const unsigned long long *>(h_pin + pin.dup);   // (the duplicate rule's come with them)
    for (int k = 0; k < 4; ++k) { rs->dup_stat[k] = (int64_t)h_dup[k]; ctx->stat_dup[k] += rs->dup_stat[k]; }
}

// the duplicate rule's arrays out of a packer's scratch list (first: SK_MATE_IDX / OS_MATE_IDX), mate_idx[] into the join's job
template <int N> static tcmi_dedup_job dedup_job(const PkScratch<N> &S, int first, tcmi_mate_job &mj)
{
    tcmi_dedup_job dj = {};
    mj.mate_idx = S.template at<uint32_t>(first);
    dj.ends = S.template at<tcmi_dup_end>(first + 1); dj.slot_of = S.template at<uint32_t>(first + 2); dj.dup = S.template at<uint8_t>(first + 3);
    dj.table = S.template at<unsigned long long>(first + 4);
    return dj;
}

// The read set's fields from the totals.  alg, max_end, max_len: the one-sync packer folds them from its blocks' partials, the
// several-kernel packer has them in the totals.  packed: the planes are written — false: only the classification is in (the
// several-kernel packer's first read-back: n_masked counts the long reads only so far).
static void fill_readset(tcmi_readset *rs, const PackTotals &tot, int64_t alg, int32_t max_end, int32_t max_len, bool packed)
{
    const int64_t nf = (int64_t)tot.n_kept;
    rs->n_piled = nf + (int64_t)tot.n_gen; rs->f_reads = nf; rs->alg_bytes = alg; rs->max_end = max_end; rs->max_len = max_len;
    rs->s_reads = (int64_t)tot.n_gen;
    rs->n_filtered = (int64_t)tot.n_filtered;
    rs->n_masked = (int64_t)tot.n_masked;
    if (!packed) return;
    rs->f_chunks = nf ? tot.n_chunks : 0; rs->f_words = nf ? (int64_t)tot.n_words + 4 : 0; rs->f_events = tot.n_events;
    rs->dev_bytes = packed_bytes(tot);
}

// Pack `n` reads described by `src` (device pointers) into a read set.  Returns TCMI_E_UNSUPPORTED (with `*why` set) when
// the input needs the host packer: entries longer than TCMI_D_MAXLEN, positions beyond 2^29, malformed reads (the host
// packer words the error).  The arena must already hold the source arrays; this takes its temporaries behind them.
int tcmi_pack_on_device(tcmi_ctx *ctx, const void *src_, tcmi_readset *rs, uint32_t *why)
{
    PackSrc src = *static_cast<const PackSrc *>(src_);
    *why = 0;
    const int64_t n = src.n;
    // the rules: a stream's read set was stamped where it was born (bam_device.hip: a file without a record never comes here); one of
    // flat arrays is born here, under none.  The kernels' filter and floor come from the read set's record, like everything below.
    if (src.mode != 1) tcmi_rules_stamp(rs, ctx, false);
    tcmi_rules_args(src, rs->rules);
    PlaneRules pr = plane_rules(rs);
    PrimerTab &pt = pr.pt;
    if (n > 0xFFFFFFF0ll) { *why = PKF_LONG; return TCMI_E_UNSUPPORTED; }
    const int64_t n_blk = (n + PB - 1) / PB;
    PkScratch<SK_N> S = pk_several_scratch(n, src.mode, pr.join, pr.dedup);       // (every array below: pack_caps.h lists them)
    if (!take_scratch(ctx, S, SK_INFO, SK_MATE_TABLE)) return tcmi_fail(ctx, TCMI_E_NOMEM, "internal: pack scratch under-reserved");
    uint32_t *info = S.at<uint32_t>(SK_INFO), *gen_idx = S.at<uint32_t>(SK_GEN_IDX);      // (gen_idx: a stream's; else null)
    uint2 *rd_seq = S.at<uint2>(SK_RD_SEQ), *blk_sum = S.at<uint2>(SK_BLK_SUM);
    int32_t *rd_pos = S.at<int32_t>(SK_RD_POS), *blk_end = S.at<int32_t>(SK_BLK_END);
    unsigned long long *blk_alg = S.at<unsigned long long>(SK_BLK_ALG);
    PackTotals *d_tot = S.at<PackTotals>(SK_TOT);
    const ReportPin pin(0);                     // (pinned: the two read-backs below, and the mate join's counters)
    PackTotals *h_tot = (PackTotals *)tcmi_ctx_pinned(ctx, pin.bytes);
    if (!h_tot) return tcmi_fail(ctx, TCMI_E_NOMEM, "pinned scratch for the packer's totals");
    std::memset(h_tot, 0, sizeof *h_tot);
    PackTotals &tot = *h_tot;
    TCMI_HIP(ctx, hipMemsetAsync(d_tot, 0, sizeof(PackTotals), ctx->stream));
    bool counts_owed = false;
    const int32_t n_lay = ctx->layout.n();
    std::vector<int32_t> h_ext((size_t)n_lay);
    if (n_lay) {                            // the context's contig layout (tcmi_ctx_set_layout): its table, the extents zeroed
        src.lay = ctx->d_lay; src.lay_ext = ctx->d_lay + 2 * n_lay; src.n_lay = n_lay;
        TCMI_HIP(ctx, hipMemsetAsync(src.lay_ext, 0, (size_t)n_lay * 4, ctx->stream));
    }
    if (n > 0) {
        (void)hipGetLastError();
        tcmi_prof_begin(ctx, TCMI_K_PACK_CLASSIFY);
        hipLaunchKernelGGL(pk_classify, dim3((unsigned)n_blk), dim3(PB), 0, ctx->stream, src, info, rd_seq, rd_pos, blk_sum, blk_alg, blk_end, d_tot, gen_idx);
        hipLaunchKernelGGL(pk_scan, dim3(1), dim3(1024), 0, ctx->stream, blk_sum, blk_alg, blk_end, n_blk, d_tot);
        if (pt.seg && gen_idx) hipLaunchKernelGGL(pk_mask_long, dim3(64), dim3(PB), 0, ctx->stream, src, gen_idx, d_tot, pt);
        tcmi_prof_end(ctx, TCMI_K_PACK_CLASSIFY);
        TCMI_HIP(ctx, hipGetLastError());
    }
    TCMI_HIP(ctx, hipMemcpyAsync(h_tot, d_tot, sizeof tot, hipMemcpyDeviceToHost, ctx->stream));
    if (n_lay) TCMI_HIP(ctx, hipMemcpyAsync(h_ext.data(), src.lay_ext, (size_t)n_lay * 4, hipMemcpyDeviceToHost, ctx->stream));
    TCMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (tot.flags & PKF_SLOT_OVF) {         // (the host packer / host reader word it with the contig's name: the caller falls back to them)
        *why = tot.flags;
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "read %lld on reference %d ends past the end of its contig's slot", (long long)(tot.slot_ovf >> 24) - 1,
                         (int)(tot.slot_ovf & 0xFFFFFF));
    }
    if (tot.flags) { *why = tot.flags; return TCMI_E_UNSUPPORTED; }
    const int64_t nf = (int64_t)tot.n_kept;
    rs->n_lay = n_lay; rs->d_lay = src.lay; rs->lay_gen = ctx->lay_gen; rs->n_dropped = (int64_t)tot.n_dropped;
    rs->ref_ext.assign(h_ext.begin(), h_ext.end());
    fill_readset(rs, tot, (int64_t)tot.alg_bytes, tot.max_end, (int32_t)tot.max_len, false);
    rs->packed_on_device = 1;
    if (pr.join && n > 0) {
        // the mate join (and the duplicate rule behind it), in front of the plane kernel: the record count is the host's here; its counters are copied now and read behind
        // the next wait this function makes anyway (take_counts)
        if (!take_scratch(ctx, S, SK_MATE_TABLE, SK_C_IDX)) return tcmi_fail(ctx, TCMI_E_NOMEM, "internal: mate join scratch under-reserved");
        tcmi_mate_job mj = {};
        mj.src = src; mj.stream_len = ~0ull;                    // (the host has checked the record chain: every record ends inside the stream)
        mj.n = n; mj.rec_cap = (uint32_t)n;
        mj.table = S.at<unsigned long long>(SK_MATE_TABLE);
        mj.clip = S.at<uint32_t>(SK_CLIP);
        mj.apply = pr.mate;
        tcmi_dedup_job dj = {};
        if (pr.dedup) dj = dedup_job(S, SK_MATE_IDX, mj);
        if (const int rc = tcmi_mate_join_enqueue(ctx, mj, pr.dedup ? &dj : nullptr)) return rc;
        TCMI_HIP(ctx, hipMemcpyAsync(reinterpret_cast<char *>(h_tot) + pin.mate, tcmi_mate_counters(mj), 32, hipMemcpyDeviceToHost, ctx->stream));
        if (pr.dedup) {
            TCMI_HIP(ctx, hipMemcpyAsync(reinterpret_cast<char *>(h_tot) + pin.dup, tcmi_dup_counters(mj, dj), 32, hipMemcpyDeviceToHost, ctx->stream));
            rs->d_dup = dj.dup;
        }
        counts_owed = true;
        rs->d_clip = mj.clip; pt.clip = mj.clip;
        keep_stream(ctx, rs, src.stream, src.rec_off);
    }
    auto take_counts = [&]() {              // (behind a wait of the host for the stream)
        if (counts_owed) take_mate_counts(ctx, rs, reinterpret_cast<const char *>(h_tot), pin);
        counts_owed = false;
    };
    if (tot.n_gen) {                        // long reads: tallied from the stream
        keep_stream(ctx, rs, src.stream, src.rec_off);
        rs->d_gen_idx = gen_idx;
    }
    if (nf == 0) {                          // (long reads only: nothing else is queued — the counters get a wait of their own)
        if (counts_owed) TCMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
        take_counts();
        return TCMI_OK;
    }
    if (tot.n_words > PK_WORD_MOST) { *why = PKF_WORD_OVF; return TCMI_E_UNSUPPORTED; }

    // reads per pk_pack workgroup, its grid and the read set's capacities: from the exact count (its twin from a capacity: pk_pack, dev_slots > 0)
    const ChunkOpts co = chunk_opts(ctx);
    const PkCaps cr = pk_chunk_rule(nf, tot.n_words + PK_WORD_SLACK, true, co.slots, co.balance, (int64_t)tot.max_end);

    pk_several_kept(S, nf);
    if (!take_scratch(ctx, S, SK_C_IDX, SK_N)) return tcmi_fail(ctx, TCMI_E_NOMEM, "internal: pack scratch under-reserved");
    uint32_t *c_idx = S.at<uint32_t>(SK_C_IDX), *c_info = S.at<uint32_t>(SK_C_INFO), *c_woff = S.at<uint32_t>(SK_C_WOFF);
    int32_t *c_pos = S.at<int32_t>(SK_C_POS);
    uint2 *c_seq = S.at<uint2>(SK_C_SEQ);

    uint32_t event_cap = cr.event_cap;
    const uint32_t h_masked_long = tot.n_masked;
    for (int attempt = 0;; ++attempt) {
        PackOut o = {};
        uint32_t *drop = nullptr;
        size_t drop_bytes = 0;
        if (const int rc = carve_blob(ctx, rs, (size_t)nf, (uint32_t)cr.word_cap, cr.chunk_cap, event_cap, &o, pr.drop_on ? &drop : nullptr, &drop_bytes)) return rc;
        if (attempt > 0) TCMI_HIP(ctx, hipMemsetAsync(&d_tot->n_chunks, 0, 4 * sizeof(uint32_t), ctx->stream));    // n_chunks, n_events, n_runs, word_cursor (the first time: pk_scan)
        if (attempt > 0 && pt.seg) TCMI_HIP(ctx, hipMemcpyAsync(&d_tot->n_masked, &h_masked_long, 4, hipMemcpyHostToDevice, ctx->stream));    // (the plane kernel counts its reads again)
        (void)hipGetLastError();
        tcmi_prof_begin(ctx, TCMI_K_PACK);
        zero_drop(ctx, drop, drop_bytes);
        if (attempt == 0)
            hipLaunchKernelGGL(pk_scatter, dim3((unsigned)n_blk), dim3(PB), 0, ctx->stream, src, info, rd_seq, rd_pos, blk_sum, c_idx, c_pos, c_info, c_woff, c_seq);
        hipLaunchKernelGGL(pk_pack, dim3((unsigned)cr.n_wg), dim3(PB), 0, ctx->stream, o, c_pos, c_info, c_woff, (uint32_t)nf,
                           (uint32_t)tot.n_words, (int)cr.reads_per_wg, co.n_stages, ctx->stage_cap, d_tot, (int64_t)0);
        if (pr.drop_on)
            hipLaunchKernelGGL(pk_planes_bq, dim3((unsigned)((nf + PB - 1) / PB)), dim3(PB), 0, ctx->stream, src, o, c_idx, c_pos, c_info, c_woff, c_seq,
                               (uint32_t)nf, (uint32_t)tot.n_words, d_tot, drop, pr.min_bq, pt);
        else
            hipLaunchKernelGGL(pk_planes, dim3((unsigned)((nf + PB - 1) / PB)), dim3(PB), 0, ctx->stream, src, o, c_idx, c_pos, c_info, c_woff, c_seq,
                               (uint32_t)nf, (uint32_t)tot.n_words, d_tot);
        tcmi_prof_end(ctx, TCMI_K_PACK);
        TCMI_HIP(ctx, hipGetLastError());
        TCMI_HIP(ctx, hipMemcpyAsync(h_tot, d_tot, sizeof tot, hipMemcpyDeviceToHost, ctx->stream));
        TCMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
        take_counts();
        if (tot.n_events > event_cap && attempt == 0) {          // rare: a read set full of N / indel tokens — once more with room for all
            (void)hipFree(rs->d_blob);
            rs->d_blob = nullptr;
            rs->blob_bytes = 0;
            event_cap = tot.n_events + 1024;
            continue;
        }
        if (tot.flags || tot.n_events > event_cap) {
            *why = tot.flags ? tot.flags : (uint32_t)PKF_EVENT_OVF;
            return TCMI_E_UNSUPPORTED;
        }
        point_at_blob(rs, o, drop);
        if (src.mode == 1) {
            keep_stream(ctx, rs, src.stream, src.rec_off);
            rs->d_cidx = c_idx; rs->d_cpos = c_pos;
        }
        fill_readset(rs, tot, (int64_t)tot.alg_bytes, tot.max_end, (int32_t)tot.max_len, true);
        return TCMI_OK;
    }
}

// what the host checks after its one wait, stored by the kernel itself into pinned host memory (a copy command between two kernels
// costs the stream 40 - 100 us of hand-over between the copy engine and the compute queue; these stores cross PCIe on their own)
// (mate: the mate join's four counters, null when the setting is off; they land behind everything else of the pinned buffer)
__global__ __launch_bounds__(256) void pk_report(const PackTotals *tot, const unsigned long long *blk_alg, const int32_t *blk_end, const uint32_t *stat,
                                                 int32_t nb, PackTotals *h_tot, unsigned long long *h_alg, int32_t *h_end, uint32_t *h_stat,
                                                 const unsigned long long *mate, unsigned long long *h_mate, const unsigned long long *dup)
{
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i < nb) { h_alg[i] = blk_alg[i]; h_end[i] = blk_end[i]; h_stat[i] = stat[i]; }
    if (i == 0) *h_tot = *tot;
    if (mate && i < 4) h_mate[i] = mate[i];
    if (dup && i < 4) h_mate[4 + i] = dup[i];               // (the duplicate rule's four, behind the join's: ReportPin::dup)
}

// ---- the one-sync path: pk_index + pk_place + pk_pack queued from capacities, checked after the caller's one wait ------------------------------
int tcmi_pack_fused_enqueue(tcmi_ctx *ctx, tcmi_fused_job *job, tcmi_readset *rs)
{
    // capacities: what the arrays of the packed read set are sized for (a file beyond them takes the several-kernel path)
    const ChunkOpts co = chunk_opts(ctx);
    const PkCaps caps = job->caps = pk_one_sync_caps(job->stream_len, job->rec_hint, job->safe_caps, job->len_bound, co.slots, co.balance);
    const int64_t nb = job->n_blocks, cap = caps.rec_cap;
    if (cap > PK_REC_MOST) return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "too many records for the one-pass packer");
    tcmi_rules_stamp(rs, ctx, true);
    PlaneRules pr = plane_rules(rs);
    const bool prefix = pk_prefix_on(ctx->prefix_kernels, nb);
    PkScratch<OS_N> S = pk_one_sync_scratch(cap, nb, pr.join, prefix, pr.dedup);      // (every array below: pack_caps.h lists them)
    if (!take_scratch(ctx, S, 0, OS_N)) return tcmi_fail(ctx, TCMI_E_NOMEM, "internal: one-pass packer scratch under-reserved");
    PackTotals *d_tot = S.at<PackTotals>(OS_TOT);
    unsigned long long *pre = S.at<unsigned long long>(OS_PRE);
    job->d_rec = S.at<uint64_t>(OS_REC_OFF); job->c_idx = S.at<uint32_t>(OS_C_IDX); job->c_pos = S.at<int32_t>(OS_C_POS); job->gen_idx = S.at<uint32_t>(OS_GEN_IDX);
    tcmi_mate_job mj = {};
    mj.table = S.at<unsigned long long>(OS_MATE_TABLE); mj.clip = S.at<uint32_t>(OS_CLIP);      // (null without the rule)
    job->d_tot = d_tot;
    job->h_pin = (char *)tcmi_ctx_pinned(ctx, ReportPin(nb).bytes);
    if (!job->h_pin) return tcmi_fail(ctx, TCMI_E_NOMEM, "pinned scratch for the packer's totals");
    if (caps.word_cap > PK_WORD_MOST) return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "too many plane words for the one-pass packer");
    PackOut o = {};
    PrimerTab &pt = pr.pt;
    pt.clip = mj.clip;
    uint32_t *drop = nullptr;
    size_t drop_bytes = 0;
    if (const int rc = carve_blob(ctx, rs, (size_t)cap, (uint32_t)caps.word_cap, caps.chunk_cap, caps.event_cap, &o, pr.drop_on ? &drop : nullptr, &drop_bytes)) return rc;
    TCMI_HIP(ctx, hipMemsetAsync(d_tot, 0, sizeof(PackTotals), ctx->stream));
    FusedArgs a = {};
    a.stream = job->d_stream; a.stream_len = job->stream_len; a.blocks = static_cast<const BlockDesc *>(job->d_desc);
    a.rec_slot = job->d_slot; a.n_rec = job->d_nrec; a.first = job->d_first; a.over = job->d_over; a.stat = job->d_stat;
    a.n_blocks = (int32_t)nb; a.n_own = (int32_t)job->n_own; a.ranged = job->ranged;
    a.agg = S.at<uint2>(OS_AGG); a.fn = S.at<unsigned long long>(OS_FN); a.rec_base = S.at<uint32_t>(OS_REC_BASE); a.rrec = S.at<uint4>(OS_RREC); a.rec_off = job->d_rec; a.rec_cap = (uint32_t)cap;
    a.c_idx = job->c_idx; a.c_pos = job->c_pos; a.c_info = S.at<uint32_t>(OS_C_INFO); a.c_woff = S.at<uint32_t>(OS_C_WOFF); a.c_seq = S.at<uint2>(OS_C_SEQ); a.gen_idx = job->gen_idx;
    a.o = o; a.blk_alg = S.at<unsigned long long>(OS_BLK_ALG); a.blk_end = S.at<int32_t>(OS_BLK_END); a.tot = d_tot;
    tcmi_rules_args(a, rs->rules);
    a.drop = drop;
    a.pt = pt;
    const size_t pre_n = pk_prefix_words(nb);
    if (prefix) { a.pre_rec = pre; a.pre_k = pre + pre_n; a.pre_w = pre + 2 * pre_n; }
    (void)hipGetLastError();
    tcmi_prof_begin(ctx, TCMI_K_PACK_CLASSIFY);
    if (prefix) hipLaunchKernelGGL(pk_prefix, dim3(1), dim3(1024), 0, ctx->stream, job->d_nrec, 1, (int)nb, (int)job->n_own, pre);
    hipLaunchKernelGGL(pk_index, dim3((unsigned)nb), dim3(PB), 0, ctx->stream, a);
    tcmi_prof_end(ctx, TCMI_K_PACK_CLASSIFY);
    TCMI_HIP(ctx, hipGetLastError());
    if (pr.join) {
        // the mate join (and the duplicate rule behind it) between pk_index and pk_place_bq: nobody has read the record count back — its kernels take it from what pk_index
        // left, their grid is sized from the capacity
        mj.src.stream = job->d_stream; mj.src.rec_off = job->d_rec; mj.src.mode = 1; mj.src.n = cap; mj.src.flt = a.flt;
        mj.stream_len = job->stream_len; mj.n = -1; mj.rec_cap = (uint32_t)cap;
        mj.rec_base = a.rec_base; mj.n_rec = job->d_nrec; mj.n_blocks = (int32_t)nb; mj.n_own = (int32_t)job->n_own;
        mj.flags = &d_tot->flags; mj.ovf = PKF_REC_OVF;
        mj.apply = pr.mate;
        tcmi_dedup_job dj = {};
        if (pr.dedup) dj = dedup_job(S, OS_MATE_IDX, mj);
        if (const int rc = tcmi_mate_join_enqueue(ctx, mj, pr.dedup ? &dj : nullptr)) return rc;
        job->d_mate_cnt = tcmi_mate_counters(mj);
        if (pr.dedup) { job->d_dup_cnt = tcmi_dup_counters(mj, dj); rs->d_dup = dj.dup; }
        rs->d_clip = mj.clip;
    }
    tcmi_prof_begin(ctx, TCMI_K_PACK);
    zero_drop(ctx, drop, drop_bytes);
    if (prefix) {
        hipLaunchKernelGGL(pk_prefix, dim3(1), dim3(1024), 0, ctx->stream, reinterpret_cast<const uint32_t *>(a.agg), 2, (int)nb, (int)nb, pre + pre_n);
        hipLaunchKernelGGL(pk_prefix, dim3(1), dim3(1024), 0, ctx->stream, reinterpret_cast<const uint32_t *>(a.agg) + 1, 2, (int)nb, (int)nb, pre + 2 * pre_n);
    }
    if (pr.drop_on) hipLaunchKernelGGL(pk_place_bq, dim3((unsigned)nb), dim3(PB), 0, ctx->stream, a);
    else hipLaunchKernelGGL(pk_place, dim3((unsigned)nb), dim3(PB), 0, ctx->stream, a);
    if (pt.seg) {
        PackSrc ls = {};
        ls.stream = job->d_stream; ls.rec_off = job->d_rec; ls.mode = 1; ls.n = cap;
        hipLaunchKernelGGL(pk_mask_long, dim3(64), dim3(PB), 0, ctx->stream, ls, job->gen_idx, d_tot, pt);
    }
    hipLaunchKernelGGL(pk_pack, dim3((unsigned)caps.n_wg), dim3(PB), 0, ctx->stream, o, job->c_pos, a.c_info, a.c_woff, 0u, 0u, 0, co.n_stages, ctx->stage_cap, d_tot,
                       co.balance ? co.slots : (int64_t)1 << 30);
    tcmi_prof_end(ctx, TCMI_K_PACK);
    TCMI_HIP(ctx, hipGetLastError());
    // (the report of the packer's verdicts is queued by tcmi_pack_fused_report, behind whatever the caller queues behind the packer)
    job->d_blk_alg = a.blk_alg; job->d_blk_end = a.blk_end;
    // the read set as the tally launch needs it before anyone has read the totals: capacities + where the real counts lie
    rs->packed_on_device = 1;
    point_at_blob(rs, o, drop);
    rs->f_chunks = caps.chunk_cap; rs->f_events = caps.event_cap;
    rs->d_dev_counts = &d_tot->n_chunks;
    static_assert(offsetof(PackTotals, n_events) == offsetof(PackTotals, n_chunks) + 4, "the tally kernel reads {n_chunks, n_events}");
    rs->n_piled = 1;                            // (unknown yet: "there may be reads")
    rs->max_end = 0;
    keep_stream(ctx, rs, job->d_stream, job->d_rec);
    rs->d_cidx = job->c_idx; rs->d_cpos = job->c_pos; rs->d_gen_idx = job->gen_idx;
    return TCMI_OK;
}

// the last launch of the one-sync path's chain: totals and per-block verdicts into the job's pinned buffer
int tcmi_pack_fused_report(tcmi_ctx *ctx, tcmi_fused_job *job)
{
    const int64_t nb = job->n_blocks;
    const ReportPin pin(nb);
    char *h = job->h_pin;
    (void)hipGetLastError();
    hipLaunchKernelGGL(pk_report, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, ctx->stream, static_cast<const PackTotals *>(job->d_tot),
                       static_cast<const unsigned long long *>(job->d_blk_alg), static_cast<const int32_t *>(job->d_blk_end), job->d_stat, (int32_t)nb,
                       reinterpret_cast<PackTotals *>(h), reinterpret_cast<unsigned long long *>(h + pin.alg), reinterpret_cast<int32_t *>(h + pin.end),
                       reinterpret_cast<uint32_t *>(h + pin.stat), static_cast<const unsigned long long *>(job->d_mate_cnt),
                       reinterpret_cast<unsigned long long *>(h + pin.mate), static_cast<const unsigned long long *>(job->d_dup_cnt));
    TCMI_HIP(ctx, hipGetLastError());
    return TCMI_OK;
}

int tcmi_pack_fused_finish(tcmi_ctx *ctx, tcmi_fused_job *job, tcmi_readset *rs, uint32_t *why)
{
    const int64_t nb = job->n_blocks;
    const ReportPin pin(nb);
    const PackTotals &tot = *reinterpret_cast<const PackTotals *>(job->h_pin);
    const unsigned long long *blk_alg = reinterpret_cast<const unsigned long long *>(job->h_pin + pin.alg);
    const int32_t *blk_end = reinterpret_cast<const int32_t *>(job->h_pin + pin.end);
    const uint32_t *stat = reinterpret_cast<const uint32_t *>(job->h_pin + pin.stat);
    uint32_t flags = tot.flags | pk_beyond_caps(job->caps, tot.n_rec, tot.n_words, tot.n_chunks, tot.n_events);
    for (int64_t b = 0; b < nb; ++b) if (stat[b] != ST_OK) flags |= PKF_STAT;
    *why = flags;
    rs->d_dev_counts = nullptr;
    if (flags) return TCMI_E_UNSUPPORTED;
    unsigned long long alg = 0, mlen = 0;
    int32_t mend = 0;
    for (int64_t b = 0; b < nb; ++b) { alg += blk_alg[b] & 0xFFFFFFFFFFFFull; mlen = std::max(mlen, blk_alg[b] >> 48); mend = std::max(mend, blk_end[b]); }
    rs->n_reads = (int64_t)tot.n_rec;
    fill_readset(rs, tot, (int64_t)alg, mend, (int32_t)mlen, true);
    if (job->d_mate_cnt) take_mate_counts(ctx, rs, job->h_pin, pin);
    rs->range_first = tot.range_first ? (int64_t)(tot.range_first - 1ull) : -1;
    rs->range_next = tot.range_next ? (int64_t)(tot.range_next - 1ull) : -1;
    return TCMI_OK;
}

// the flat arrays of struct tcmi_reads -> device (one arena block) -> tcmi_pack_on_device
int tcmi_upload_and_pack_on_device(tcmi_ctx *ctx, const tcmi_reads *r, tcmi_readset *rs, uint32_t *why)
{
    *why = 0;
    const int64_t n = r->n_reads;
    const size_t n_cig = n ? (size_t)r->cigar_off[n] : 0, n_seq = n ? (size_t)r->seq_off[n] : 0;
    const size_t b_n4 = tcmi_align256((size_t)n * 4), b_off = tcmi_align256((size_t)(n + 1) * 8);
    const size_t sz[8] = {b_n4, tcmi_align256((size_t)n * 2), b_n4, r->tid ? b_n4 : 0, b_off, tcmi_align256(n_cig * 4 + 64), b_off, tcmi_align256(n_seq + 128)};
    size_t src_bytes = 0;
    for (size_t b : sz) src_bytes += b + 256;
    const size_t tmp_bytes = pk_several_scratch(n, 0, false).end(0) + 256;      // (what tcmi_pack_on_device takes: no flat arrays under the mate rule)
    int rc = tcmi_arena_reserve(ctx, src_bytes + tmp_bytes);
    if (rc) return rc;
    PackSrc s = {};
    s.mode = 0; s.n = n; s.pos_shift = 0;
    struct Item { const void *h; size_t bytes, room; const void **d; };
    const Item items[8] = {{r->pos, (size_t)n * 4, sz[0], (const void **)&s.pos}, {r->flag, (size_t)n * 2, sz[1], (const void **)&s.flag},
                           {r->l_qseq, (size_t)n * 4, sz[2], (const void **)&s.l_qseq}, {r->tid, (size_t)n * 4, sz[3], (const void **)&s.tid},
                           {r->cigar_off, (size_t)(n + 1) * 8, sz[4], (const void **)&s.cigar_off}, {r->cigar, n_cig * 4, sz[5], (const void **)&s.cigar},
                           {r->seq_off, (size_t)(n + 1) * 8, sz[6], (const void **)&s.seq_off}, {r->seq, n_seq, sz[7], (const void **)&s.seq}};
    for (const Item &it : items) {
        if (!it.h || it.room == 0) { *it.d = nullptr; continue; }
        char *d = (char *)tcmi_arena_take(ctx, it.room);
        *it.d = d;
        if (it.bytes) TCMI_HIP(ctx, hipMemcpyAsync(d, it.h, it.bytes, hipMemcpyHostToDevice, ctx->stream));
        TCMI_HIP(ctx, hipMemsetAsync(d + it.bytes, 0, it.room - it.bytes, ctx->stream));   // the 24-byte window loads of fetch32 may run past the last read
    }
    if (n == 0) { rs->packed_on_device = 1; return TCMI_OK; }
    return tcmi_pack_on_device(ctx, &s, rs, why);
}
