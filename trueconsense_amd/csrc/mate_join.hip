// mate_join.hip — --mate-overlap on gfx950: for every record of a device-decoded stream, the columns at its head that its mate counts
// already (include/tcmi.h: tcmi_ctx_set_mate_overlap; the rule: mate_rule.h).  A hash join over the records where they lie, between the
// packers' classification and their plane kernels (pack_device.hip), launched only when the setting is on.
//
// The table: open addressing in global memory, 8-byte entries {32-bit tag of the key's hash << 32 | record index + 1}, 0: empty; a power
// of two of at least twice the record capacity, so it cannot fill; the four counters behind it; both zeroed by one hipMemsetAsync;
// nothing is ever deleted.
//   mate_build_kernel   one lane per record (stream_count.h's each_record): a kept, eligible record hashes its key — FNV-1a over the
//                       name, refID, min and max of pos and next_pos — and takes the first empty slot from the hash's on: linear probing,
//                       one 64-bit atomicCAS per slot tried, no slot is tried twice; it gives up once it has met three members of its
//                       own group (ambiguous either way), so a group's chain holds at most three of them.
//   mate_probe_kernel   a launch of its own — the only ordering between build and probe: no lane waits for another workgroup, nothing
//                       spins.  Every eligible record walks its chain from the hash's slot to the first empty one; an entry with its
//                       tag is compared field by field (the key's integers, then the name: equal lengths, dwords through ld_u32, a
//                       masked tail) and counted, up to three.  A group of one or two is walked to the chain's end, so its size and
//                       its other member do not depend on the order in which the build's lanes arrived, and "three or more" does not
//                       either: every run gives the same clip[].  A group of two is put to
//                       the pair test; the pair's loser gets its clip.  clip[i] is written for every record below the record count,
//                       0 for all others.  The four counters: one ballot per wavefront, the sums by shuffles, one atomic per counter
//                       that is not zero.
// Under the duplicate rule (dedup.hip) the probe also leaves every pair's two records each other's index + 1 in mate_idx[], and with
// that rule alone (apply == 0) nothing else: clip[] is zeros, the counters stay 0.
// Which record is kept and where it lies (kept_span), the unaligned loads (ld_u32): pack_device.h.  The stream is only read.
#include "stream_count.h"
#include "mate_rule.h"

namespace {

constexpr int BLOCK = SC_BLOCK;
using MjArgs = tcmi_mate_job;           // the kernels take the job as it is, and the table's mask beside it (the record count: stream_count.h)

// one record as the join sees it: the rule's fields and the name
struct Mate {
    tcmi_mate_fields f;
    const uint8_t *name;
    uint32_t n_name;                    // without the NUL
};

__device__ inline Mate mate_of(const uint8_t *rec, const ReadView &v)
{
    Mate m;
    m.f.flag = v.flag; m.f.tid = v.tid; m.f.pos = v.pos;
    m.f.next_tid = (int32_t)ld_u32(rec + 4 + 20); m.f.next_pos = (int32_t)ld_u32(rec + 4 + 24);
    m.name = rec + 4 + 32;
    m.n_name = (ld_u32(rec + 4 + 8) & 0xFFu) - 1u;             // (l_read_name >= 1: view_rec calls a record without it bad)
    return m;
}

// record i -> is it kept and eligible?  [p, q]: its columns.  Nothing of a record that claims to lie or end behind the stream is followed.
__device__ inline bool open_mate(const MjArgs &a, int64_t i, Mate &m, int64_t &p, int64_t &q)
{
    const uint64_t roff = a.src.rec_off[i];
    if (roff + 36ull > a.stream_len) return false;
    const uint8_t *rec = a.src.stream + roff;
    if (roff + 4ull + ld_u32(rec) > a.stream_len) return false;
    ReadView v;
    if (!kept_span(a.src, i, v, p, q)) return false;
    m = mate_of(rec, v);
    return tcmi_mate_eligible(m.f);
}

__device__ inline uint64_t hash_of(const Mate &m)
{
    uint64_t h = TCMI_MATE_FNV_BASIS;
    uint32_t k = 0;
    for (; k + 4 <= m.n_name; k += 4) h = tcmi_mate_hash_word(h, ld_u32(m.name + k));
    if (k < m.n_name) h = tcmi_mate_hash_word(h, ld_u32(m.name + k), (int)(m.n_name - k));     // (the load ends inside the record: the NUL, the CIGAR or SEQ follow)
    return tcmi_mate_hash_finish(h, m.f);
}

// (the compare itself: mate_rule.h, which tests/mate_rule_main.cpp runs over every length and every differing byte)
__device__ inline bool same_name(const Mate &a, const Mate &b)
{
    const uint8_t *na = a.name, *nb = b.name;
    return tcmi_mate_same_name(a.n_name, b.n_name, [na](uint32_t k) { return ld_u32(na + k); }, [nb](uint32_t k) { return ld_u32(nb + k); });
}

__global__ __launch_bounds__(BLOCK) void mate_build_kernel(MjArgs a, uint32_t slot_mask)
{
    const int64_t n = record_count(a);
    each_record(n, [&](int64_t i) {
        Mate m;
        int64_t p, q;
        if (i >= n || !open_mate(a, i, m, p, q)) return;
        const uint64_t h = hash_of(m);
        const unsigned long long entry = ((unsigned long long)tcmi_mate_tag(h) << 32) | (unsigned long long)(i + 1);
        uint32_t slot = (uint32_t)h & slot_mask, seen = 0;
        // (the table has twice the records' slots: an empty one comes.  A record that meets three members of its own group on its way
        //  is not entered: the group is ambiguous with or without it, and the probe of every member, entered or not, finds three — so
        //  a file whose records all share one key builds a chain of three entries, not of all of them)
        for (uint32_t tries = 0; tries <= slot_mask && seen < 3u; ++tries) {
            const unsigned long long old = atomicCAS(&a.table[slot], 0ull, entry);
            if (old == 0ull) break;
            if ((uint32_t)(old >> 32) == tcmi_mate_tag(h)) {
                const uint8_t *rec = a.src.stream + a.src.rec_off[(int64_t)(uint32_t)old - 1];
                const Mate c = mate_of(rec, view_rec(rec));
                if (tcmi_mate_same_ints(m.f, c.f) && same_name(m, c)) ++seen;
            }
            slot = (slot + 1u) & slot_mask;
        }
    });
}

__global__ __launch_bounds__(BLOCK) void mate_probe_kernel(MjArgs a, uint32_t slot_mask)
{
    const int64_t n = record_count(a);
    const int lane = threadIdx.x & 63;
    unsigned long long *cnt = a.table + (size_t)slot_mask + 1;     // (the four counters lie behind the table: one memset zeroes both)
    each_record(n, [&](int64_t i) {
        uint32_t clip = 0, pairs = 0, amb = 0, mate = 0;
        Mate m;
        int64_t p, q;
        if (i < n && open_mate(a, i, m, p, q)) {
            const uint64_t h = hash_of(m);
            const uint32_t tag = tcmi_mate_tag(h);
            uint32_t slot = (uint32_t)h & slot_mask, members = 0;
            int64_t other = -1;
            // every entry of the table is a kept, eligible record below n (the build put nothing else there): a candidate is read for its
            // fields and its name only — no CIGAR is walked here.  A third member settles the verdict: the walk ends there, so a file
            // whose records all share one key costs every lane three comparisons, not the group's size.
            for (uint32_t tries = 0; tries <= slot_mask && members < 3u; ++tries) {
                const unsigned long long e = a.table[slot];
                if (e == 0ull) break;
                if ((uint32_t)(e >> 32) == tag) {
                    const int64_t j = (int64_t)(uint32_t)e - 1;
                    if (j == i) ++members;
                    else if (j >= 0 && j < n) {
                        const uint8_t *rec = a.src.stream + a.src.rec_off[j];
                        const Mate c = mate_of(rec, view_rec(rec));
                        if (tcmi_mate_same_ints(m.f, c.f) && same_name(m, c)) { other = j; ++members; }
                    }
                }
                slot = (slot + 1u) & slot_mask;
            }
            // (members counts this record too; `other` is the one other member of a group of two)
            if (members >= 3u) amb = 1;
            else if (members == 2u && other >= 0) {
                Mate c;
                int64_t pc, qc;
                if (open_mate(a, other, c, pc, qc) && tcmi_mate_pair(m.f, c.f)) {
                    mate = (uint32_t)other + 1u;                // (from both sides: the duplicate rule's templates, dedup.hip)
                    if (a.apply && tcmi_mate_loses(m.f, c.f)) {
                        pairs = 1;                              // (a pair is counted where it loses)
                        clip = tcmi_mate_clip(p, q, qc);
                    }
                }
            }
        }
        if (!a.apply) amb = 0;                                  // (the join runs for mate_idx alone: its counters stay 0)
        if (i < n) a.clip[i] = clip;
        if (a.mate_idx && i < n) a.mate_idx[i] = mate;
        // the four counters of the wavefront.  A clip is a record's span: the packers decline a file with a column at or beyond 2^29
        // (PKF_FARPOS), so it fits the int32 that open_walk and tally_stream_kernel add it in; 64 of them do not fit 32 bits: that
        // sum is 64 bits wide.
        if (__ballot((pairs | amb) != 0u)) {
            uint32_t c0 = pairs, c1 = clip ? 1u : 0u, c3 = amb;
            unsigned long long c2 = clip;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                c0 += (uint32_t)__shfl_xor((int)c0, d, 64); c1 += (uint32_t)__shfl_xor((int)c1, d, 64);
                c2 += (unsigned long long)__shfl_xor((long long)c2, d, 64); c3 += (uint32_t)__shfl_xor((int)c3, d, 64);
            }
            if (lane == 0) {
                if (c0) atomicAdd(&cnt[0], (unsigned long long)c0);
                if (c1) atomicAdd(&cnt[1], (unsigned long long)c1);
                if (c2) atomicAdd(&cnt[2], c2);
                if (c3) atomicAdd(&cnt[3], (unsigned long long)c3);
            }
        }
    });
}

} // namespace

int tcmi_mate_join_enqueue(tcmi_ctx *ctx, const tcmi_mate_job &job, const tcmi_dedup_job *dedup)
{
    const size_t slots = tcmi_mate_slots(job.rec_cap);
    if (slots > (1ull << 32)) return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "%s: %u records are more than the join's table takes", job.apply ? "--mate-overlap" : "--dedup", job.rec_cap);
    const uint32_t slot_mask = (uint32_t)(slots - 1);
    const int64_t most = job.n >= 0 ? job.n : (int64_t)job.rec_cap;
    const int64_t blocks = (std::max<int64_t>(most, 1) + BLOCK - 1) / BLOCK;
    const unsigned grid = (unsigned)std::min<int64_t>(blocks, (int64_t)std::max(ctx->n_cu, 1) * SC_WG_PER_CU);
    (void)hipGetLastError();
    tcmi_prof_begin(ctx, TCMI_K_MATE_JOIN);
    (void)hipMemsetAsync(job.table, 0, (slots + 4) * 8, ctx->stream);          // (the table and the four counters behind it)
    hipLaunchKernelGGL(mate_build_kernel, dim3(grid), dim3(BLOCK), 0, ctx->stream, job, slot_mask);
    hipLaunchKernelGGL(mate_probe_kernel, dim3(grid), dim3(BLOCK), 0, ctx->stream, job, slot_mask);
    if (dedup) tcmi_dedup_launch(ctx, job, *dedup, grid, slot_mask);           // (the duplicate rule: the same bracket, dedup.hip)
    tcmi_prof_end(ctx, TCMI_K_MATE_JOIN);
    TCMI_HIP(ctx, hipGetLastError());
    return TCMI_OK;
}
