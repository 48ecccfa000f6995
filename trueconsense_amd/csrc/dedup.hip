// dedup.hip — --dedup on gfx950: which records of a device-decoded stream belong to a duplicate template (include/tcmi.h:
// tcmi_ctx_set_dedup; the rule: dedup_rule.h).  A second producer of clip[]: a duplicate record is clipped from end to end, so every
// consumer of the mate join's clip (the packers' plane kernels, tally_stream_kernel, open_walk) leaves it out without knowing why.
// Launched behind the mate join, inside its profiling bracket, only when the setting is on (mate_join.hip: tcmi_mate_join_enqueue);
// the join has left every pair's records each other's index in mate_idx[] and written clip[] for every record.
//
// The table: open addressing in global memory, one slot per KEY: {32-bit tag of the key's hash << 32 | the claiming leader + 1}, 0:
// empty; tcmi_mate_slots(rec_cap) of them, at least twice the records, so it cannot fill.  Behind it best[slot], the largest
// tcmi_dup_rank of the key's templates; the four counters; count[slot], the key's templates.  One hipMemsetAsync zeroes all of it.
//   dup_ends_kernel    one lane per record (stream_count.h's each_record): an examined record's end and score — one walk over its CIGAR
//                      for u5, QUAL four bytes at a time through ld_u32 (l_seq bytes a record: the feature's memory traffic) —
//                      and its span into ends[i] (sixteen bytes); meta 0 for every other record below the record count.
//   dup_build_kernel   leaders only (a fragment; a pair's record of the lower index).  The key from ends[i] and ends[mate], its slot by
//                      linear probing from the hash's: an empty slot is claimed by one 64-bit atomicCAS; an entry with the key's tag is
//                      compared by the full key, which is recomputed from ends[] of the claimant and its mate (the launch before wrote
//                      them).  A lane's work does not grow with its key's templates: there is no chain over members, the probe ends at
//                      the key's one slot.  The lanes of a wavefront that hold one slot are reduced among themselves (wave_join): one
//                      atomicMax on best[slot] and one atomicAdd on count[slot] per distinct slot per wavefront.  slot_of[leader].
//   dup_mark_kernel    leaders only, a launch of its own — the only ordering: nothing spins, no lane waits for another workgroup.  A
//                      leader that best[slot_of[i]] does not name is a duplicate: dup[] = 1 and clip[] = max(clip[], span) for itself
//                      and its mate (the leader is the only writer of its mate's entries); dup[] = 0 otherwise: written for every
//                      record below the record count.  The four counters: summed per lane over its records, then by shuffles and
//                      through LDS: one atomic per counter per WORKGROUP; a key with two templates or more is counted once, by its winner.
// Which record is kept (kept_span), the unaligned loads (ld_u32), the wave join: pack_device.h.  The stream is only read.
#include "stream_count.h"
#include "dedup_rule.h"

namespace {

constexpr int BLOCK = SC_BLOCK;
using MjArgs = tcmi_mate_job;
using DdArgs = tcmi_dedup_job;
static_assert(sizeof(tcmi_dup_end) == TCMI_DUP_END_BYTES, "pack_caps.h sizes ends[] by it");

struct DupTable {
    unsigned long long *slot, *best, *cnt;
    uint32_t *count;
};
__device__ inline DupTable table_of(const DdArgs &d, uint32_t slot_mask)
{
    const size_t slots = (size_t)slot_mask + 1;
    DupTable t;
    t.slot = d.table; t.best = d.table + slots; t.cnt = d.table + 2 * slots;
    t.count = reinterpret_cast<uint32_t *>(d.table + 2 * slots + 4);
    return t;
}

// the score of QUAL [l_seq]: whole dwords, then the tail as the last four bytes of QUAL shifted down — no load ends behind QUAL, which
// ends inside the record; a QUAL shorter than a dword byte by byte through aligned loads
__device__ inline uint32_t score_of(const uint8_t *qual, int32_t l_seq)
{
    uint32_t s = 0;
    int32_t k = 0;
    for (; k + 4 <= l_seq; k += 4) s = tcmi_dup_score_add(s, tcmi_dup_score_word(ld_u32(qual + k)));
    const int rest = (int)(l_seq - k);
    if (rest > 0) {
        if (l_seq >= 4) s = tcmi_dup_score_add(s, tcmi_dup_score_word(ld_u32(qual + l_seq - 4) >> (8 * (4 - rest)), rest));
        else for (; k < l_seq; ++k) s = tcmi_dup_score_add(s, tcmi_dup_score_word(byte_at(qual + k), 1));
    }
    return s;
}

__global__ __launch_bounds__(BLOCK) void dup_ends_kernel(MjArgs a, DdArgs d)
{
    const int64_t n = record_count(a);
    each_record(n, [&](int64_t i) {
        if (i >= n) return;
        tcmi_dup_end e = {0, 0u, 0u, 0u};
        // (nothing of a record that claims to lie or end behind the stream is followed: as the join's open_mate)
        const uint64_t roff = a.src.rec_off[i];
        if (roff + 36ull <= a.stream_len && roff + 4ull + ld_u32(a.src.stream + roff) <= a.stream_len) {
            ReadView v;
            int64_t p, q;
            if (kept_span(a.src, i, v, p, q) && tcmi_dup_examined(v.flag)) {
                const bool rev = (v.flag & 0x10u) != 0u;
                const uint8_t *cg = v.cigar;
                const int64_t u5 = tcmi_dup_u5(v.pos, rev, v.n_cigar, [cg](uint32_t k) { return ld_u32(cg + 4 * (size_t)k); });
                e = tcmi_dup_end_make(v.tid, u5, rev, score_of(v.seq + ((size_t)v.l_seq + 1) / 2, v.l_seq), (uint32_t)(q - p + 1));
            }
        }
        d.ends[i] = e;
    });
}

// the key and the score of the template that record i leads (its mate: m - 1, m == 0: a fragment)
__device__ inline tcmi_dup_key template_of(const DdArgs &d, const tcmi_dup_end &e, uint32_t m, uint32_t &score)
{
    if (!m) { score = e.score; return tcmi_dup_key_fragment(e); }
    const tcmi_dup_end o = d.ends[m - 1u];
    score = tcmi_dup_score_add(e.score, o.score);
    return tcmi_dup_key_pair(e, o);
}

__global__ __launch_bounds__(BLOCK) void dup_build_kernel(MjArgs a, DdArgs d, uint32_t slot_mask)
{
    const int64_t n = record_count(a);
    const int lane = threadIdx.x & 63;
    const DupTable t = table_of(d, slot_mask);
    each_record(n, [&](int64_t i) {
        bool todo = false;
        uint32_t slot = 0;
        unsigned long long rank = 0;
        if (i < n) {
            const tcmi_dup_end e = d.ends[i];
            const uint32_t m = tcmi_dup_end_examined(e) ? a.mate_idx[i] : 0u;
            if (tcmi_dup_end_examined(e) && (m == 0u || (int64_t)m - 1 > i)) {
                uint32_t score;
                const tcmi_dup_key key = template_of(d, e, m, score);
                const uint64_t h = tcmi_dup_hash(key);
                const uint32_t tag = tcmi_mate_tag(h);
                const unsigned long long entry = ((unsigned long long)tag << 32) | (unsigned long long)(i + 1);
                slot = (uint32_t)h & slot_mask;
                // (the table has twice the records' slots and every leader claims at most one: an empty one comes)
                for (uint32_t tries = 0; tries <= slot_mask; ++tries) {
                    // (a plain look first: a million templates of one key would otherwise queue a million CAS on one address — 12 ms
                    //  measured; once the slot is claimed everybody reads it.  A stale 0 only sends the lane to the CAS, which decides)
                    unsigned long long old = __atomic_load_n(&t.slot[slot], __ATOMIC_RELAXED);
                    if (old == 0ull) old = atomicCAS(&t.slot[slot], 0ull, entry);
                    if (old == 0ull) break;
                    if ((uint32_t)(old >> 32) == tag) {
                        const int64_t c = (int64_t)(uint32_t)old - 1;       // (a leader below n: the build puts nothing else there)
                        if (c >= 0 && c < n) {
                            uint32_t cs;
                            const tcmi_dup_end ce = d.ends[c];
                            if (tcmi_dup_key_same(key, template_of(d, ce, a.mate_idx[c], cs))) break;
                        }
                    }
                    slot = (slot + 1u) & slot_mask;
                }
                d.slot_of[i] = slot;
                rank = tcmi_dup_rank(score, (uint32_t)i);
                todo = true;
            }
        }
        // one atomic pair per distinct slot of the wavefront: an amplicon-style file puts all 64 lanes on one
        wave_join(todo, slot, [&](int lead, uint32_t ls, bool same) {
            const uint32_t c = (uint32_t)__popcll(__ballot(same));
            unsigned long long r = same ? rank : 0ull;
            if (c > 1u) {                                       // (uniform over the wavefront)
#pragma unroll
                for (int s = 32; s >= 1; s >>= 1) {
                    const unsigned long long o = (unsigned long long)__shfl_xor((long long)r, s, 64);
                    r = o > r ? o : r;
                }
            }
            if (lane == lead) {
                atomicMax(&t.best[ls], r);
                atomicAdd(&t.count[ls], c);
            }
        });
    });
}

// a duplicate record: clipped from end to end (its span lies in ends[]: the stream is not opened again)
__device__ inline void clip_whole(const MjArgs &a, int64_t j, uint32_t span)
{
    if (a.clip[j] < span) a.clip[j] = span;
}

__global__ __launch_bounds__(BLOCK) void dup_mark_kernel(MjArgs a, DdArgs d, uint32_t slot_mask)
{
    const int64_t n = record_count(a);
    const int lane = threadIdx.x & 63;
    const DupTable t = table_of(d, slot_mask);
    // the four counters — templates, duplicate templates, duplicate records, duplicate sets — of this lane over all its records
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    each_record(n, [&](int64_t i) {
        if (i >= n) return;
        const tcmi_dup_end e = d.ends[i];
        const bool examined = tcmi_dup_end_examined(e);
        const uint32_t m = examined ? a.mate_idx[i] : 0u;
        if (m != 0u && (int64_t)m - 1 < i) return;              // (a pair's second record: its leader writes for it)
        bool is_dup = false;
        if (examined) {
            const uint32_t slot = d.slot_of[i];
            ++c0;
            if (tcmi_dup_rank_leader(t.best[slot]) != (uint32_t)i) { is_dup = true; ++c1; c2 += m ? 2u : 1u; }
            else if (t.count[slot] >= 2u) ++c3;
        }
        d.dup[i] = is_dup ? 1 : 0;
        if (m) d.dup[m - 1u] = is_dup ? 1 : 0;
        if (is_dup) {
            clip_whole(a, i, e.span);
            if (m) clip_whole(a, (int64_t)m - 1, d.ends[m - 1u].span);
        }
    });
    // ONE atomic per counter per workgroup, behind its last record: an atomic per wavefront per trip put 47 000 of them on four
    // addresses for a million records, and atomics on one address queue (the lanes by shuffles, the four wavefronts through LDS)
    __shared__ uint32_t wg[4];
    if (threadIdx.x < 4) wg[threadIdx.x] = 0u;
    __syncthreads();
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        c0 += (uint32_t)__shfl_xor((int)c0, s, 64); c1 += (uint32_t)__shfl_xor((int)c1, s, 64);
        c2 += (uint32_t)__shfl_xor((int)c2, s, 64); c3 += (uint32_t)__shfl_xor((int)c3, s, 64);
    }
    if (lane == 0) {
        if (c0) atomicAdd(&wg[0], c0);
        if (c1) atomicAdd(&wg[1], c1);
        if (c2) atomicAdd(&wg[2], c2);
        if (c3) atomicAdd(&wg[3], c3);
    }
    __syncthreads();
    if (threadIdx.x < 4 && wg[threadIdx.x]) atomicAdd(&t.cnt[threadIdx.x], (unsigned long long)wg[threadIdx.x]);
}

} // namespace

// (the caller holds the join's profiling bracket open and asks hipGetLastError behind it)
void tcmi_dedup_launch(tcmi_ctx *ctx, const tcmi_mate_job &job, const tcmi_dedup_job &dedup, unsigned grid, uint32_t slot_mask)
{
    (void)hipMemsetAsync(dedup.table, 0, tcmi_dup_table_bytes(job.rec_cap), ctx->stream);
    hipLaunchKernelGGL(dup_ends_kernel, dim3(grid), dim3(BLOCK), 0, ctx->stream, job, dedup);
    hipLaunchKernelGGL(dup_build_kernel, dim3(grid), dim3(BLOCK), 0, ctx->stream, job, dedup, slot_mask);
    hipLaunchKernelGGL(dup_mark_kernel, dim3(grid), dim3(BLOCK), 0, ctx->stream, job, dedup, slot_mask);
}

// dup[] of a read set built under the rule, while its stream (and dup[] beside it) is resident on this context
extern "C" int tcmi_readset_duplicates(tcmi_ctx *ctx, const tcmi_readset *rs, uint8_t *out, int64_t cap, int64_t *n)
{
    if (!ctx || !rs || !n || cap < 0 || (cap > 0 && !out)) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    *n = 0;
    if (!rs->rules.dedup)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "tcmi_readset_duplicates: the read set was not built under the duplicate rule (--dedup)");
    if (rs->n_reads == 0 || (!rs->d_dup && rs->n_piled == 0)) return TCMI_OK;    // (a file without a record never reached a packer)
    if (rs->device != ctx->device || tcmi_stream_gone(ctx, rs) || !rs->d_dup)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "tcmi_readset_duplicates: the read set's decoded stream (--dedup keeps its verdicts beside it) is no longer "
                         "resident on this context (another upload happened on it)");
    if (cap < rs->n_reads) return tcmi_fail(ctx, TCMI_E_ARG, "tcmi_readset_duplicates: room for %lld records, the read set holds %lld", (long long)cap, (long long)rs->n_reads);
    TCMI_HIP(ctx, hipSetDevice(ctx->device));
    TCMI_HIP(ctx, hipMemcpyAsync(out, rs->d_dup, (size_t)rs->n_reads, hipMemcpyDeviceToHost, ctx->stream));
    TCMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n = rs->n_reads;
    return TCMI_OK;
}
