// evidence_counts.hip — --variant-evidence on gfx950: per queried column and plane of the count matrix the number of tokens and the sums
// of their base quality, of their records' MAPQ and of their distance to the nearer end of the read's aligned part, counted in the
// inflated BAM stream a device-decoded read set left in the context's arena (include/tcmi.h: tcmi_readset_evidence_counts).  The matrix
// and the packed set keep neither QUAL per token, nor MAPQ, nor the query index: only the records have them.
//
// Here: the kernel and the entry that checks and narrows the columns and unpacks the sums.  The per-column walk and the token rule
// (open_walk, token_at, first_at_or_above): stream_walk.h; which record is kept (kept_span), the leaves of the token rule (qual_at) and
// the wave join: pack_device.h; the residency refusals, the scratch, the launch shape, the download, the sub-ranges and the counter
// frame: stream_count.h; when the frame may be staged: evidence_rule.h.
//
// One launch, strand_counts.hip's shape: one lane per record, 256-lane workgroups that stride over the records, the grid
// min(ceil(records / 256), compute units x 8).  LDS: the columns and [n][28] uint32 counters of up to TCMI_EVIDENCE_LDS columns, 14.5 KiB.
//   per record   as in strand_counts.hip: kept_span, the primer table's bounds, a binary search for the first queried column; a record
//                with a queried column reads its CIGAR once more for [a0, a1), the aligned part of its query.
//   the walk     one incremental walk over the queried columns, token_at per column: a token counts here exactly when it counts in the
//                matrix.  Behind token_at the walk stands on the op that holds the column, which gives the query index qi the floor
//                tested: the token's quality is qual_at(v, qi) (read whatever the floor), its distance min(255, max(0, min(qi - a0,
//                a1 - 1 - qi))).
//   counters     (column, plane) -> n | qual | mapq | dist, four neighbours.  A sorted BAM puts a wavefront's 64 records on the same
//                few columns: per round the lanes that hit the same column are joined (wave_join), and per plane the group has at all
//                the leader adds the popcount and the three sums — the three bytes travel in 16-bit fields of one 64-bit word (a
//                field holds at most 64 x 255) through a butterfly of __shfl_xor, lanes outside the group or the plane giving 0.
//                Memory counters are 64-bit; an LDS counter holds at most 255 x the records its workgroup visits, which the host
//                bounds before it lets the kernel stage (tcmi_evidence_lds_ok).
// The sums are integers: their order does not matter and every run gives the same numbers.  The stream is only read.
#include <vector>

#include "evidence_rule.h"
#include "stream_count.h"
#include "stream_walk.h"

namespace {

constexpr int BLOCK = SC_BLOCK;
constexpr int LDS_N = TCMI_EVIDENCE_LDS;
constexpr int NK = 28;                  // counters per column: per plane n, qual, mapq, dist
constexpr int64_t MAX_N = 1 << 20;
typedef unsigned long long Sum;         // a memory counter

struct EvArgs {
    PackSrc src;                        // the resident stream, the read set's filter, floor and layout
    tcmi_primer_tab pt;                 // the primer table the read set was built under (none: zeros)
    const int32_t *cols;                // [n] ascending
    Sum *counts;                        // [n][28]
    int32_t n;
    int32_t staged;                     // count in LDS (tcmi_evidence_lds_ok)
};

// [a0, a1): the aligned part of the record's query, from the CIGAR alone
__device__ inline void aligned_part(const ReadView &v, int64_t &a0, int64_t &a1)
{
    int64_t head = 0, tail = 0, total = 0;
    bool inside = false;                                    // behind the first op that is neither S nor H
    for (uint32_t k = 0; k < v.n_cigar; ++k) {
        const uint32_t cw = ld_u32(v.cigar + 4 * (size_t)k), op = cw & 0xFu;
        const int64_t len = cw >> 4;
        if (consumes_query(op)) total += len;
        if (op == 4) {
            if (inside) tail += len;
            else head += len;
        } else if (op != 5) {
            inside = true;
            tail = 0;
        }
    }
    a0 = head;
    a1 = total - tail;
}

__global__ __launch_bounds__(BLOCK) void evidence_counts_kernel(EvArgs a)
{
    __shared__ int32_t s_cols[LDS_N];
    __shared__ uint32_t s_cnt[NK * LDS_N];
    const int tid = threadIdx.x, lane = tid & 63;
    const CountFrame<Sum> cnt = {s_cnt, a.counts, a.staged != 0};
    const int n_cnt = NK * a.n;
    if (cnt.staged) {
        for (int k = tid; k < a.n; k += BLOCK) s_cols[k] = a.cols[k];
        cnt.zero(n_cnt);
        __syncthreads();
    }
    const int32_t *cols = cnt.staged ? s_cols : a.cols;
    const uint32_t Q = a.src.min_bq;
    each_record(a.src.n, [&](int64_t i) {
        Walk w;
        int32_t ci = 0;
        int64_t a0 = 0, a1 = 0;
        bool have = i < a.src.n && open_walk(a.src, a.pt, i, w);
        if (have) {
            ci = first_at_or_above(cols, a.n, w.x);
            have = ci < a.n && cols[ci] <= w.q;
        }
        if (have) aligned_part(w.v, a0, a1);
        while (__ballot(have)) {                            // one round per queried column of the wavefront's busiest record
            uint32_t bits = 0u;
            Sum word = 0;                                   // qual | mapq << 16 | dist << 32
            if (have) {
                const int32_t c = cols[ci];
                bits = token_at(w, c, Q);
                if (bits) {                                 // (the walk stands on the op that holds c)
                    const uint32_t op = ld_u32(w.v.cigar + 4 * (size_t)w.k) & 0xFu;
                    const int32_t qi = is_match(op) ? w.y + (c - w.x) : w.y;
                    const int64_t d = min((int64_t)255, max((int64_t)0, min(qi - a0, a1 - 1 - qi)));
                    word = (Sum)qual_at(w.v, qi) | (Sum)w.v.mapq << 16 | (Sum)(uint32_t)d << 32;
                }
            }
            // one pass per distinct column the round's tokens hit
            wave_join(bits != 0u, (uint32_t)ci, [&](int lead, uint32_t lk, bool same) {
#pragma unroll
                for (int pl = 0; pl < TCMI_NCOL; ++pl) {
                    const bool mine = same && ((bits >> pl) & 1u);
                    const unsigned long long mp = __ballot(mine);
                    if (!mp) continue;                      // (uniform: no lane of the group has this plane)
                    Sum s = mine ? word : 0;
#pragma unroll
                    for (int step = 32; step > 0; step >>= 1) s += __shfl_xor(s, step, 64);
                    if (lane == lead) {
                        const int64_t k = (int64_t)NK * lk + 4 * pl;
                        cnt.add(k, __popcll(mp));
                        cnt.add(k + 1, (int)(s & 0xFFFFu));
                        cnt.add(k + 2, (int)((s >> 16) & 0xFFFFu));
                        cnt.add(k + 3, (int)((s >> 32) & 0xFFFFu));
                    }
                }
            });
            if (have) {
                ++ci;
                have = ci < a.n && cols[ci] <= w.q;
            }
        }
    });
    cnt.flush(n_cnt);
}

} // namespace

extern "C" int tcmi_readset_evidence_counts(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t n, const int64_t *cols, tcmi_evidence_counts *records)
{
    if (!ctx || !rs) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    if (n < 1 || n > MAX_N) return tcmi_fail(ctx, TCMI_E_ARG, "evidence counts: %lld columns: 1..1048576 are allowed", (long long)n);
    if (!cols || !records) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    std::vector<int32_t> c32;
    std::vector<int64_t> sums;
    if (const int rc = tcmi_count_columns(ctx, "evidence counts", n, cols, c32)) return rc;
    try {
        sums.assign((size_t)NK * (size_t)n, 0);
    } catch (...) {                                         // (no exception may cross the C ABI)
        return tcmi_fail(ctx, TCMI_E_NOMEM, "evidence counts: no host memory for %lld columns", (long long)n);
    }
    // the columns (int32) in, [n][28] 64-bit counters out; the primer table is the one each part was built under, the staging is
    // decided per part from its own records and grid
    const int rc = tcmi_stream_count_parts<Sum>(
        ctx, rs, "evidence counts", TCMI_K_EVIDENCE_COUNTS, c32.data(), c32.size() * 4, sums,
        [n](tcmi_ctx *cx, const tcmi_readset *part, const PackSrc &src, const char *d_in, Sum *d_cnt, unsigned grid) {
            const EvArgs a = {src, tcmi_mask_args(part), reinterpret_cast<const int32_t *>(d_in), d_cnt, (int32_t)n,
                              tcmi_evidence_lds_ok(n, src.n, grid, BLOCK) ? 1 : 0};
            hipLaunchKernelGGL(evidence_counts_kernel, dim3(grid), dim3(BLOCK), 0, cx->stream, a);
        });
    if (rc) return rc;
    for (int64_t i = 0; i < n; ++i) {
        for (int k = 0; k < TCMI_NCOL; ++k) {
            const int64_t *s = &sums[(size_t)(NK * i + 4 * k)];
            records[i].n[k] = (int32_t)s[0];
            records[i].qual[k] = s[1];
            records[i].mapq[k] = s[2];
            records[i].dist[k] = s[3];
        }
        records[i].pos = (int32_t)cols[i];
    }
    return TCMI_OK;
}
