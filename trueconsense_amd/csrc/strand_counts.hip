// strand_counts.hip — --variant-strand on gfx950: the count matrix's seven planes at given columns, split by the strand of the record
// (FLAG 0x10), counted in the inflated BAM stream a device-decoded read set left in the context's arena (include/tcmi.h:
// tcmi_readset_strand_counts).  The matrix sums the strands and the packed set does not keep the flag: only the records have it.
//
// Here: the kernel and the entry that checks and narrows the columns and unpacks the sums.  The per-column walk and the token rule
// (open_walk, token_at, first_at_or_above), shared with link_counts.hip: stream_walk.h; which record is kept and where it lies on the
// axis (kept_span), the primer table's lookup (seg_find) and the leaves of the token rule (base_plane, qual_at): pack_device.h; the
// residency refusals, the scratch, the launch shape, the download and the sub-ranges: stream_count.h.
//
// One launch, one lane per record, 256-lane workgroups that stride over the records: the grid is min(ceil(records / 256), compute
// units x 8).  LDS: the columns and [n][14] counters of up to TCMI_STRAND_LDS columns, 15 KiB.
//   per record   kept_span for [p, q], the primer table's head_end / tail_start when the set has one, then a binary search for the
//                first queried column >= p.  A record without a queried column in [p, q] — nearly every record of a sparse query —
//                is done here.
//   the walk     the others visit their queried columns in ascending order with ONE incremental walk of the CIGAR (the op index, the
//                op's first column and query index are kept between columns).  Per column the token rule of tally_stream_kernel
//                (tally.hip), restated for one column: a matched base counts coverage and its letter; a D column coverage and X,
//                unless it is the deletion's last column with an insertion behind it; an N column coverage; the I mark goes to the
//                last column of an op in front of an insertion; a token below the floor (a matched base by its own QUAL byte, a D / N
//                token by that of the query index at which its op starts, a query index at or beyond l_seq quality 0) or on a column
//                outside [head_end, tail_start) adds nothing at all, the I mark included.
//   counters     a sorted BAM puts a wavefront's 64 records on the same few columns: per round (each lane's next column) the lanes
//                that hit the same (column, strand) are joined (pack_device.h's wave_join), and per plane the group's leader adds
//                the popcount — through the workgroup's counter frame (stream_count.h's CountFrame: LDS while the columns are
//                staged, else memory).
// The sums are integers: their order does not matter and every run gives the same numbers.  The stream is only read.
#include <vector>

#include "stream_count.h"
#include "stream_walk.h"

namespace {

constexpr int BLOCK = SC_BLOCK;
constexpr int LDS_N = TCMI_STRAND_LDS;
constexpr int NK = 14;                  // counters per column: fwd[7] | rev[7] in plane order
constexpr int64_t MAX_N = 1 << 20;

struct ScArgs {
    PackSrc src;                        // the resident stream, the read set's filter, floor and layout
    tcmi_primer_tab pt;                 // the primer table the read set was built under (none: zeros)
    const int32_t *cols;                // [n] ascending
    int32_t *counts;                    // [n][14]
    int32_t n;
};

__global__ __launch_bounds__(BLOCK) void strand_counts_kernel(ScArgs a)
{
    __shared__ int32_t s_cols[LDS_N];
    __shared__ uint32_t s_cnt[NK * LDS_N];
    const int tid = threadIdx.x, lane = tid & 63;
    const CountFrame<int32_t> cnt = {s_cnt, a.counts, a.n <= LDS_N};
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
        bool have = i < a.src.n && open_walk(a.src, a.pt, i, w);
        if (have) {
            ci = first_at_or_above(cols, a.n, w.x);
            have = ci < a.n && cols[ci] <= w.q;
        }
        const uint32_t strand = have && (w.v.flag & 0x10u) ? 1u : 0u;
        while (__ballot(have)) {                            // one round per queried column of the wavefront's busiest record
            const uint32_t bits = have ? token_at(w, cols[ci], Q) : 0u;
            // one pass per distinct (column, strand) the round's tokens hit
            wave_join(bits != 0u, 2u * (uint32_t)ci + strand, [&](int lead, uint32_t lk, bool same) {
#pragma unroll
                for (int pl = 0; pl < TCMI_NCOL; ++pl) {
                    const unsigned long long mp = __ballot(same && ((bits >> pl) & 1u));
                    if (lane == lead && mp) cnt.add((int64_t)(NK / 2) * lk + pl, __popcll(mp));
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

extern "C" int tcmi_readset_strand_counts(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t n, const int64_t *cols, tcmi_strand_counts *records)
{
    if (!ctx || !rs) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    if (n < 1 || n > MAX_N) return tcmi_fail(ctx, TCMI_E_ARG, "strand counts: %lld columns: 1..1048576 are allowed", (long long)n);
    if (!cols || !records) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    std::vector<int32_t> c32;
    std::vector<int64_t> sums;
    if (const int rc = tcmi_count_columns(ctx, "strand counts", n, cols, c32)) return rc;
    try {
        sums.assign((size_t)NK * (size_t)n, 0);
    } catch (...) {                                         // (no exception may cross the C ABI)
        return tcmi_fail(ctx, TCMI_E_NOMEM, "strand counts: no host memory for %lld columns", (long long)n);
    }
    // the columns (int32) in, [n][14] int32 counters out; the primer table is the one each part was built under
    const int rc = tcmi_stream_count_parts<int32_t>(
        ctx, rs, "strand counts", TCMI_K_STRAND_COUNTS, c32.data(), c32.size() * 4, sums,
        [n](tcmi_ctx *cx, const tcmi_readset *part, const PackSrc &src, const char *d_in, int32_t *d_cnt, unsigned grid) {
            const ScArgs a = {src, tcmi_mask_args(part), reinterpret_cast<const int32_t *>(d_in), d_cnt, (int32_t)n};
            hipLaunchKernelGGL(strand_counts_kernel, dim3(grid), dim3(BLOCK), 0, cx->stream, a);
        });
    if (rc) return rc;
    for (int64_t i = 0; i < n; ++i) {
        for (int k = 0; k < TCMI_NCOL; ++k) {
            records[i].fwd[k] = (int32_t)sums[(size_t)(NK * i + k)];
            records[i].rev[k] = (int32_t)sums[(size_t)(NK * i + TCMI_NCOL + k)];
        }
        records[i].pos = (int32_t)cols[i];
        records[i].reserved = 0;
    }
    return TCMI_OK;
}
