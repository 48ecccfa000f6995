// link_counts.hip — --variant-links on gfx950: for pairs of nearby queried columns, how many kept records carry which token class at
// the first column AND which at the second, counted in the inflated BAM stream a device-decoded read set left in the context's arena
// (include/tcmi.h: tcmi_readset_link_counts).  The count matrix forgets which read a token came from: only the records know whether
// two alleles sit on the same molecule.  RECORDS are counted, not templates: the two mates of a pair are two records, each with its
// own columns, as in tcmi_readset_amplicon_reads.
//
// Here: the kernel and the entry that checks and narrows the columns and unpacks the sums.  The per-column walk and the token rule
// (open_walk, token_at, first_at_or_above), shared with strand_counts.hip: stream_walk.h; which record is kept and where it lies on the
// axis (kept_span): pack_device.h; the residency refusals, the scratch, the launch shape, the download and the sub-ranges:
// stream_count.h.
//
// One launch, one lane per record, 256-lane workgroups that stride over the records: the grid is min(ceil(records / 256), compute
// units x 8).  LDS: the columns and the [n * K][49] counters of up to TCMI_LINKS_LDS pairs, 16 000 bytes (ten workgroups a CU by LDS).
//   per record   kept_span for [p, q], the primer table's head_end / tail_start when the set has one, then a binary search for the
//                first queried column >= p.  A record without a queried column in [p, q] is done here: at every column its class is 0,
//                and [0][0] is not counted.
//   the walk     the others visit their queried columns in ascending order with the one incremental walk of the CIGAR.  The class of
//                the token at a column: 0 nothing (masked, below the floor), 1..4 a matched base on plane A, T, C, G, 5 a deleted
//                column that counts X, 6 a token that counts coverage and none of those planes.  The I mark takes no part.
//   the pairs    the lane keeps the classes at its last K visited columns in one register, four bits each.  At column index ci with
//                class t, for d = 1..K with ci - d >= 0: prev is the d-th nibble, and when prev | t is not zero one count goes to pair
//                (ci - d) * K + d - 1 at [prev][t].  Columns in front of the first visited one have class 0 (the register starts at
//                zero).  Behind the last queried column <= q the lane goes on over up to K more columns with t = 0 (while ci < n and
//                the register is not zero): the pairs whose second column lies beyond the record get their [x][0].
//   counters     a sorted BAM puts a wavefront's 64 records on the same few pairs and most of them on one class pair: per round and d
//                the lanes with the same (pair, prev, t) are joined (pack_device.h's wave_join) and the group's leader adds the
//                popcount — through the workgroup's counter frame (stream_count.h's CountFrame: LDS while n * K <= TCMI_LINKS_LDS,
//                else memory).
// The sums are integers: their order does not matter and every run gives the same numbers.  The stream is only read.
#include <vector>

#include "stream_count.h"
#include "stream_walk.h"

namespace {

constexpr int BLOCK = SC_BLOCK;
constexpr int LDS_P = TCMI_LINKS_LDS;   // pairs (n * K) whose counters are staged; then n <= LDS_P as well
constexpr int NC = 7;                   // token classes
constexpr int NJ = NC * NC;             // counters per pair
constexpr int MAX_K = 7;
constexpr int64_t MAX_PAIRS = 1 << 17;
static_assert(LDS_P * (NJ + 1) * 4 <= 16384, "the staged columns and counters stay at or under 16 KiB");
static_assert(sizeof(tcmi_link_counts) == 208, "tcmi_link_counts is fifty-two int32");

struct LcArgs {
    PackSrc src;                        // the resident stream, the read set's filter, floor and layout
    tcmi_primer_tab pt;                 // the primer table the read set was built under (none: zeros)
    const int32_t *cols;                // [n] ascending
    int32_t *counts;                    // [n * K][49]
    int32_t n, K;
};

__global__ __launch_bounds__(BLOCK) void link_counts_kernel(LcArgs a)
{
    __shared__ int32_t s_cols[LDS_P];
    __shared__ uint32_t s_cnt[NJ * LDS_P];
    const int tid = threadIdx.x, lane = tid & 63;
    const int K = a.K;
    const int n_cnt = NJ * a.n * K;                         // (n * K <= 2^17: below 2^23)
    const CountFrame<int32_t> cnt = {s_cnt, a.counts, a.n * K <= LDS_P};
    if (cnt.staged) {
        for (int k = tid; k < a.n; k += BLOCK) s_cols[k] = a.cols[k];
        cnt.zero(n_cnt);
        __syncthreads();
    }
    const int32_t *cols = cnt.staged ? s_cols : a.cols;
    const uint32_t Q = a.src.min_bq;
    const uint32_t keep = (1u << (4 * K)) - 1u;             // the K <= 7 nibbles the register holds
    each_record(a.src.n, [&](int64_t i) {
        Walk w;
        int32_t ci = 0;
        bool have = i < a.src.n && open_walk(a.src, a.pt, i, w);
        if (have) {
            ci = first_at_or_above(cols, a.n, w.x);
            have = ci < a.n && cols[ci] <= w.q;
        }
        uint32_t hist = 0u;                                 // nibble d - 1: the class at column index ci - d
        int tail = 0;                                       // columns behind the record still to run
        bool live = have;
        while (__ballot(live)) {                            // one round per column of the wavefront's busiest record
            const uint32_t t = have ? class_of(token_at(w, cols[ci], Q)) : 0u;
            for (int d = 1; d <= K; ++d) {                  // (K is uniform)
                const uint32_t prev = (hist >> (4 * (d - 1))) & 15u;
                const uint32_t key = (uint32_t)(((ci - d) * K + d - 1) * NJ) + prev * NC + t;     // (only read by a lane that counts)
                // one pass per distinct (pair, prev, t)
                wave_join(live && ci >= d && (prev | t) != 0u, key, [&](int lead, uint32_t lk, bool same) {
                    const unsigned long long ms = __ballot(same);
                    if (lane == lead) cnt.add(lk, __popcll(ms));
                });
            }
            if (live) {
                hist = ((hist << 4) | t) & keep;
                ++ci;
                if (have) {
                    have = ci < a.n && cols[ci] <= w.q;
                    if (!have) tail = K;
                } else --tail;
                live = have || (tail > 0 && ci < a.n && hist != 0u);
            }
        }
    });
    cnt.flush(n_cnt);
}

} // namespace

extern "C" int tcmi_readset_link_counts(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t n, const int64_t *cols, int32_t k, tcmi_link_counts *records)
{
    if (!ctx || !rs) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    if (k < 1 || k > MAX_K) return tcmi_fail(ctx, TCMI_E_ARG, "link counts: %d neighbours: 1..7 are allowed", (int)k);
    if (n < 1 || n * k > MAX_PAIRS)
        return tcmi_fail(ctx, TCMI_E_ARG, "link counts: %lld columns with %d neighbours each: 1..131072 pairs are allowed", (long long)n, (int)k);
    if (!cols || !records) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    const size_t n_pairs = (size_t)n * (size_t)k;
    std::vector<int32_t> c32;
    std::vector<int64_t> sums;
    if (const int rc = tcmi_count_columns(ctx, "link counts", n, cols, c32)) return rc;
    try {
        sums.assign((size_t)NJ * n_pairs, 0);
    } catch (...) {                                         // (no exception may cross the C ABI)
        return tcmi_fail(ctx, TCMI_E_NOMEM, "link counts: no host memory for %lld columns", (long long)n);
    }
    // the columns (int32) in, [n * K][49] int32 counters out; the primer table is the one each part was built under
    const int rc = tcmi_stream_count_parts<int32_t>(
        ctx, rs, "link counts", TCMI_K_LINK_COUNTS, c32.data(), c32.size() * 4, sums,
        [n, k](tcmi_ctx *cx, const tcmi_readset *part, const PackSrc &src, const char *d_in, int32_t *d_cnt, unsigned grid) {
            const LcArgs a = {src, tcmi_mask_args(part), reinterpret_cast<const int32_t *>(d_in), d_cnt, (int32_t)n, k};
            hipLaunchKernelGGL(link_counts_kernel, dim3(grid), dim3(BLOCK), 0, cx->stream, a);
        });
    if (rc) return rc;
    for (int64_t i = 0; i < n; ++i) {
        for (int d = 1; d <= k; ++d) {
            const size_t pr = (size_t)i * (size_t)k + (size_t)(d - 1);
            tcmi_link_counts &r = records[pr];
            for (int x = 0; x < NC; ++x)
                for (int y = 0; y < NC; ++y) r.j[x][y] = (int32_t)sums[pr * NJ + (size_t)(x * NC + y)];
            r.a = (int32_t)cols[i];
            r.b = i + d < n ? (int32_t)cols[i + d] : -1;    // (no such pair: the kernel never counts there)
            r.reserved = 0;
        }
    }
    return TCMI_OK;
}
