// codon_counts.hip — --codon-table on gfx950: for queried codons (three adjacent columns of the count matrix's axis), how many kept records
// carry which token class at the first column AND at the second AND at the third, counted in the inflated BAM stream a device-decoded
// read set left in the context's arena (include/tcmi.h: tcmi_readset_codon_counts).  The count matrix forgets which read a token came
// from: only the records know the triplet a molecule carries, so only they can say what two changes inside one codon mean for the
// protein.  RECORDS are counted, not templates, as in link_counts.hip.
//
// Here: the kernel and the entry that checks and narrows the codons and unpacks the sums.  The per-column walk, the token rule and the
// classes (open_walk, token_at, first_at_or_above, class_of): stream_walk.h; which record is kept and where it lies on the axis
// (kept_span): pack_device.h; the residency refusals, the scratch, the launch shape, the download and the sub-ranges: stream_count.h.
//
// One launch, one lane per record, 256-lane workgroups that stride over the records: the grid is min(ceil(records / 256), compute
// units x 8).  LDS: the first columns and the [344] counters of up to TCMI_CODONS_LDS codons, 15 180 bytes.
//   per record   open_walk for [p, q] and the masks, then a binary search for the first codon with c0 + 2 >= p.  A record without a
//                codon that starts at or below q is done here: at every column its class is 0, and [0][0][0] is not counted.
//   the walk     the others visit their codons in ascending order, one round of the wavefront per codon, with the one incremental walk
//                of the CIGAR.  Codons may overlap (c0 one or two above the last one's): the lane keeps the nibbles — class, and the I
//                mark as bit 3 — of the last three columns below `top`, the column behind the highest one it has settled, in one
//                register, and asks token_at only for a column at or above top.  top starts at p with a register of zeros: the columns
//                below p read 0.  A column beyond q is 0 without a call.  Across a gap the register is shifted by the columns skipped
//                (three or more: cleared); they are never read again, since the codons ascend.
//   counters     per round the lanes with the same (codon, t0, t1, t2) are joined (pack_device.h's wave_join) and the group's leader
//                adds the popcount — through the workgroup's counter frame (stream_count.h's CountFrame: LDS while
//                n <= TCMI_CODONS_LDS, else memory).  Counter 343 of a codon is ins_inside: the counted records whose token at the
//                first or second column carries the I mark, joined the same way.
// The sums are integers: their order does not matter and every run gives the same numbers.  The stream is only read.
#include <vector>

#include "stream_count.h"
#include "stream_walk.h"

namespace {

constexpr int BLOCK = SC_BLOCK;
constexpr int LDS_C = TCMI_CODONS_LDS;  // codons whose counters are staged
constexpr int NC = 7;                   // token classes
constexpr int NJ = NC * NC * NC;        // joint counters per codon
constexpr int NK = NJ + 1;              // ... and ins_inside behind them
constexpr int64_t MAX_CODONS = 1 << 14;
constexpr int64_t MAX_C0 = WALK_MAX_COL - 2;                // every column of a codon lies in [0, 2^29)
static_assert(LDS_C * (NK + 1) * 4 == 15180 && LDS_C * (NK + 1) * 4 <= 16384, "the staged columns and counters stay at or under 16 KiB");
static_assert(MAX_CODONS * NK < (1 << 23), "a counter's index fits the join's 32-bit key");
static_assert(sizeof(tcmi_codon_counts) == 346 * 4, "tcmi_codon_counts is 346 int32");

struct CcArgs {
    PackSrc src;                        // the resident stream, the read set's filter, floor and layout
    tcmi_primer_tab pt;                 // the primer table the read set was built under (none: zeros)
    const int32_t *c0;                  // [n] ascending: the codons' first columns
    int32_t *counts;                    // [n][344]
    int32_t n;
};

// a record's last three settled columns
struct Seen {
    int32_t top;                        // the columns below top are settled
    uint32_t hist;                      // nibble d: column top - 1 - d (class | I mark << 3); 0: below p, skipped, or no token
};

// the nibble of column c; c >= top - 3, and never below an earlier call's c - 2
__device__ inline uint32_t nibble_at(Walk &w, Seen &s, int32_t c, uint32_t Q)
{
    if (c < s.top) {
        const int32_t d = s.top - 1 - c;
        return d < 3 ? (s.hist >> (4 * d)) & 15u : 0u;
    }
    if (c > w.q) return 0u;                                 // (beyond the record: nothing, and no call)
    const int32_t gap = c - s.top;                          // the columns nobody asked for
    s.hist = gap < 3 ? s.hist << (4 * gap) : 0u;
    const uint32_t bits = token_at(w, c, Q);
    const uint32_t nib = class_of(bits) | (((bits >> TCMI_I) & 1u) << 3);
    s.hist = ((s.hist << 4) | nib) & 0xFFFu;
    s.top = c + 1;
    return nib;
}

__global__ __launch_bounds__(BLOCK) void codon_counts_kernel(CcArgs a)
{
    __shared__ int32_t s_c0[LDS_C];
    __shared__ uint32_t s_cnt[NK * LDS_C];
    const int tid = threadIdx.x, lane = tid & 63;
    const int n_cnt = NK * a.n;                             // (n <= 2^14: below 2^23)
    const CountFrame<int32_t> cnt = {s_cnt, a.counts, a.n <= LDS_C};
    if (cnt.staged) {
        for (int k = tid; k < a.n; k += BLOCK) s_c0[k] = a.c0[k];
        cnt.zero(n_cnt);
        __syncthreads();
    }
    const int32_t *c0 = cnt.staged ? s_c0 : a.c0;
    const uint32_t Q = a.src.min_bq;
    each_record(a.src.n, [&](int64_t i) {
        Walk w;
        Seen s = {0, 0u};
        int32_t ci = 0;
        bool live = i < a.src.n && open_walk(a.src, a.pt, i, w);
        if (live) {
            s.top = w.x;
            ci = first_at_or_above(c0, a.n, w.x - 2);       // (the first codon with c0 + 2 >= p)
            live = ci < a.n && c0[ci] <= w.q;
        }
        while (__ballot(live)) {                            // one round per codon of the wavefront's busiest record
            uint32_t t0 = 0u, t1 = 0u, t2 = 0u;
            if (live) {
                const int32_t c = c0[ci];
                t0 = nibble_at(w, s, c, Q);
                t1 = nibble_at(w, s, c + 1, Q);
                t2 = nibble_at(w, s, c + 2, Q);
            }
            const uint32_t cls = (t0 & 7u) * (NC * NC) + (t1 & 7u) * NC + (t2 & 7u);
            const uint32_t base = (uint32_t)ci * NK;        // (only read by a lane that counts)
            const bool counted = live && cls != 0u;
            // one pass per distinct (codon, t0, t1, t2)
            wave_join(counted, base + cls, [&](int lead, uint32_t lk, bool same) {
                const unsigned long long ms = __ballot(same);
                if (lane == lead) cnt.add(lk, __popcll(ms));
            });
            // ... and per codon with inserted bases inside (an I mark on the third column lies behind the codon)
            wave_join(counted && ((t0 | t1) & 8u) != 0u, base + NJ, [&](int lead, uint32_t lk, bool same) {
                const unsigned long long ms = __ballot(same);
                if (lane == lead) cnt.add(lk, __popcll(ms));
            });
            if (live) {
                ++ci;
                live = ci < a.n && c0[ci] <= w.q;
            }
        }
    });
    cnt.flush(n_cnt);
}

} // namespace

extern "C" int tcmi_readset_codon_counts(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t n, const int64_t *c0, tcmi_codon_counts *records)
{
    if (!ctx || !rs) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    if (n < 1 || n > MAX_CODONS) return tcmi_fail(ctx, TCMI_E_ARG, "codon counts: %lld codons: 1..16384 are allowed", (long long)n);
    if (!c0 || !records) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    for (int64_t i = 0; i < n; ++i) {
        if (c0[i] < 0 || c0[i] >= MAX_C0)
            return tcmi_fail(ctx, TCMI_E_ARG, "codon counts: codon %lld starts at column %lld, outside [0, 2^29 - 2)", (long long)i, (long long)c0[i]);
        if (i && c0[i] <= c0[i - 1])
            return tcmi_fail(ctx, TCMI_E_ARG, "codon counts: the codons are not strictly ascending at index %lld (%lld after %lld)", (long long)i,
                             (long long)c0[i], (long long)c0[i - 1]);
    }
    std::vector<int32_t> c32;
    std::vector<int64_t> sums;
    try {
        c32.assign(c0, c0 + n);
        sums.assign((size_t)NK * (size_t)n, 0);
    } catch (...) {                                         // (no exception may cross the C ABI)
        return tcmi_fail(ctx, TCMI_E_NOMEM, "codon counts: no host memory for %lld codons", (long long)n);
    }
    // the first columns (int32) in, [n][344] int32 counters out; the primer table is the one each part was built under.  The launch is
    // filed under the link counts' bracket (the profile slots are part of the ABI)
    const int rc = tcmi_stream_count_parts<int32_t>(
        ctx, rs, "codon counts", TCMI_K_LINK_COUNTS, c32.data(), c32.size() * 4, sums,
        [n](tcmi_ctx *cx, const tcmi_readset *part, const PackSrc &src, const char *d_in, int32_t *d_cnt, unsigned grid) {
            const CcArgs a = {src, tcmi_mask_args(part), reinterpret_cast<const int32_t *>(d_in), d_cnt, (int32_t)n};
            hipLaunchKernelGGL(codon_counts_kernel, dim3(grid), dim3(BLOCK), 0, cx->stream, a);
        });
    if (rc) return rc;
    for (int64_t i = 0; i < n; ++i) {
        tcmi_codon_counts &r = records[i];
        const int64_t *s = sums.data() + (size_t)i * NK;
        for (int x = 0; x < NC; ++x)
            for (int y = 0; y < NC; ++y)
                for (int z = 0; z < NC; ++z) r.j[x][y][z] = (int32_t)s[(x * NC + y) * NC + z];
        r.ins_inside = (int32_t)s[NJ];
        r.pos = (int32_t)c0[i];
        r.reserved = 0;
    }
    return TCMI_OK;
}
