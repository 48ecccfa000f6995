// amplicon_reads.hip — --amplicon-reads on gfx950: the records of a device-decoded read set, read where they lie in the inflated BAM
// stream the packer left in the context's arena, counted per amplicon of a scheme (include/tcmi.h: tcmi_readset_amplicon_reads; the
// rule, the compiled table and the lookup: amplicon_reads_rule.h).
//
// Here: the kernel and the entry that compiles the table and unpacks the sums.  Which record is kept and where it lies on the axis:
// pack_device.h's kept_span; the residency refusals, the scratch, the launch shape, the download and the sub-ranges: stream_count.h.
//
// One launch, one lane per record, 256-lane workgroups that stride over the records: the grid is min(ceil(records / 256), compute
// units x 8).  Eight workgroups per CU is what the kernel's LDS (16 KiB: the table and the counters of up to TCMI_AMPLICON_READS_LDS
// amplicons) and its wavefront slots admit; striding instead of one workgroup per 256 records lets a workgroup stage the table once and
// hand its counters to memory once, whatever the file's size.  No workgroup waits for another.
//   per record   kept_span (the fixed fields, the read filter, the contig's shift, one walk over the CIGAR for the reference span), then
//                the lookup: a binary search over the widened starts and three more words.
//   the table    staged in LDS while n <= TCMI_AMPLICON_READS_LDS; a larger one is searched where it lies (L2).
//   counters     a sorted BAM puts a wavefront's 64 reads into one or two amplicons: the lanes that hit the same counter are joined
//                first (pack_device.h's wave_join), and the group's leader adds two popcounts, `reads` and, when any, `full` — through
//                the workgroup's counter frame (stream_count.h's CountFrame: LDS while the table is staged, else memory).
// The sums are integers: their order does not matter and every run gives the same numbers.  The stream is only read.
#include <vector>

#include "stream_count.h"
#include "amplicon_reads_rule.h"

namespace {

constexpr int BLOCK = SC_BLOCK;
constexpr int LDS_N = TCMI_AMPLICON_READS_LDS;

struct ArArgs {
    PackSrc src;                    // the resident stream, the read set's filter and layout
    const int32_t *table;           // [6 * n] (amplicon_reads_rule.h)
    unsigned long long *counts;     // [2 * (n + 2)]: {reads, full} of amplicon i at 2 i; ambiguous at 2 n, unassigned at 2 n + 2
    int32_t n;
};

// the counter slot of record i: the amplicon's index, n (ambiguous), n + 1 (unassigned), or -1 for a record that is not kept
__device__ inline int32_t slot_of(const ArArgs &a, const tcmi_ar_table &tab, int64_t i, bool *full)
{
    *full = false;
    ReadView v;
    int64_t p, q;
    if (!kept_span(a.src, i, v, p, q)) return -1;
    // (the packer refuses a file with a read that ends at or beyond 2^29; a column up there is beyond every amplicon all the same)
    const int32_t hit = tcmi_ar_lookup(tab, (int32_t)(p < INT32_MAX ? p : INT32_MAX), (int32_t)(q < INT32_MAX ? q : INT32_MAX), full);
    return hit >= 0 ? hit : hit == TCMI_AR_AMBIGUOUS ? a.n : a.n + 1;
}

__global__ __launch_bounds__(BLOCK) void amplicon_reads_kernel(ArArgs a)
{
    __shared__ int32_t s_tab[TCMI_AR_WORDS * LDS_N];
    __shared__ uint32_t s_cnt[2 * (LDS_N + 2)];
    const int tid = threadIdx.x, lane = tid & 63;
    const CountFrame<unsigned long long> cnt = {s_cnt, a.counts, a.n <= LDS_N};
    const int n_cnt = 2 * (a.n + 2);
    if (cnt.staged) {
        for (int k = tid; k < TCMI_AR_WORDS * a.n; k += BLOCK) s_tab[k] = a.table[k];
        cnt.zero(n_cnt);
        __syncthreads();
    }
    const tcmi_ar_table tab = tcmi_ar_view(cnt.staged ? s_tab : a.table, a.n);
    each_record(a.src.n, [&](int64_t i) {
        bool full = false;
        const int32_t slot = i < a.src.n ? slot_of(a, tab, i, &full) : -1;
        wave_join(slot >= 0, slot, [&](int lead, int32_t ls, bool same) {   // one pass per distinct counter the wavefront's reads hit
            const unsigned long long ms = __ballot(same), mf = __ballot(same && full);
            if (lane == lead) {
                cnt.add(2 * (int64_t)ls, __popcll(ms));
                if (mf) cnt.add(2 * (int64_t)ls + 1, __popcll(mf));
            }
        });
    });
    cnt.flush(n_cnt);
}

} // namespace

extern "C" int tcmi_readset_amplicon_reads(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t n, const int64_t *fs, const int64_t *le, const int64_t *rs_,
                                           const int64_t *fe, int32_t slack, tcmi_amplicon_reads *records)
{
    if (!ctx || !rs || !records) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    char msg[200] = "";
    std::vector<int32_t> table;
    std::vector<int64_t> sums;
    try {
        if (n >= 1 && n <= TCMI_AR_MAX_N) { table.resize((size_t)TCMI_AR_WORDS * (size_t)n); sums.assign((size_t)2 * ((size_t)n + 2), 0); }
    } catch (...) {                                         // (no exception may cross the C ABI)
        return tcmi_fail(ctx, TCMI_E_NOMEM, "amplicon reads: no host memory for %lld amplicons", (long long)n);
    }
    if (tcmi_amplicon_reads_build(n, fs, le, rs_, fe, slack, table.data(), msg, sizeof msg)) return tcmi_fail(ctx, TCMI_E_ARG, "amplicon reads: %s", msg);
    // the compiled table (6 n words) in, {reads, full} of n + 2 slots out
    const int rc = tcmi_stream_count_parts<unsigned long long>(
        ctx, rs, "amplicon reads", TCMI_K_AMPLICON_READS, table.data(), table.size() * 4, sums,
        [n](tcmi_ctx *cx, const tcmi_readset *, const PackSrc &src, const char *d_in, unsigned long long *d_cnt, unsigned grid) {
            const ArArgs a = {src, reinterpret_cast<const int32_t *>(d_in), d_cnt, (int32_t)n};
            hipLaunchKernelGGL(amplicon_reads_kernel, dim3(grid), dim3(BLOCK), 0, cx->stream, a);
        });
    if (rc) return rc;
    for (int64_t i = 0; i < n + 2; ++i) { records[i].reads = sums[(size_t)(2 * i)]; records[i].full = sums[(size_t)(2 * i + 1)]; }
    return TCMI_OK;
}
