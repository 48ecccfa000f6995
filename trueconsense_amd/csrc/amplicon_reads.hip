// amplicon_reads.hip — --amplicon-reads on gfx950: the records of a device-decoded read set, read where they lie in the inflated BAM
// stream the packer left in the context's arena, counted per amplicon of a scheme (include/tcmi.h: tcmi_readset_amplicon_reads; the
// rule, the compiled table and the lookup: amplicon_reads_rule.h).
//
// One launch, one lane per record, 256-lane workgroups that stride over the records: the grid is min(ceil(records / 256), compute
// units x 8).  Eight workgroups per CU is what the kernel's LDS (16 KiB: the table and the counters of up to TCMI_AMPLICON_READS_LDS
// amplicons) and its wavefront slots admit; striding instead of one workgroup per 256 records lets a workgroup stage the table once and
// hand its counters to memory once, whatever the file's size.  No workgroup waits for another.
//   per record   the fixed fields (view_rec: two unaligned loads), the read filter the set was built under (passes), the contig's
//                shift (shift_of), one walk over the CIGAR for the reference span — unaligned dword loads, no base is read —, then
//                the lookup: a binary search over the widened starts and three more words.
//   the table    staged in LDS while n <= TCMI_AMPLICON_READS_LDS; a larger one is searched where it lies (L2).
//   counters     a sorted BAM puts a wavefront's 64 reads into one or two amplicons: the lanes that hit the same counter are joined
//                first (a ballot loop over the distinct ids: one pass per id the wavefront holds), and one lane adds the popcount —
//                to the workgroup's counters in LDS while the table is staged, else straight to memory.  At its end a workgroup
//                hands every non-zero LDS counter to memory with one atomic add.
// The sums are integers: their order does not matter and every run gives the same numbers.  The stream is only read.
#include <algorithm>
#include <cstring>
#include <vector>

#include "pack_device.h"
#include "amplicon_reads_rule.h"

namespace {

constexpr int BLOCK = 256;
constexpr int LDS_N = TCMI_AMPLICON_READS_LDS;
constexpr int WG_PER_CU = 8;

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
    const ReadView v = view_rec(a.src.stream + a.src.rec_off[i]);
    // kept exactly when the device packer keeps it (pack_device.hip: classify_view)
    if ((v.flag & 0x4u) || !passes(a.src.flt, v) || v.bad || v.pos < 0) return -1;
    const int32_t shift = shift_of(a.src, v.tid);
    if (shift < 0) return -1;
    int64_t span = 0;
    for (uint32_t k = 0; k < v.n_cigar; ++k) {
        const uint32_t c = ld_u32(v.cigar + 4 * (size_t)k);
        if (consumes_ref(c & 0xFu)) span += c >> 4;
    }
    if (span <= 0) return -1;
    const int64_t p = (int64_t)v.pos + shift, q = p + span - 1;
    // (the packer refuses a file with a read that ends at or beyond 2^29; a column up there is beyond every amplicon all the same)
    const int32_t hit = tcmi_ar_lookup(tab, (int32_t)(p < INT32_MAX ? p : INT32_MAX), (int32_t)(q < INT32_MAX ? q : INT32_MAX), full);
    return hit >= 0 ? hit : hit == TCMI_AR_AMBIGUOUS ? a.n : a.n + 1;
}

__global__ __launch_bounds__(BLOCK) void amplicon_reads_kernel(ArArgs a)
{
    __shared__ int32_t s_tab[TCMI_AR_WORDS * LDS_N];
    __shared__ uint32_t s_cnt[2 * (LDS_N + 2)];
    const int tid = threadIdx.x, lane = tid & 63;
    const bool staged = a.n <= LDS_N;                       // (uniform)
    const int n_cnt = 2 * (a.n + 2);
    if (staged) {
        for (int k = tid; k < TCMI_AR_WORDS * a.n; k += BLOCK) s_tab[k] = a.table[k];
        for (int k = tid; k < n_cnt; k += BLOCK) s_cnt[k] = 0u;
        __syncthreads();
    }
    const tcmi_ar_table tab = tcmi_ar_view(staged ? s_tab : a.table, a.n);
    // (the bound is uniform over the workgroup: every lane of a wavefront takes part in every ballot)
    for (int64_t base = (int64_t)blockIdx.x * BLOCK; base < a.src.n; base += (int64_t)gridDim.x * BLOCK) {
        const int64_t i = base + tid;
        bool full = false;
        const int32_t slot = i < a.src.n ? slot_of(a, tab, i, &full) : -1;
        bool todo = slot >= 0;
        for (;;) {                                          // one pass per distinct counter the wavefront's reads hit
            const unsigned long long m = __ballot(todo);
            if (!m) break;
            const int lead = (int)__builtin_ctzll(m);
            const int32_t ls = __shfl(slot, lead, 64);
            const bool same = todo && slot == ls;
            const unsigned long long ms = __ballot(same), mf = __ballot(same && full);
            if (lane == lead) {
                if (staged) {
                    atomicAdd(&s_cnt[2 * ls], (uint32_t)__popcll(ms));
                    if (mf) atomicAdd(&s_cnt[2 * ls + 1], (uint32_t)__popcll(mf));
                } else {
                    atomicAdd(&a.counts[2 * (int64_t)ls], (unsigned long long)__popcll(ms));
                    if (mf) atomicAdd(&a.counts[2 * (int64_t)ls + 1], (unsigned long long)__popcll(mf));
                }
            }
            if (same) todo = false;
        }
    }
    if (staged) {
        __syncthreads();
        for (int k = tid; k < n_cnt; k += BLOCK) {
            const uint32_t c = s_cnt[k];
            if (c) atomicAdd(&a.counts[k], (unsigned long long)c);
        }
    }
}

// one read set on its own context: the compiled table (host, 6 n words) -> sums[2 * (n + 2)] ADDED to
int count_one(tcmi_ctx *ctx, const tcmi_readset *rs, int32_t n, const int32_t *table, int64_t *sums)
{
    if (rs->packed_on_device != 2)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "amplicon reads: the read set was not decoded on the device (flat arrays or the host reader): there is no record stream to count in");
    if (rs->n_piled == 0) return TCMI_OK;                   // (no kept record: nothing to add; such a set may hold no stream at all)
    if (rs->device != ctx->device)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "amplicon reads: the read set lives on device %d, this context on device %d", rs->device, ctx->device);
    if (!rs->d_stream || !rs->d_rec_off || rs->arena_epoch != ctx->arena_epoch)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "amplicon reads: the read set's decoded stream is no longer resident on this context (another upload happened on it)");
    if (rs->n_lay && rs->lay_gen != ctx->lay_gen)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "amplicon reads: the context's contig layout changed since the read set was uploaded");
    TCMI_HIP(ctx, hipSetDevice(ctx->device));
    const size_t b_tab = tcmi_align256((size_t)TCMI_AR_WORDS * n * 4), b_cnt = tcmi_align256((size_t)2 * (n + 2) * 8);
    // scratch of the context, grow-only (no hipMalloc / hipFree per call: hipFree waits for the whole device)
    if (ctx->ar_dev_cap < b_tab + b_cnt) {
        if (ctx->ar_dev) { TCMI_HIP(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(ctx->ar_dev); ctx->ar_dev = nullptr; ctx->ar_dev_cap = 0; }
        const size_t want = b_tab + b_cnt + (64u << 10);
        if (hipMalloc((void **)&ctx->ar_dev, want) != hipSuccess) return tcmi_fail(ctx, TCMI_E_NOMEM, "amplicon reads: device scratch (%zu bytes)", want);
        ctx->ar_dev_cap = want;
    }
    char *pin = static_cast<char *>(tcmi_ctx_pinned(ctx, b_tab + b_cnt));
    if (!pin) return tcmi_fail(ctx, TCMI_E_NOMEM, "amplicon reads: pinned scratch");
    std::memcpy(pin, table, (size_t)TCMI_AR_WORDS * n * 4);
    ArArgs a;
    a.src = stream_src(rs);
    a.src.lay = rs->d_lay; a.src.n_lay = rs->n_lay;
    a.table = reinterpret_cast<const int32_t *>(ctx->ar_dev);
    a.counts = reinterpret_cast<unsigned long long *>(ctx->ar_dev + b_tab);
    a.n = n;
    TCMI_HIP(ctx, hipMemcpyAsync(ctx->ar_dev, pin, (size_t)TCMI_AR_WORDS * n * 4, hipMemcpyHostToDevice, ctx->stream));
    TCMI_HIP(ctx, hipMemsetAsync(a.counts, 0, (size_t)2 * (n + 2) * 8, ctx->stream));
    if (rs->n_reads > 0) {
        const int64_t blocks = (rs->n_reads + BLOCK - 1) / BLOCK;
        const int64_t grid = std::min<int64_t>(blocks, (int64_t)std::max(ctx->n_cu, 1) * WG_PER_CU);
        (void)hipGetLastError();                            // drop any stale error of this thread
        tcmi_prof_begin(ctx, TCMI_K_AMPLICON_READS);
        hipLaunchKernelGGL(amplicon_reads_kernel, dim3((unsigned)grid), dim3(BLOCK), 0, ctx->stream, a);
        tcmi_prof_end(ctx, TCMI_K_AMPLICON_READS);
        TCMI_HIP(ctx, hipGetLastError());
    }
    TCMI_HIP(ctx, hipMemcpyAsync(pin + b_tab, a.counts, (size_t)2 * (n + 2) * 8, hipMemcpyDeviceToHost, ctx->stream));
    TCMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int64_t *got = reinterpret_cast<const int64_t *>(pin + b_tab);
    for (int64_t k = 0; k < 2 * ((int64_t)n + 2); ++k) sums[k] += got[k];
    return TCMI_OK;
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
    if (!rs->parts.empty()) {
        // a read set of sub-ranges (tcmi_split_step, "split_sub"): every record starts in exactly one part — the sum over the parts,
        // each counted on its own context, where its stream lives
        for (const tcmi_readset::Part &pt : rs->parts) {
            const int rc = count_one(pt.cx, pt.rs, (int32_t)n, table.data(), sums.data());
            if (rc) return tcmi_fail(ctx, rc, "%s", pt.cx->err.c_str());
        }
    } else {
        const int rc = count_one(ctx, rs, (int32_t)n, table.data(), sums.data());
        if (rc) return rc;
    }
    for (int64_t i = 0; i < n + 2; ++i) { records[i].reads = sums[(size_t)(2 * i)]; records[i].full = sums[(size_t)(2 * i + 1)]; }
    return TCMI_OK;
}
