// stream_count.h — (.hip files only) the calls that go back to the inflated BAM stream a device-decoded read set left in its context's
// arena.  HOST side: is the stream still there (tally.hip's long reads, ins_entries.hip, the counting calls), grow-only scratch of a
// context, and the driver of a COUNTING call — one kernel over the records, one lane per record, that turns a small input (a table, a
// list of columns) into integer counters: tcmi_readset_amplicon_reads (amplicon_reads.hip), tcmi_readset_strand_counts
// (strand_counts.hip), tcmi_readset_link_counts (link_counts.hip), tcmi_readset_codon_counts (codon_counts.hip) — with the column check
// of the strand and link counts; tcmi_readset_indel_events
// (indel_events.hip) keeps a driver of its own (a keyed table, attempts) on the same refusals, scratch and launch shape.  DEVICE side,
// at the end: the frame such a kernel holds around its counting rule — the workgroup's counters (CountFrame) and the walk over the
// records (each_record).  Which record such a kernel counts: pack_device.h's kept_span; how its lanes are joined per counter:
// wave_join there.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "pack_device.h"

namespace {

// one lane per record, 256-lane workgroups that stride over the records; eight workgroups per CU is what the counting kernels' LDS
// (15 - 16 KiB) and their wavefront slots admit
constexpr int SC_BLOCK = 256;
constexpr int SC_WG_PER_CU = 8;

// the read set's decoded stream is not (or no longer) on this context: no stream, another upload since, or another device
inline bool tcmi_stream_gone(const tcmi_ctx *ctx, const tcmi_readset *rs)
{
    return !rs->d_stream || rs->arena_epoch != ctx->arena_epoch || rs->device != ctx->device;
}

// Grow-only scratch of a context: at least `bytes` behind p afterwards, `bytes + slack` when it had to grow (what was there is lost).
// No hipMalloc / hipFree per call: they cost more than the kernels, and hipFree waits for the whole device.  false: no memory.
inline bool tcmi_grow_dev(tcmi_ctx *ctx, char *&p, size_t &cap, size_t bytes, size_t slack)
{
    if (cap >= bytes) return true;
    if (p) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(p); p = nullptr; cap = 0; }
    if (hipMalloc((void **)&p, bytes + slack) != hipSuccess) { p = nullptr; return false; }
    cap = bytes + slack;
    return true;
}
inline bool tcmi_grow_pinned(tcmi_ctx *ctx, char *&p, size_t &cap, size_t bytes, size_t slack)
{
    if (cap >= bytes) return true;
    if (p) { (void)hipStreamSynchronize(ctx->stream); (void)hipHostFree(p); p = nullptr; cap = 0; }
    if (hipHostMalloc((void **)&p, bytes + slack, hipHostMallocDefault) != hipSuccess) { p = nullptr; return false; }
    cap = bytes + slack;
    return true;
}

// The columns of a query (strand counts, link counts): each in [0, 2^29), strictly ascending; narrowed to int32 into c32.  `what` goes in
// front of every message.
inline int tcmi_count_columns(tcmi_ctx *ctx, const char *what, int64_t n, const int64_t *cols, std::vector<int32_t> &c32)
{
    for (int64_t i = 0; i < n; ++i) {
        if (cols[i] < 0 || cols[i] >= WALK_MAX_COL)
            return tcmi_fail(ctx, TCMI_E_ARG, "%s: column %lld (%lld) lies outside [0, 2^29)", what, (long long)i, (long long)cols[i]);
        if (i && cols[i] <= cols[i - 1])
            return tcmi_fail(ctx, TCMI_E_ARG, "%s: the columns are not strictly ascending at index %lld (%lld after %lld)", what, (long long)i,
                             (long long)cols[i], (long long)cols[i - 1]);
    }
    try {
        c32.assign(cols, cols + n);
    } catch (...) {                                         // (no exception may cross the C ABI)
        return tcmi_fail(ctx, TCMI_E_NOMEM, "%s: no host memory for %lld columns", what, (long long)n);
    }
    return TCMI_OK;
}

// May a call count in the read set's record stream on this context?  TCMI_OK: yes; 1: there is nothing to count (no kept record: such a
// set may hold no stream at all); < 0: refused, worded on ctx with `what` in front.  The refusals of every counting call, the indel
// events' (indel_events.hip) included.
inline int tcmi_stream_countable(tcmi_ctx *ctx, const tcmi_readset *rs, const char *what)
{
    if (rs->packed_on_device != 2)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "%s: the read set was not decoded on the device (flat arrays or the host reader): there is no record stream to count in", what);
    if (rs->n_piled == 0) return 1;
    if (rs->device != ctx->device)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "%s: the read set lives on device %d, this context on device %d", what, rs->device, ctx->device);
    if (tcmi_stream_gone(ctx, rs) || !rs->d_rec_off)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "%s: the read set's decoded stream is no longer resident on this context (another upload happened on it)", what);
    if (rs->n_lay && rs->lay_gen != ctx->lay_gen)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "%s: the context's contig layout changed since the read set was uploaded", what);
    return TCMI_OK;
}

// One read set on its own context.  `in` (in_bytes, host) goes to the device, sums.size() counters of type T are zeroed behind it,
//   launch(ctx, rs, src, d_in, d_cnt, grid)   enqueues the one kernel on ctx->stream (src: the resident stream with the read set's
//                                             filter, floor and layout), here between the profiling brackets of `slot`,
// the downloaded counters (pinned) are added into `sums`, one wait.  No launch when the set holds no record, nothing at all when it
// keeps none.  `what` goes in front of every message.
template <class T, class Launch>
int tcmi_stream_count(tcmi_ctx *ctx, const tcmi_readset *rs, const char *what, int slot, const void *in, size_t in_bytes, std::vector<int64_t> &sums, Launch launch)
{
    const size_t cnt_bytes = sums.size() * sizeof(T);
    if (const int rc = tcmi_stream_countable(ctx, rs, what)) return rc < 0 ? rc : TCMI_OK;
    TCMI_HIP(ctx, hipSetDevice(ctx->device));
    const size_t b_in = tcmi_align256(in_bytes), b_cnt = tcmi_align256(cnt_bytes);
    if (!tcmi_grow_dev(ctx, ctx->count_dev, ctx->count_dev_cap, b_in + b_cnt, 64u << 10))
        return tcmi_fail(ctx, TCMI_E_NOMEM, "%s: device scratch (%zu bytes)", what, b_in + b_cnt + (64u << 10));
    char *pin = static_cast<char *>(tcmi_ctx_pinned(ctx, b_in + b_cnt));
    if (!pin) return tcmi_fail(ctx, TCMI_E_NOMEM, "%s: pinned scratch", what);
    std::memcpy(pin, in, in_bytes);
    PackSrc src = stream_src(rs);
    src.lay = rs->d_lay; src.n_lay = rs->n_lay;
    char *d_cnt = ctx->count_dev + b_in;
    TCMI_HIP(ctx, hipMemcpyAsync(ctx->count_dev, pin, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    TCMI_HIP(ctx, hipMemsetAsync(d_cnt, 0, cnt_bytes, ctx->stream));
    if (rs->n_reads > 0) {
        const int64_t blocks = (rs->n_reads + SC_BLOCK - 1) / SC_BLOCK;
        const int64_t grid = std::min<int64_t>(blocks, (int64_t)std::max(ctx->n_cu, 1) * SC_WG_PER_CU);
        (void)hipGetLastError();                            // drop any stale error of this thread
        tcmi_prof_begin(ctx, slot);
        launch(ctx, rs, src, static_cast<const char *>(ctx->count_dev), reinterpret_cast<T *>(d_cnt), (unsigned)grid);
        tcmi_prof_end(ctx, slot);
        TCMI_HIP(ctx, hipGetLastError());
    }
    TCMI_HIP(ctx, hipMemcpyAsync(pin + b_in, d_cnt, cnt_bytes, hipMemcpyDeviceToHost, ctx->stream));
    TCMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const T *got = reinterpret_cast<const T *>(pin + b_in);
    int64_t *s = sums.data();
    for (size_t k = 0, m = sums.size(); k < m; ++k) s[k] += (int64_t)got[k];
    return TCMI_OK;
}

// ... and a read set of sub-ranges (tcmi_split_step, "split_sub"): every record starts in exactly one part — the sum over the parts,
// each counted on its own context, where its stream lives; a part's error is worded on the caller's context
template <class T, class Launch>
int tcmi_stream_count_parts(tcmi_ctx *ctx, const tcmi_readset *rs, const char *what, int slot, const void *in, size_t in_bytes, std::vector<int64_t> &sums, Launch launch)
{
    if (rs->parts.empty()) return tcmi_stream_count<T>(ctx, rs, what, slot, in, in_bytes, sums, launch);
    for (const tcmi_readset::Part &pt : rs->parts) {
        const int rc = tcmi_stream_count<T>(pt.cx, pt.rs, what, slot, in, in_bytes, sums, launch);
        if (rc) return tcmi_fail(ctx, rc, "%s", pt.cx->err.c_str());
    }
    return TCMI_OK;
}

// ---- DEVICE: the frame of a counting kernel ---------------------------------------------------------------------------------------------
// The workgroup's counters.  While the query fits (`staged`, uniform over the grid) a workgroup counts in LDS and hands every non-zero
// counter to memory once, at its end; a larger query is counted straight in memory (T: the memory counter's type).  The kernel declares
// the LDS array and its size, stages its own table or columns beside zero(), and syncs once.
template <class T> struct CountFrame {
    uint32_t *lds;                      // [n] while staged
    T *mem;                             // [n], zeroed by the host
    bool staged;
    // (staged only; the kernel's __syncthreads follows)
    __device__ void zero(int n) const { for (int k = threadIdx.x; k < n; k += SC_BLOCK) lds[k] = 0u; }
    // one lane adds c to counter k
    __device__ void add(int64_t k, int c) const
    {
        if (staged) atomicAdd(&lds[k], (uint32_t)c);
        else atomicAdd(&mem[k], (T)c);
    }
    // every lane of the workgroup, behind its last add
    __device__ void flush(int n) const
    {
        if (!staged) return;
        __syncthreads();
        for (int k = threadIdx.x; k < n; k += SC_BLOCK) {
            const uint32_t c = lds[k];
            if (c) atomicAdd(&mem[k], (T)c);
        }
    }
};

// The workgroup's walk over the n records of the stream: f(i) with one lane per record, the workgroups striding over the records.  The
// bound is uniform over the workgroup, so EVERY lane of a wavefront calls f together, also with i >= n (it has no record then): f may
// ballot, shuffle and wave_join.
template <class F> __device__ inline void each_record(int64_t n, F f)
{
    for (int64_t base = (int64_t)blockIdx.x * SC_BLOCK; base < n; base += (int64_t)gridDim.x * SC_BLOCK) f(base + (int64_t)threadIdx.x);
}

// the records of the stream a mate job (mate_join.hip, dedup.hip) walks (uniform over the grid): the host's count, or what pk_index left
__device__ inline int64_t record_count(const tcmi_mate_job &a)
{
    if (a.n >= 0) return a.n;
    if (a.n_blocks <= 0 || (*a.flags & a.ovf)) return 0;       // (an index with holes: the host declines the file after its wait)
    const int32_t b = a.n_blocks - 1;
    const uint64_t n = (uint64_t)a.rec_base[b] + (b < a.n_own ? a.n_rec[b] : 0u);
    return (int64_t)(n < a.rec_cap ? n : a.rec_cap);
}

} // namespace
