// stream_count.h — HOST side (.hip files only) of the calls that go back to the inflated BAM stream a device-decoded read set left in
// its context's arena: is the stream still there (tally.hip's long reads, ins_entries.hip, the counting calls), grow-only scratch of a
// context, and the driver of a COUNTING call — one kernel over the records, one lane per record, that turns a small input (a table, a
// list of columns) into integer counters: tcmi_readset_amplicon_reads (amplicon_reads.hip), tcmi_readset_strand_counts
// (strand_counts.hip), tcmi_readset_link_counts (link_counts.hip).  Which record such a kernel counts: pack_device.h's kept_span.
#pragma once
#include <algorithm>
#include <cstring>

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

// One read set on its own context.  `in` (in_bytes, host) goes to the device, cnt_bytes of counters are zeroed behind it,
//   launch(ctx, rs, src, d_in, d_cnt, grid)   enqueues the one kernel on ctx->stream, between the profiling brackets of the caller's slot
//                                             (src: the resident stream with the read set's filter, floor and layout),
//   got(counts)                               adds the downloaded counters (pinned, cnt_bytes) into the caller's sums,
// one wait.  No launch when the set holds no record, nothing at all when it keeps none.  `what` goes in front of every message.
template <class Launch, class Got>
int tcmi_stream_count(tcmi_ctx *ctx, const tcmi_readset *rs, const char *what, const void *in, size_t in_bytes, size_t cnt_bytes, Launch launch, Got got)
{
    if (rs->packed_on_device != 2)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "%s: the read set was not decoded on the device (flat arrays or the host reader): there is no record stream to count in", what);
    if (rs->n_piled == 0) return TCMI_OK;                   // (no kept record: nothing to add; such a set may hold no stream at all)
    if (rs->device != ctx->device)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "%s: the read set lives on device %d, this context on device %d", what, rs->device, ctx->device);
    if (tcmi_stream_gone(ctx, rs) || !rs->d_rec_off)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "%s: the read set's decoded stream is no longer resident on this context (another upload happened on it)", what);
    if (rs->n_lay && rs->lay_gen != ctx->lay_gen)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "%s: the context's contig layout changed since the read set was uploaded", what);
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
        launch(ctx, rs, src, static_cast<const char *>(ctx->count_dev), d_cnt, (unsigned)grid);
        TCMI_HIP(ctx, hipGetLastError());
    }
    TCMI_HIP(ctx, hipMemcpyAsync(pin + b_in, d_cnt, cnt_bytes, hipMemcpyDeviceToHost, ctx->stream));
    TCMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    got(static_cast<const char *>(pin + b_in));
    return TCMI_OK;
}

// ... and a read set of sub-ranges (tcmi_split_step, "split_sub"): every record starts in exactly one part — the sum over the parts,
// each counted on its own context, where its stream lives; a part's error is worded on the caller's context
template <class Launch, class Got>
int tcmi_stream_count_parts(tcmi_ctx *ctx, const tcmi_readset *rs, const char *what, const void *in, size_t in_bytes, size_t cnt_bytes, Launch launch, Got got)
{
    if (rs->parts.empty()) return tcmi_stream_count(ctx, rs, what, in, in_bytes, cnt_bytes, launch, got);
    for (const tcmi_readset::Part &pt : rs->parts) {
        const int rc = tcmi_stream_count(pt.cx, pt.rs, what, in, in_bytes, cnt_bytes, launch, got);
        if (rc) return tcmi_fail(ctx, rc, "%s", pt.cx->err.c_str());
    }
    return TCMI_OK;
}

} // namespace
