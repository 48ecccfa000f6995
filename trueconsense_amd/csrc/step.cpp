// step.cpp — a step of a context: tally, the per-step tables (tables.cpp) and call over the context's workspace, begun and ended
// apart so that the host works meanwhile, and the pipeline's ride-along form whose call is carried by the next step's tally launch.
#include "tcmi_internal.h"

// The launches of one step on ctx->stream: [memset] tally, [the variant table's three,] [the amplicon table's one,] call.  When the counts are not wanted on the host the
// call kernel zeroes them behind itself and the next step into this workspace needs no memset.  The call records
// (3 bytes per position) go straight to the pinned host buffer: the kernel's own stores cross PCIe, which saves a
// separate copy and one launch boundary per step.
static int enqueue_step(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t L, int32_t mincov, int include_ambig, int want_counts,
                        bool memset_first)
{
    const int64_t ld = ctx->ws_ld;
    if (!rs->parts.empty()) return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "a read set of sub-ranges (tcmi_split_step) takes no step of its own: tcmi_tally_dev + tcmi_call_dev");
    if (memset_first) TCMI_HIP(ctx, hipMemsetAsync(ctx->d_counts, 0, (size_t)ld * TCMI_NCOL * 4, ctx->stream));
    int rc = tcmi_tally_dev(ctx, rs, L, ld, ctx->d_counts, 0);
    if (rc) return rc;
    rc = tcmi_tables_enqueue(ctx, L);
    if (rc) return rc;
    rc = tcmi_launch_call(ctx, ctx->d_counts, L, ld, mincov, include_ambig, want_counts ? 0 : 1, ctx->h_rec, ctx->h_rec + ld,
                          ctx->h_rec + 2 * ld, nullptr, nullptr);
    if (rc) return rc;
    if (want_counts)
        TCMI_HIP(ctx, hipMemcpyAsync(ctx->h_counts, ctx->d_counts, (size_t)ld * TCMI_NCOL * 4, hipMemcpyDeviceToHost, ctx->stream));
    return TCMI_OK;
}

// ---- ride-along call (used by the pipeline; internal C++ linkage: tcmi_internal.h) -------------------------------
// A step without its call kernel: the tally is launched now; the call of this matrix is carried by the tally launch
// of the NEXT step on the stream (`prev` of that call), or launched on its own by tcmi_step_flush.  One launch per
// step instead of two, and the call's PCIe stores overlap with the next tally's streaming.
static int launch_pending_call(tcmi_ctx *ctx)
{
    const int64_t ld = ctx->ws_ld;
    int rc = tcmi_launch_call(ctx, ctx->d_counts, ctx->pend_L, ld, ctx->pend_mincov, ctx->pend_amb, 1, ctx->h_rec, ctx->h_rec + ld,
                              ctx->h_rec + 2 * ld, nullptr, nullptr);
    if (rc) return rc;
    TCMI_HIP(ctx, hipEventRecord(ctx->step_done, ctx->stream));
    ctx->call_pending = false;
    ctx->counts_clean = true;
    return TCMI_OK;
}

int tcmi_step_flush(tcmi_ctx *ctx)
{
    if (!ctx) return tcmi_fail(ctx, TCMI_E_ARG, "ctx is NULL");
    if (!ctx->call_pending) return TCMI_OK;
    TCMI_HIP(ctx, hipSetDevice(ctx->device));
    return launch_pending_call(ctx);
}

int tcmi_step_begin_deferred(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t L, int32_t mincov, int include_ambig, tcmi_ctx *prev)
{
    if (!ctx || !rs) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    if (L <= 0 || rs->max_end > L) return tcmi_fail(ctx, TCMI_E_ARG, "L=%lld does not cover the reads (extent %lld)", (long long)L, (long long)rs->max_end);
    if (rs->device != ctx->device) return tcmi_fail(ctx, TCMI_E_ARG, "read set lives on device %d, context on %d", rs->device, ctx->device);
    if (ctx->step_L > 0 || ctx->call_pending) return tcmi_fail(ctx, TCMI_E_ARG, "tcmi_step_begin: the previous step of this context has not been ended");
    if (tcmi_var_table_on(ctx))
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "a variant table (--variant-table, tcmi_ctx_set_variants) is set on this context: the array pipeline's ride-along steps compute none; use tcmi_step or the file runner");
    if (tcmi_iv_table_on(ctx))
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "an amplicon table (--amplicon-table, tcmi_ctx_set_intervals) is set on this context: the array pipeline's ride-along steps compute none; use tcmi_step or the file runner");
    int rc = tcmi_ws_ensure(ctx, L);
    if (rc) return rc;
    TCMI_HIP(ctx, hipSetDevice(ctx->device));
    if (prev && (prev == ctx || !prev->call_pending)) prev = nullptr;
    if (prev && prev->stream != ctx->stream) {                 // no stream order between the two: the call goes out on its own
        rc = launch_pending_call(prev);
        if (rc) return rc;
        prev = nullptr;
    }
    if (!ctx->counts_clean) TCMI_HIP(ctx, hipMemsetAsync(ctx->d_counts, 0, (size_t)ctx->ws_ld * TCMI_NCOL * 4, ctx->stream));
    ctx->counts_clean = false;
    const bool sampled = ctx->prof && (ctx->step_tick++ % ctx->prof_every) == 0;
    tcmi_ride ride = {};
    if (prev) {
        ride.counts = prev->d_counts; ride.ld = prev->ws_ld; ride.L = prev->pend_L; ride.mincov = prev->pend_mincov;
        ride.amb = prev->pend_amb; ride.plain = prev->h_rec; ride.alt = prev->h_rec + prev->ws_ld; ride.flags = prev->h_rec + 2 * prev->ws_ld;
        ctx->ride = &ride;
    }
    ctx->prof_mute = !sampled;
    rc = tcmi_tally_dev(ctx, rs, L, ctx->ws_ld, ctx->d_counts, 0);
    ctx->prof_mute = false;
    ctx->ride = nullptr;
    if (rc) return rc;
    if (prev) {
        if (ride.taken) {
            TCMI_HIP(ctx, hipEventRecord(prev->step_done, ctx->stream));
            prev->call_pending = false;
            prev->counts_clean = true;
        } else {                                               // this step had no fast-kernel launch to carry it
            rc = launch_pending_call(prev);
            if (rc) return rc;
        }
    }
    ctx->call_pending = true;
    ctx->pend_L = L; ctx->pend_mincov = mincov; ctx->pend_amb = include_ambig;
    ctx->step_L = L;
    ctx->step_counts = false;
    tcmi_tables_step_begin(ctx, true);
    return TCMI_OK;
}

extern "C" {

int tcmi_step_begin(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t L, int32_t mincov, int include_ambig, int want_counts)
{
    if (!ctx || !rs) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    if (L <= 0 || rs->max_end > L) return tcmi_fail(ctx, TCMI_E_ARG, "L=%lld does not cover the reads (extent %lld)", (long long)L, (long long)rs->max_end);
    if (rs->device != ctx->device) return tcmi_fail(ctx, TCMI_E_ARG, "read set lives on device %d, context on %d", rs->device, ctx->device);
    if (ctx->step_L > 0) return tcmi_fail(ctx, TCMI_E_ARG, "tcmi_step_begin: the previous step of this context has not been ended");
    int rc = tcmi_ws_ensure(ctx, L);
    if (rc) return rc;
    TCMI_HIP(ctx, hipSetDevice(ctx->device));
    const bool memset_first = !ctx->counts_clean;
    ctx->counts_clean = false;
    // with profiling on, every prof_every-th step has its kernels bracketed by events
    const bool sampled = ctx->prof && (ctx->step_tick++ % ctx->prof_every) == 0;
    ctx->prof_mute = !sampled;
    rc = enqueue_step(ctx, rs, L, mincov, include_ambig, want_counts, memset_first);
    ctx->prof_mute = false;
    if (rc) return rc;
    ctx->counts_clean = !want_counts;
    TCMI_HIP(ctx, hipEventRecord(ctx->step_done, ctx->stream));
    ctx->step_L = L;
    ctx->step_counts = want_counts != 0;
    tcmi_tables_step_begin(ctx, false);
    return TCMI_OK;
}

int tcmi_step_end(tcmi_ctx *ctx, const uint8_t **plain, const uint8_t **alt, const uint8_t **flags,
                  const int32_t **counts_planes, int64_t *ld_out)
{
    if (!ctx) return tcmi_fail(ctx, TCMI_E_ARG, "ctx is NULL");
    if (ctx->step_L <= 0) return tcmi_fail(ctx, TCMI_E_ARG, "tcmi_step_end without tcmi_step_begin");
    if (ctx->call_pending) {                                  // nobody carried this step's call: launch it now
        const int rc = tcmi_step_flush(ctx);
        if (rc) return rc;
    }
    TCMI_HIP(ctx, hipEventSynchronize(ctx->step_done));      // only this step: the stream may be shared
    const int64_t ld = ctx->ws_ld;
    if (plain) *plain = ctx->h_rec;
    if (alt) *alt = ctx->h_rec + ld;
    if (flags) *flags = ctx->h_rec + 2 * ld;
    if (counts_planes) *counts_planes = ctx->step_counts ? ctx->h_counts : nullptr;
    if (ld_out) *ld_out = ld;
    tcmi_tables_step_end(ctx);
    ctx->step_L = 0;
    return TCMI_OK;
}

int tcmi_step(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t L, int32_t mincov, int include_ambig,
              const uint8_t **plain, const uint8_t **alt, const uint8_t **flags, const int32_t **counts_planes,
              int64_t *ld_out)
{
    const int rc = tcmi_step_begin(ctx, rs, L, mincov, include_ambig, counts_planes != nullptr);
    if (rc) return rc;
    return tcmi_step_end(ctx, plain, alt, flags, counts_planes, ld_out);
}

} // extern "C"
