// tables.cpp — the two per-step tables, everything but their kernels: the variant table (variants.hip) and the amplicon table
// (intervals.hip) as calls of their own, as settings of a context, and as the launches of a step between its tally and its call.
#include <algorithm>
#include <cstring>
#include <memory>
#include <new>

#include "tcmi_internal.h"
#include "intervals_rule.h"

// ---- variant table (variants.hip) --------------------------------------------------------------
static int var_rule_build(tcmi_ctx *ctx, int64_t num, int64_t den, int32_t min_alt_depth, int32_t min_depth, tcmi_var_rule *out)
{
    if (den < 1 || den > 1000000) return tcmi_fail(ctx, TCMI_E_ARG, "variants: the frequency's denominator %lld is outside 1..1000000", (long long)den);
    if (num < 0 || num > den) return tcmi_fail(ctx, TCMI_E_ARG, "variants: the frequency %lld / %lld is outside 0..1", (long long)num, (long long)den);
    if (min_alt_depth < 1) return tcmi_fail(ctx, TCMI_E_ARG, "variants: min_alt_depth %d is below 1", (int)min_alt_depth);
    if (min_depth < 0) return tcmi_fail(ctx, TCMI_E_ARG, "variants: min_depth %d is negative", (int)min_depth);
    out->num = num; out->den = den; out->min_alt_depth = min_alt_depth; out->min_depth = min_depth;
    return TCMI_OK;
}

// blk_cnt | blk_base of the table's launches for `blocks` workgroups, and the pinned words of the totals (grow-only; growing waits
// for the stream: nothing queued may still use the old scratch)
static int var_scratch(tcmi_ctx *ctx, int64_t blocks)
{
    tcmi_var_table &S = ctx->var;
    if (!S.h_tot) {
        TCMI_HIP(ctx, hipHostMalloc((void **)&S.h_tot, 64, hipHostMallocDefault));
        std::memset(S.h_tot, 0, 64);
    }
    if (blocks <= S.scr_blocks) return TCMI_OK;
    if (S.d_scr) { TCMI_HIP(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(S.d_scr); S.d_scr = nullptr; S.scr_blocks = 0; }
    TCMI_HIP(ctx, hipMalloc((void **)&S.d_scr, (size_t)blocks * 12 + 256));
    S.scr_blocks = blocks;
    return TCMI_OK;
}

static void var_job_scratch(tcmi_ctx *ctx, tcmi_var_job *j)
{   // (blk_base first: 8-byte words at the head of the allocation)
    j->blk_base = reinterpret_cast<unsigned long long *>(ctx->var.d_scr);
    j->blk_cnt = reinterpret_cast<uint32_t *>(ctx->var.d_scr + (size_t)ctx->var.scr_blocks * 8);
}

// a step's table: the context's matrix, reference and rule; records and total into the context's pinned memory
static int enqueue_variants(tcmi_ctx *ctx, int64_t L)
{
    const tcmi_var_table &V = ctx->var;
    if (std::min(L, V.n_ref) <= 0) return TCMI_OK;            // (a setting with an empty reference: nothing to launch, no record)
    tcmi_var_job j = {};
    var_job_scratch(ctx, &j);
    j.counts = ctx->d_counts; j.L = L; j.ld = ctx->ws_ld; j.ref = V.d_ref; j.n_ref = V.n_ref; j.rule = V.rule;
    j.total = V.h_tot; j.records = V.h_rec; j.cap = 5 * V.n_ref;
    return tcmi_launch_variants(ctx, j);
}

extern "C" {

int tcmi_variants_dev(tcmi_ctx *ctx, const void *d_counts, int64_t L, int64_t ld, const void *d_ref, int64_t n_ref, int64_t num, int64_t den,
                      int32_t min_alt_depth, int32_t min_depth, void *d_records, int64_t cap, int64_t *n_found)
{
    if (!ctx || !d_counts || !n_found) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    *n_found = 0;
    if (L <= 0 || ld < L) return tcmi_fail(ctx, TCMI_E_ARG, "need 0 < L <= ld");
    if (L > INT32_MAX - 1024) return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "L too large");
    if (n_ref < 0 || cap < 0 || (n_ref > 0 && !d_ref) || (cap > 0 && !d_records))
        return tcmi_fail(ctx, TCMI_E_ARG, "variants: negative size, or a size without its buffer (n_ref=%lld cap=%lld)", (long long)n_ref, (long long)cap);
    if (reinterpret_cast<uintptr_t>(d_counts) % 4 || reinterpret_cast<uintptr_t>(d_records) % 4)
        return tcmi_fail(ctx, TCMI_E_ARG, "d_counts and d_records must be aligned to 4 bytes");
    tcmi_var_job j = {};
    int rc = var_rule_build(ctx, num, den, min_alt_depth, min_depth, &j.rule);
    if (rc) return rc;
    const int64_t Lv = std::min(L, n_ref);
    if (Lv == 0) return TCMI_OK;                              // (no position has a reference base)
    TCMI_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t blocks = (Lv + 255) / 256;
    rc = var_scratch(ctx, blocks);
    if (rc) return rc;
    var_job_scratch(ctx, &j);
    j.counts = (const int32_t *)d_counts; j.L = L; j.ld = ld; j.ref = (const uint8_t *)d_ref; j.n_ref = n_ref;
    j.total = ctx->var.h_tot + 1; j.records = (tcmi_variant *)d_records; j.cap = cap;
    rc = tcmi_launch_variants(ctx, j);
    if (rc) return rc;
    TCMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_found = (int64_t)ctx->var.h_tot[1];
    if (*n_found > cap && (cap > 0 || d_records))
        return tcmi_fail(ctx, TCMI_E_ARG, "variants: %lld records, room for %lld (the first %lld were written)", (long long)*n_found, (long long)cap, (long long)cap);
    return TCMI_OK;
}

int tcmi_variants(tcmi_ctx *ctx, const int32_t *counts, int64_t L, const uint8_t *ref, int64_t n_ref, int64_t num, int64_t den,
                  int32_t min_alt_depth, int32_t min_depth, tcmi_variant *records, int64_t cap, int64_t *n_found)
{
    if (!ctx || !counts || !n_found) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    *n_found = 0;
    if (L <= 0) return tcmi_fail(ctx, TCMI_E_ARG, "L must be positive");
    if (n_ref < 0 || cap < 0 || (n_ref > 0 && !ref) || (cap > 0 && !records))
        return tcmi_fail(ctx, TCMI_E_ARG, "variants: negative size, or a size without its buffer (n_ref=%lld cap=%lld)", (long long)n_ref, (long long)cap);
    tcmi_var_rule rule;
    int rc = var_rule_build(ctx, num, den, min_alt_depth, min_depth, &rule);
    if (rc) return rc;
    rc = tcmi_ws_load_counts(ctx, counts, L);
    if (rc) return rc;
    const int64_t Lv = std::min(L, n_ref), room = std::min(cap, 5 * Lv);       // (5 per position: more than `room` records means more than cap)
    tcmi_dev_tmp d_ref, d_rec;
    if (Lv > 0) TCMI_HIP(ctx, d_ref.alloc((size_t)Lv));
    hipError_t e = Lv > 0 ? hipMemcpy(d_ref.p, ref, (size_t)Lv, hipMemcpyHostToDevice) : hipSuccess;
    if (e == hipSuccess && room > 0) e = d_rec.alloc((size_t)room * sizeof(tcmi_variant));
    if (e != hipSuccess) return tcmi_fail(ctx, TCMI_E_HIP, "variants: device buffers: %s", hipGetErrorString(e));
    rc = tcmi_variants_dev(ctx, ctx->d_counts, L, ctx->ws_ld, d_ref.p, Lv, num, den, min_alt_depth, min_depth, d_rec.p, room, n_found);
    if ((rc == TCMI_OK || (rc == TCMI_E_ARG && *n_found > room)) && room > 0) {      // (more records than room: the first `room` all the same)
        e = hipMemcpy(records, d_rec.p, (size_t)std::min(room, *n_found) * sizeof(tcmi_variant), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = tcmi_fail(ctx, TCMI_E_HIP, "variants: record download failed: %s", hipGetErrorString(e));
    }
    if (rc == TCMI_OK && *n_found > cap && (cap > 0 || records))
        return tcmi_fail(ctx, TCMI_E_ARG, "variants: %lld records, room for %lld", (long long)*n_found, (long long)cap);
    return rc;
}

int tcmi_ctx_set_variants(tcmi_ctx *c, const uint8_t *ref, int64_t n_ref, int64_t num, int64_t den, int32_t min_alt_depth, int32_t min_depth)
{
    if (!c) return tcmi_fail(nullptr, TCMI_E_ARG, "ctx is NULL");
    if (c->step_L > 0) return tcmi_fail(c, TCMI_E_ARG, "tcmi_ctx_set_variants between tcmi_step_begin and tcmi_step_end");
    if (!ref) { c->var.on = false; c->var.valid = false; return TCMI_OK; }       // (the buffers stay for the next setting)
    tcmi_var_rule rule;
    const int rc = var_rule_build(c, num, den, min_alt_depth, min_depth, &rule);
    if (rc) return rc;
    if (n_ref < 0 || n_ref > INT32_MAX - 1024) return tcmi_fail(c, TCMI_E_ARG, "variants: n_ref %lld is negative or too large", (long long)n_ref);
    TCMI_HIP(c, hipSetDevice(c->device));
    TCMI_HIP(c, hipStreamSynchronize(c->stream));             // (nothing queued may still read the reference or write the records)
    c->var.release();
    const int r2 = var_scratch(c, (n_ref + 255) / 256);
    if (r2) return r2;
    TCMI_HIP(c, hipMalloc((void **)&c->var.d_ref, (size_t)n_ref + 1));
    if (n_ref) TCMI_HIP(c, hipMemcpy(c->var.d_ref, ref, (size_t)n_ref, hipMemcpyHostToDevice));
    TCMI_HIP(c, hipHostMalloc((void **)&c->var.h_rec, (size_t)(5 * n_ref + 1) * sizeof(tcmi_variant), hipHostMallocDefault));
    c->var.n_ref = n_ref; c->var.rule = rule; c->var.on = true;
    return TCMI_OK;
}

int tcmi_step_variants(tcmi_ctx *c, const tcmi_variant **records, int64_t *n)
{
    if (!c || !records || !n) return tcmi_fail(c, TCMI_E_ARG, "null argument");
    *records = nullptr; *n = 0;
    if (c->step_L > 0) return tcmi_fail(c, TCMI_E_ARG, "tcmi_step_variants: the context's step has not been ended");
    if (!c->var.valid) return tcmi_fail(c, TCMI_E_ARG, "tcmi_step_variants: the last step computed no variant table (tcmi_ctx_set_variants)");
    *records = c->var.h_rec; *n = c->var.n;
    return TCMI_OK;
}

} // extern "C"

// ---- amplicon table (intervals.hip) --------------------------------------------------------------
static int iv_check(tcmi_ctx *ctx, int64_t n, const int64_t *start, const int64_t *end, int32_t min_depth)
{
    int64_t bad = -1;
    switch (tcmi_intervals_check(n, start, end, min_depth, &bad)) {
    case 0: return TCMI_OK;
    case 1: return tcmi_fail(ctx, TCMI_E_ARG, "intervals: n = %lld is outside 0..%d", (long long)n, (int)TCMI_IV_MAX_N);
    case 2: return tcmi_fail(ctx, TCMI_E_ARG, "intervals: min_depth %d is negative", (int)min_depth);
    case 3: return tcmi_fail(ctx, TCMI_E_ARG, "intervals: interval %lld, [%lld, %lld), does not satisfy 0 <= start <= end <= 2^29", (long long)bad,
                             (long long)start[bad], (long long)end[bad]);
    default: return tcmi_fail(ctx, TCMI_E_ARG, "intervals: n = %lld without both arrays", (long long)n);
    }
}

extern "C" {

int tcmi_interval_stats_dev(tcmi_ctx *ctx, const void *d_counts, int64_t L, int64_t ld, int64_t n, const void *d_start, const void *d_end,
                            int32_t min_depth, void *d_records)
{
    if (!ctx || !d_counts) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    if (L <= 0 || ld < L) return tcmi_fail(ctx, TCMI_E_ARG, "need 0 < L <= ld");
    if (L > INT32_MAX - 1024) return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "L too large");
    if (n < 0 || n > TCMI_IV_MAX_N) return tcmi_fail(ctx, TCMI_E_ARG, "intervals: n = %lld is outside 0..%d", (long long)n, (int)TCMI_IV_MAX_N);
    if (min_depth < 0) return tcmi_fail(ctx, TCMI_E_ARG, "intervals: min_depth %d is negative", (int)min_depth);
    if (n == 0) return TCMI_OK;
    if (!d_start || !d_end || !d_records) return tcmi_fail(ctx, TCMI_E_ARG, "intervals: n = %lld without its arrays", (long long)n);
    if (reinterpret_cast<uintptr_t>(d_counts) % 4 || reinterpret_cast<uintptr_t>(d_records) % 4)
        return tcmi_fail(ctx, TCMI_E_ARG, "d_counts and d_records must be aligned to 4 bytes");
    if (reinterpret_cast<uintptr_t>(d_start) % 8 || reinterpret_cast<uintptr_t>(d_end) % 8)
        return tcmi_fail(ctx, TCMI_E_ARG, "d_start and d_end must be aligned to 8 bytes");
    TCMI_HIP(ctx, hipSetDevice(ctx->device));
    // the kernel trusts its intervals: they are looked at here (16 bytes each; the call waits for the stream anyway)
    const std::unique_ptr<int64_t[]> se(new (std::nothrow) int64_t[(size_t)2 * n]);       // (no exception may cross the C ABI)
    if (!se) return tcmi_fail(ctx, TCMI_E_NOMEM, "intervals: no host memory for %lld intervals", (long long)n);
    TCMI_HIP(ctx, hipMemcpy(se.get(), d_start, (size_t)n * 8, hipMemcpyDeviceToHost));
    TCMI_HIP(ctx, hipMemcpy(se.get() + n, d_end, (size_t)n * 8, hipMemcpyDeviceToHost));
    int rc = iv_check(ctx, n, se.get(), se.get() + n, min_depth);
    if (rc) return rc;
    const tcmi_iv_job j = {(const int32_t *)d_counts, L, ld, n, (const int64_t *)d_start, (const int64_t *)d_end, min_depth, (tcmi_interval_stat *)d_records};
    rc = tcmi_launch_intervals(ctx, j);
    if (rc) return rc;
    TCMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TCMI_OK;
}

int tcmi_interval_stats(tcmi_ctx *ctx, const int32_t *counts, int64_t L, int64_t n, const int64_t *start, const int64_t *end,
                        int32_t min_depth, tcmi_interval_stat *records)
{
    if (!ctx || !counts) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    if (L <= 0) return tcmi_fail(ctx, TCMI_E_ARG, "L must be positive");
    int rc = iv_check(ctx, n, start, end, min_depth);
    if (rc) return rc;
    if (n == 0) return TCMI_OK;
    if (!records) return tcmi_fail(ctx, TCMI_E_ARG, "intervals: n = %lld without room for the records", (long long)n);
    rc = tcmi_ws_load_counts(ctx, counts, L);
    if (rc) return rc;
    tcmi_dev_tmp d_se, d_rec;
    TCMI_HIP(ctx, d_se.alloc((size_t)2 * n * 8));
    hipError_t e = hipMemcpy(d_se.p, start, (size_t)n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy((int64_t *)d_se.p + n, end, (size_t)n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = d_rec.alloc((size_t)n * sizeof(tcmi_interval_stat));
    if (e != hipSuccess) return tcmi_fail(ctx, TCMI_E_HIP, "intervals: device buffers: %s", hipGetErrorString(e));
    rc = tcmi_interval_stats_dev(ctx, ctx->d_counts, L, ctx->ws_ld, n, d_se.p, (int64_t *)d_se.p + n, min_depth, d_rec.p);
    if (rc) return rc;
    e = hipMemcpy(records, d_rec.p, (size_t)n * sizeof(tcmi_interval_stat), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return tcmi_fail(ctx, TCMI_E_HIP, "intervals: record download failed: %s", hipGetErrorString(e));
    return TCMI_OK;
}

int tcmi_ctx_set_intervals(tcmi_ctx *c, int64_t n, const int64_t *start, const int64_t *end, int32_t min_depth)
{
    if (!c) return tcmi_fail(nullptr, TCMI_E_ARG, "ctx is NULL");
    if (c->step_L > 0) return tcmi_fail(c, TCMI_E_ARG, "tcmi_ctx_set_intervals between tcmi_step_begin and tcmi_step_end");
    if (n == 0) { c->iv.on = false; c->iv.valid = false; return TCMI_OK; }       // (the buffers stay until the next setting or the end)
    const int rc = iv_check(c, n, start, end, min_depth);
    if (rc) return rc;
    TCMI_HIP(c, hipSetDevice(c->device));
    TCMI_HIP(c, hipStreamSynchronize(c->stream));             // (nothing queued may still read the intervals or write the records)
    c->iv.release();
    TCMI_HIP(c, hipMalloc((void **)&c->iv.d_iv, (size_t)2 * n * 8));
    TCMI_HIP(c, hipMemcpy(c->iv.d_iv, start, (size_t)n * 8, hipMemcpyHostToDevice));
    TCMI_HIP(c, hipMemcpy(c->iv.d_iv + n, end, (size_t)n * 8, hipMemcpyHostToDevice));
    TCMI_HIP(c, hipHostMalloc((void **)&c->iv.h_rec, (size_t)n * sizeof(tcmi_interval_stat), hipHostMallocDefault));
    c->iv.n = n; c->iv.min_depth = min_depth; c->iv.on = true;
    return TCMI_OK;
}

int tcmi_step_intervals(tcmi_ctx *c, const tcmi_interval_stat **records, int64_t *n)
{
    if (!c || !records || !n) return tcmi_fail(c, TCMI_E_ARG, "null argument");
    *records = nullptr; *n = 0;
    if (c->step_L > 0) return tcmi_fail(c, TCMI_E_ARG, "tcmi_step_intervals: the context's step has not been ended");
    if (!c->iv.valid) return tcmi_fail(c, TCMI_E_ARG, "tcmi_step_intervals: the last step computed no interval records (tcmi_ctx_set_intervals)");
    *records = c->iv.h_rec; *n = c->iv.n;
    return TCMI_OK;
}

} // extern "C"

// ---- the tables' slot in a step (step.cpp) -----------------------------------------------------------
int tcmi_tables_enqueue(tcmi_ctx *ctx, int64_t L)
{
    if (ctx->var.on) {              // the variant table: behind the tally, in front of the call kernel, which may zero the matrix
        const int rc = enqueue_variants(ctx, L);
        if (rc) return rc;
    }
    if (!ctx->iv.on) return TCMI_OK;                            // the amplicon table: the same slot (both only read the matrix)
    const tcmi_iv_table &I = ctx->iv;
    const tcmi_iv_job j = {ctx->d_counts, L, ctx->ws_ld, I.n, I.d_iv, I.d_iv + I.n, I.min_depth, I.h_rec};
    return tcmi_launch_intervals(ctx, j);
}

void tcmi_tables_step_begin(tcmi_ctx *ctx, bool ride_along)
{
    ctx->var.in_step = !ride_along && ctx->var.on;
    ctx->iv.in_step = !ride_along && ctx->iv.on;
}

void tcmi_tables_step_end(tcmi_ctx *ctx)
{
    tcmi_var_table &V = ctx->var;
    V.valid = V.in_step;
    ctx->iv.valid = ctx->iv.in_step;
    if (V.in_step) V.n = std::min(ctx->step_L, V.n_ref) > 0 ? (int64_t)V.h_tot[0] : 0;
}

void tcmi_tables_release(tcmi_ctx *ctx)
{
    tcmi_var_table &V = ctx->var;
    V.release();
    if (V.d_scr) (void)hipFree(V.d_scr);
    if (V.h_tot) (void)hipHostFree(V.h_tot);
    V.d_scr = nullptr; V.h_tot = nullptr; V.scr_blocks = 0;
    ctx->iv.release();
}

bool tcmi_var_table_on(const tcmi_ctx *ctx) { return ctx->var.on; }
bool tcmi_iv_table_on(const tcmi_ctx *ctx) { return ctx->iv.on; }
int64_t tcmi_iv_table_n(const tcmi_ctx *ctx) { return ctx->iv.n; }
