// api.cpp — context, its settings and workspace, error text, profiling brackets and the tally / call / counts host-buffer
// conveniences of the C ABI declared in include/tcmi.h.  The per-step tables: tables.cpp; a step: step.cpp; tcmi_split_step: split_step.cpp.
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <string>
#include <memory>
#include <thread>

#include "tcmi_internal.h"
#include "primer_table.h"

static thread_local std::string g_err;

void *tcmi_ctx_pinned(tcmi_ctx *ctx, size_t bytes)
{
    if (ctx->h_pin_cap < bytes) {
        if (ctx->h_pin) { (void)hipStreamSynchronize(ctx->stream); (void)hipHostFree(ctx->h_pin); ctx->h_pin = nullptr; ctx->h_pin_cap = 0; }
        const size_t want = bytes + bytes / 2 + 4096;
        if (hipHostMalloc((void **)&ctx->h_pin, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); ctx->h_pin = nullptr; return nullptr; }
        ctx->h_pin_cap = want;
    }
    return ctx->h_pin;
}

int tcmi_arena_reserve(tcmi_ctx *ctx, size_t bytes)
{
    tcmi_dev_arena &A = ctx->dev_arena;
    A.used = 0;
    ++ctx->arena_epoch;                         // whatever lived in the arena is gone
    if (A.cap >= bytes) return TCMI_OK;
    if (A.base) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(A.base); A.base = nullptr; A.cap = 0; }
    const size_t want = bytes + bytes / 8 + (1 << 20);
    if (hipMalloc((void **)&A.base, want) != hipSuccess) return tcmi_fail(ctx, TCMI_E_NOMEM, "hipMalloc(%zu) for the pack scratch failed", want);
    A.cap = want;
    return TCMI_OK;
}

void *tcmi_arena_take(tcmi_ctx *ctx, size_t bytes)
{
    tcmi_dev_arena &A = ctx->dev_arena;
    const size_t at = tcmi_align256(A.used);
    A.used = at + bytes;
    return A.base + at;
}

int tcmi_fail(tcmi_ctx *ctx, int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    if (ctx) ctx->err = buf;
    return code;
}

// ---- the workspace of tcmi_step and the host-buffer conveniences --------------------------------
static void free_ws(tcmi_ctx *c)
{
    if (c->d_counts) (void)hipFree(c->d_counts);
    if (c->d_plain) (void)hipFree(c->d_plain);
    if (c->h_rec) (void)hipHostFree(c->h_rec);
    if (c->h_counts) (void)hipHostFree(c->h_counts);
    c->d_counts = nullptr;
    c->d_plain = c->d_alt = c->d_flags = nullptr;
    c->h_rec = nullptr;
    c->h_counts = nullptr;
    c->ws_L = c->ws_ld = 0;
}

int tcmi_ws_ensure(tcmi_ctx *ctx, int64_t L)
{
    if (ctx->ws_L >= L && ctx->d_counts) return TCMI_OK;
    free_ws(ctx);
    ctx->counts_clean = false;
    int64_t ld = tcmi_round_up(L, 256);
    TCMI_HIP(ctx, hipMalloc((void **)&ctx->d_counts, (size_t)ld * TCMI_NCOL * 4 + 256));
    TCMI_HIP(ctx, hipMalloc((void **)&ctx->d_plain, (size_t)ld * 3));
    ctx->d_alt = ctx->d_plain + ld;
    ctx->d_flags = ctx->d_plain + 2 * ld;
    TCMI_HIP(ctx, hipHostMalloc((void **)&ctx->h_rec, (size_t)ld * 3, hipHostMallocDefault));
    TCMI_HIP(ctx, hipHostMalloc((void **)&ctx->h_counts, (size_t)ld * TCMI_NCOL * 4 + 256, hipHostMallocDefault));
    ctx->ws_L = L;
    ctx->ws_ld = ld;
    return TCMI_OK;
}

int tcmi_ws_load_counts(tcmi_ctx *ctx, const int32_t *counts, int64_t L)
{
    const int rc = tcmi_ws_ensure(ctx, L);
    if (rc) return rc;
    ctx->counts_clean = false;
    return tcmi_counts_upload(ctx, counts, L, ctx->ws_ld, ctx->d_counts);
}

// everything a context owns, and the context: tcmi_ctx_destroy, and ctx_create's way out of a context that was built only in part
// (whatever was not made yet is null)
static void ctx_release(tcmi_ctx *c)
{
    (void)hipSetDevice(c->device);
    if (c->stream || !c->own_stream) (void)hipStreamSynchronize(c->stream);      // (a caller's stream may be the null stream)
    for (tcmi_ctx *h : c->helpers) (void)tcmi_ctx_destroy(h);
    for (auto &p : c->pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    free_ws(c);
    tcmi_host_packed_free(c->host_packed);
    if (c->dev_arena.base) (void)hipFree(c->dev_arena.base);
    if (c->d_lay) (void)hipFree(c->d_lay);
    for (auto &b : c->blob_pool) (void)hipFree(b.p);
    if (c->tok_dev) (void)hipFree(c->tok_dev);
    if (c->tok_host) (void)hipHostFree(c->tok_host);
    if (c->count_dev) (void)hipFree(c->count_dev);
    if (c->h_pin) (void)hipHostFree(c->h_pin);
    if (c->h_desc) (void)hipHostFree(c->h_desc);
    tcmi_tables_release(c);
    if (c->step_done) (void)hipEventDestroy(c->step_done);
    if (c->ev_after_sym) (void)hipEventDestroy(c->ev_after_sym);
    if (c->copy_stream) { (void)hipStreamSynchronize(c->copy_stream); (void)hipStreamDestroy(c->copy_stream); }
    for (hipEvent_t e : c->ev_piece) (void)hipEventDestroy(e);
    if (c->stream_hi) { (void)hipStreamSynchronize(c->stream_hi); (void)hipStreamDestroy(c->stream_hi); }
    if (c->ev_split) (void)hipEventDestroy(c->ev_split);
    if (c->stream_lo) c->stream = c->stream_lo;                  // (`stream` is one of the two, whichever the launches use at the moment)
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

static int ctx_create(int device, bool own, void *stream, tcmi_ctx **out)
{
    if (!out) return tcmi_fail(nullptr, TCMI_E_ARG, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return tcmi_fail(nullptr, TCMI_E_NODEVICE,
                         "no HIP device available (%s); libtcmi has no CPU path",
                         e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    }
    if (device < 0 || device >= n)
        return tcmi_fail(nullptr, TCMI_E_ARG, "device %d out of range (%d devices)", device, n);
    if (hipSetDevice(device) != hipSuccess)
        return tcmi_fail(nullptr, TCMI_E_NODEVICE, "hipSetDevice(%d) failed", device);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess)
        return tcmi_fail(nullptr, TCMI_E_NODEVICE, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return tcmi_fail(nullptr, TCMI_E_NODEVICE, "device %d is %s; libtcmi is built for gfx950 only",
                         device, prop.gcnArchName);
    tcmi_ctx *c = new tcmi_ctx();
    c->device = device;
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    // TCMI_STREAM_SPLIT (A/B): 1 = two streams by priority (inflate low, pack + tally + call high); 2 = by compute units
    // (TCMI_CU_HI of them, default 48, for the high stream, the rest for the inflate); 3 = inflate on its share of the compute units,
    // the rest at high priority on all of them
    const char *sv = std::getenv("TCMI_STREAM_SPLIT");
    const int split = sv ? std::atoi(sv) : 0;
    if (!own) {
        c->stream = (hipStream_t)stream;
        c->own_stream = false;
    } else if (split >= 1 && split <= 3) {
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        const char *hv = std::getenv("TCMI_CU_HI");
        const int n_hi = std::max(1, std::min(c->n_cu - 1, hv ? std::atoi(hv) : 48));
        uint32_t m_lo[16] = {0}, m_hi[16] = {0};
        for (int i = 0; i < c->n_cu && i < 512; ++i) (i < c->n_cu - n_hi ? m_lo : m_hi)[i >> 5] |= 1u << (i & 31);
        const uint32_t words = (uint32_t)((c->n_cu + 31) / 32);
        hipError_t e1, e2;
        if (split == 1) {
            e1 = hipStreamCreateWithPriority(&c->stream_lo, hipStreamNonBlocking, least);
            e2 = hipStreamCreateWithPriority(&c->stream_hi, hipStreamNonBlocking, greatest);
        } else if (split == 2) {
            e1 = hipExtStreamCreateWithCUMask(&c->stream_lo, words, m_lo);
            e2 = hipExtStreamCreateWithCUMask(&c->stream_hi, words, m_hi);
        } else {
            e1 = hipExtStreamCreateWithCUMask(&c->stream_lo, words, m_lo);
            e2 = hipStreamCreateWithPriority(&c->stream_hi, hipStreamNonBlocking, greatest);
        }
        if (e1 != hipSuccess || e2 != hipSuccess || hipEventCreateWithFlags(&c->ev_split, hipEventDisableTiming) != hipSuccess) {
            const hipError_t e = e1 != hipSuccess ? e1 : e2;
            ctx_release(c);
            return tcmi_fail(nullptr, TCMI_E_HIP, "TCMI_STREAM_SPLIT=%d: the streams could not be made (%s)", split, hipGetErrorString(e));
        }
        c->stream = c->stream_lo;
    } else if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        ctx_release(c);
        return tcmi_fail(nullptr, TCMI_E_HIP, "hipStreamCreate failed");
    }
    if (hipEventCreateWithFlags(&c->step_done, hipEventDisableTiming) != hipSuccess) {
        ctx_release(c);
        return tcmi_fail(nullptr, TCMI_E_HIP, "hipEventCreate failed");
    }
    const char *v = std::getenv("TCMI_TALLY_VARIANT");
    if (v) c->tally_variant = std::atoi(v);
    v = std::getenv("TCMI_ROUNDS_PER_WG");
    if (v) c->rounds_per_wg = std::atoi(v);
    {
        const unsigned hc = std::thread::hardware_concurrency();
        c->host_threads = hc ? (int)std::min(hc, 16u) : 4;
    }
    v = std::getenv("TCMI_HOST_THREADS");
    if (v && std::atoi(v) >= 1) c->host_threads = std::atoi(v);
    if (std::getenv("TCMI_NO_FUSED")) c->one_sync = 0;          // (A/B measurements)
    v = std::getenv("TCMI_CHUNK_STAGES");
    if (v && std::atoi(v) >= 1 && std::atoi(v) <= TCMI_F_MAXSTAGE) c->chunk_stages = std::atoi(v);

    *out = c;
    return TCMI_OK;
}

extern "C" {

int tcmi_abi_version(void) { return TCMI_ABI_VERSION; }

const char *tcmi_last_error(const tcmi_ctx *ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int tcmi_device_count(int *out_count)
{
    if (!out_count) return tcmi_fail(nullptr, TCMI_E_ARG, "out_count is NULL");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    (void)hipGetLastError();
    *out_count = n;
    return TCMI_OK;
}

int tcmi_ctx_create(int device, tcmi_ctx **out) { return ctx_create(device, true, nullptr, out); }

// stream may be NULL: the device's default (null) stream, e.g. torch's default current stream
int tcmi_ctx_create_on_stream(int device, void *stream, tcmi_ctx **out) { return ctx_create(device, false, stream, out); }

int tcmi_ctx_destroy(tcmi_ctx *c)
{
    if (c) ctx_release(c);
    return TCMI_OK;
}

int tcmi_ctx_sync(tcmi_ctx *c)
{
    if (!c) return tcmi_fail(nullptr, TCMI_E_ARG, "ctx is NULL");
    TCMI_HIP(c, hipStreamSynchronize(c->stream));
    if (c->stream_hi) TCMI_HIP(c, hipStreamSynchronize(c->stream_hi));
    return TCMI_OK;
}

void *tcmi_ctx_stream(tcmi_ctx *c) { return c ? (void *)c->stream : nullptr; }

int tcmi_ctx_set_option(tcmi_ctx *c, const char *key, int value)
{
    if (!c || !key) return tcmi_fail(c, TCMI_E_ARG, "null argument");
    if (!std::strcmp(key, "tally_variant")) c->tally_variant = value;
    else if (!std::strcmp(key, "rounds_per_wg")) c->rounds_per_wg = value;
    else if (!std::strcmp(key, "host_threads")) c->host_threads = value < 1 ? 1 : value;
    else if (!std::strcmp(key, "chunk_stages")) c->chunk_stages = value < 0 ? 0 : value > TCMI_F_MAXSTAGE ? TCMI_F_MAXSTAGE : value;
    else if (!std::strcmp(key, "defer_call")) c->defer_call = value != 0;
    else if (!std::strcmp(key, "wg_per_cu")) c->wg_per_cu = value < 1 ? 1 : value;
    else if (!std::strcmp(key, "stage_cap")) c->stage_cap = value < 0 ? 0 : value;
    else if (!std::strcmp(key, "balance_chunks")) c->balance_chunks = value != 0;
    else if (!std::strcmp(key, "project_reads")) c->project_reads = value != 0;
    else if (!std::strcmp(key, "device_pack")) c->device_pack = value != 0;
    else if (!std::strcmp(key, "verify_crc")) c->verify_crc = value != 0;
    else if (!std::strcmp(key, "one_sync")) c->one_sync = value != 0;
    else if (!std::strcmp(key, "mid_wait")) c->mid_wait = value != 0;
    else if (!std::strcmp(key, "prefix_kernels")) c->prefix_kernels = value;
    else if (!std::strcmp(key, "decode_token_mb")) c->decode_token_mb = value > 0 ? value : 4096;
    else if (!std::strcmp(key, "profile_every")) c->prof_every = value < 1 ? 1 : value;
    else if (!std::strcmp(key, "sym_scratch_div")) c->sym_scratch_div = value < 1 ? 1 : value > 64 ? 64 : value;
    else if (!std::strcmp(key, "h2d_pieces")) c->h2d_pieces = value < -1 ? -1 : value > 16 ? 16 : value;
    else if (!std::strcmp(key, "split_sub")) c->split_sub = value < 0 ? 0 : value > 8 ? 8 : value;
    else if (!std::strcmp(key, "indel_slots")) c->indel_slots = value < 4 ? 4 : value > 24 ? 24 : value;
    else if (!std::strcmp(key, "indel_hash_bits")) c->indel_hash_bits = value < 0 ? 0 : value > 34 ? 34 : value;

    else return tcmi_fail(c, TCMI_E_ARG, "unknown option %s", key);
    return TCMI_OK;
}

} // extern "C"

int tcmi_read_filter_build(tcmi_ctx *ctx, int32_t min_mapq, uint32_t require_flags, uint32_t exclude_flags, tcmi_read_filter *out)
{
    if (min_mapq < 0 || min_mapq > 255) return tcmi_fail(ctx, TCMI_E_ARG, "read filter: min_mapq %d is outside 0..255", (int)min_mapq);
    if (require_flags > 0xFFFFu || exclude_flags > 0xFFFFu)
        return tcmi_fail(ctx, TCMI_E_ARG, "read filter: flag words 0x%x / 0x%x do not fit the 16 bits of a BAM FLAG", require_flags, exclude_flags);
    out->min_mapq = (uint32_t)min_mapq; out->require = require_flags; out->exclude = exclude_flags;
    return TCMI_OK;
}

int tcmi_layout_build(int32_t n_ref, const int64_t *shift, const int64_t *slot_len, tcmi_layout *out, char *msg, size_t msg_cap)
{
    out->shift.clear(); out->end.clear();
    if (n_ref < 0 || (n_ref > 0 && (!shift || !slot_len))) { std::snprintf(msg, msg_cap, "bad layout arguments"); return TCMI_E_ARG; }
    int64_t prev_end = 0;
    for (int32_t t = 0; t < n_ref; ++t) {
        if (shift[t] < 0) continue;                                 // (a reference whose reads are dropped)
        if (slot_len[t] < 1 || shift[t] < prev_end || shift[t] + slot_len[t] > (int64_t)TCMI_F_EVPOS) {
            std::snprintf(msg, msg_cap, "layout: slot %d [%lld, +%lld) overlaps the slot in front, is empty or ends beyond 2^29", t,
                          (long long)shift[t], (long long)slot_len[t]);
            return TCMI_E_ARG;
        }
        prev_end = shift[t] + slot_len[t];
    }
    out->shift.assign(shift, shift + n_ref);
    out->end.resize((size_t)n_ref);
    for (int32_t t = 0; t < n_ref; ++t) out->end[(size_t)t] = shift[t] < 0 ? -1 : shift[t] + slot_len[t];
    return TCMI_OK;
}

extern "C" {

int tcmi_ctx_set_layout(tcmi_ctx *c, int32_t n_ref, const int64_t *shift, const int64_t *slot_len)
{
    if (!c) return tcmi_fail(nullptr, TCMI_E_ARG, "ctx is NULL");
    char msg[200];
    tcmi_layout L;
    const int rc = tcmi_layout_build(n_ref, shift, slot_len, &L, msg, sizeof msg);
    if (rc) return tcmi_fail(c, rc, "%s", msg);
    if (n_ref > 0) {
        std::vector<int32_t> h((size_t)n_ref * 2);
        for (int32_t t = 0; t < n_ref; ++t) { h[(size_t)t] = (int32_t)L.shift_of(t); h[(size_t)(n_ref + t)] = (int32_t)L.end[(size_t)t]; }
        TCMI_HIP(c, hipSetDevice(c->device));
        TCMI_HIP(c, hipStreamSynchronize(c->stream));      // (nothing queued may still read the table that is rewritten)
        const size_t need = (size_t)n_ref * 3 * 4;
        if (need > c->d_lay_cap) {
            if (c->d_lay) (void)hipFree(c->d_lay);
            c->d_lay = nullptr; c->d_lay_cap = 0;
            TCMI_HIP(c, hipMalloc((void **)&c->d_lay, need));
            c->d_lay_cap = need;
        }
        TCMI_HIP(c, hipMemcpy(c->d_lay, h.data(), h.size() * 4, hipMemcpyHostToDevice));
        ++c->lay_gen;                                        // (clearing the layout leaves the table as it is)
    }
    c->layout = std::move(L);
    return TCMI_OK;
}

int tcmi_ctx_set_read_filter(tcmi_ctx *c, int32_t min_mapq, uint32_t require_flags, uint32_t exclude_flags)
{
    if (!c) return tcmi_fail(nullptr, TCMI_E_ARG, "ctx is NULL");
    tcmi_read_filter f = {0, 0, 0};
    const int rc = tcmi_read_filter_build(c, min_mapq, require_flags, exclude_flags, &f);
    if (rc) return rc;
    c->rules.flt = f;                                                 // (a kernel argument of the next upload: nothing queued reads it)
    return TCMI_OK;
}

int tcmi_ctx_set_min_base_quality(tcmi_ctx *c, int32_t q)
{
    if (!c) return tcmi_fail(nullptr, TCMI_E_ARG, "ctx is NULL");
    if (q < 0 || q > 255) return tcmi_fail(c, TCMI_E_ARG, "min_base_quality %d is outside 0..255", (int)q);
    c->rules.min_bq = q;                                              // (a kernel argument of the next upload: nothing queued reads it)
    return TCMI_OK;
}

int tcmi_ctx_set_mate_overlap(tcmi_ctx *c, int32_t on)
{
    if (!c) return tcmi_fail(nullptr, TCMI_E_ARG, "ctx is NULL");
    if (on != 0 && on != 1) return tcmi_fail(c, TCMI_E_ARG, "mate_overlap %d is neither 0 nor 1", (int)on);
    c->rules.mate = on;                                       // (read by the next upload: nothing queued reads it)
    return TCMI_OK;
}

int tcmi_ctx_set_dedup(tcmi_ctx *c, int32_t on)
{
    if (!c) return tcmi_fail(nullptr, TCMI_E_ARG, "ctx is NULL");
    if (on != 0 && on != 1) return tcmi_fail(c, TCMI_E_ARG, "dedup %d is neither 0 nor 1", (int)on);
    c->rules.dedup = on;                                      // (read by the next upload: nothing queued reads it)
    return TCMI_OK;
}

int tcmi_ctx_set_primers(tcmi_ctx *c, int32_t n, const int64_t *start, const int64_t *end, const int32_t *reverse, int32_t slack)
{
    if (!c) return tcmi_fail(nullptr, TCMI_E_ARG, "ctx is NULL");
    std::vector<tcmi_pseg> head, tail;
    char msg[200] = "";
    if (tcmi_primers_build(n, start, end, reverse, slack, head, tail, msg, sizeof msg)) return tcmi_fail(c, TCMI_E_ARG, "%s", msg);
    if (n == 0) { c->rules.primers.reset(); return TCMI_OK; }         // (read sets built under the old table keep their share of it)
    // a table of its own for every call: nothing queued, and no read set, ever sees one rewritten
    std::vector<int32_t> h(3 * (head.size() + tail.size()) + 1);
    int32_t *hh = h.data(), *ht = h.data() + 3 * head.size();
    for (size_t i = 0; i < head.size(); ++i) { hh[i] = head[i].a; hh[head.size() + i] = head[i].b; hh[2 * head.size() + i] = head[i].v; }
    for (size_t i = 0; i < tail.size(); ++i) { ht[i] = tail[i].a; ht[tail.size() + i] = tail[i].b; ht[2 * tail.size() + i] = tail[i].v; }
    TCMI_HIP(c, hipSetDevice(c->device));
    std::shared_ptr<tcmi_primer_dev> dev = std::make_shared<tcmi_primer_dev>();
    TCMI_HIP(c, hipMalloc((void **)&dev->seg, h.size() * 4));
    TCMI_HIP(c, hipMemcpy(dev->seg, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    dev->n_head = (int32_t)head.size(); dev->n_tail = (int32_t)tail.size(); dev->n_primers = n;
    c->rules.primers = std::move(dev);                                // (a kernel argument of the next upload)
    return TCMI_OK;
}

int tcmi_ctx_stat(tcmi_ctx *c, const char *key, int64_t *value)
{
    if (!c || !key || !value) return tcmi_fail(c, TCMI_E_ARG, "null argument");
    if (!std::strcmp(key, "one_sync_taken")) { *value = c->stat_one_sync_taken; for (const tcmi_ctx *h : c->helpers) *value += h->stat_one_sync_taken; }
    else if (!std::strcmp(key, "one_sync_declined")) *value = c->stat_one_sync_declined;
    else if (!std::strcmp(key, "one_sync_retried")) { *value = c->stat_one_sync_retried; for (const tcmi_ctx *h : c->helpers) *value += h->stat_one_sync_retried; }
    else if (!std::strcmp(key, "decode_batched")) { *value = c->stat_decode_batched; for (const tcmi_ctx *h : c->helpers) *value += h->stat_decode_batched; }
    else if (!std::strcmp(key, "split_sub_taken")) *value = c->stat_split_sub;
    else if (!std::strcmp(key, "indel_table_grown")) *value = c->stat_indel_grown;
    else if (!std::strcmp(key, "indel_hash_retried")) *value = c->stat_indel_retried;
    else if (!std::strcmp(key, "h2d_piped")) { *value = c->stat_h2d_piped; for (const tcmi_ctx *h : c->helpers) *value += h->stat_h2d_piped; }
    else if (!std::strcmp(key, "one_sync_last_decline_flags")) *value = c->stat_last_decline;
    else if (!std::strcmp(key, "compute_units")) *value = c->n_cu;
    else if (!std::strcmp(key, "mate_pairs")) *value = c->stat_mate[0];
    else if (!std::strcmp(key, "mate_clipped_reads")) *value = c->stat_mate[1];
    else if (!std::strcmp(key, "mate_clipped_columns")) *value = c->stat_mate[2];
    else if (!std::strcmp(key, "mate_ambiguous")) *value = c->stat_mate[3];
    else if (!std::strcmp(key, "dedup_templates")) *value = c->stat_dup[0];
    else if (!std::strcmp(key, "duplicate_templates")) *value = c->stat_dup[1];
    else if (!std::strcmp(key, "duplicate_records")) *value = c->stat_dup[2];
    else if (!std::strcmp(key, "duplicate_sets")) *value = c->stat_dup[3];
    else return tcmi_fail(c, TCMI_E_ARG, "unknown statistic %s", key);
    return TCMI_OK;
}

// ---- profiling -------------------------------------------------------------------------
int tcmi_profile_enable(tcmi_ctx *c, int on)
{
    if (!c) return tcmi_fail(nullptr, TCMI_E_ARG, "ctx is NULL");
    c->prof = on != 0;
    return TCMI_OK;
}

static int drain(tcmi_ctx *c)
{
    for (auto &p : c->pending) {
        TCMI_HIP(c, hipEventSynchronize(p.b));
        float ms = 0.f;
        TCMI_HIP(c, hipEventElapsedTime(&ms, p.a, p.b));
        c->prof_ms[p.k] += ms;
        c->prof_n[p.k] += 1;
        c->ev_pool.push_back(p.a);
        c->ev_pool.push_back(p.b);
    }
    c->pending.clear();
    return TCMI_OK;
}

int tcmi_profile_reset(tcmi_ctx *c)
{
    if (!c) return tcmi_fail(nullptr, TCMI_E_ARG, "ctx is NULL");
    int rc = drain(c);
    for (int k = 0; k < TCMI_K_NKERNELS; ++k) { c->prof_ms[k] = 0; c->prof_n[k] = 0; }
    return rc;
}

int tcmi_profile_get(tcmi_ctx *c, int k, double *total_ms, int64_t *launches)
{
    if (!c || k < 0 || k >= TCMI_K_NKERNELS) return tcmi_fail(c, TCMI_E_ARG, "bad kernel id");
    int rc = drain(c);
    if (rc) return rc;
    if (total_ms) *total_ms = c->prof_ms[k];
    if (launches) *launches = c->prof_n[k];
    return TCMI_OK;
}

} // extern "C"

static hipEvent_t get_event(tcmi_ctx *c)
{
    if (!c->ev_pool.empty()) { hipEvent_t e = c->ev_pool.back(); c->ev_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

// recycle the events of launches that have finished, so a long profiled run does not keep
// creating events (hipEventCreate is far more expensive than hipEventRecord)
static void reap(tcmi_ctx *c)
{
    size_t done = 0;
    while (done < c->pending.size() && hipEventQuery(c->pending[done].b) == hipSuccess) {
        auto &p = c->pending[done];
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { c->prof_ms[p.k] += ms; c->prof_n[p.k] += 1; }
        c->ev_pool.push_back(p.a);
        c->ev_pool.push_back(p.b);
        ++done;
    }
    (void)hipGetLastError();                                 // hipErrorNotReady from the query is expected
    if (done) c->pending.erase(c->pending.begin(), c->pending.begin() + (long)done);
}

void tcmi_prof_begin(tcmi_ctx *c, int k)
{
    c->prof_open = false;
    if (!c->prof || c->prof_mute) return;
    c->prof_open = true;
    if (c->pending.size() >= 24) reap(c);
    tcmi_ctx::Pending p{k, get_event(c), get_event(c)};
    (void)hipEventRecord(p.a, c->stream);
    c->pending.push_back(p);
}

void tcmi_prof_end(tcmi_ctx *c, int k)
{
    if (!c->prof || !c->prof_open || c->pending.empty()) return;
    c->prof_open = false;
    (void)k;
    (void)hipEventRecord(c->pending.back().b, c->stream);
}

extern "C" {

// ---- tally -----------------------------------------------------------------------------------
int tcmi_tally_dev(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t L, int64_t ld, void *d_counts, int zero)
{
    if (!ctx || !rs || !d_counts) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    if (L <= 0 || ld < L) return tcmi_fail(ctx, TCMI_E_ARG, "need 0 < L <= ld (L=%lld ld=%lld)", (long long)L, (long long)ld);
    if (reinterpret_cast<uintptr_t>(d_counts) % 4) return tcmi_fail(ctx, TCMI_E_ARG, "d_counts must be aligned to 4 bytes");
    if (L > INT32_MAX - 1024) return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "L too large");
    if (rs->device != ctx->device) return tcmi_fail(ctx, TCMI_E_ARG, "read set lives on device %d, context on %d", rs->device, ctx->device);
    if (rs->max_end > L)
        return tcmi_fail(ctx, TCMI_E_ARG, "L=%lld is smaller than the read extent %lld (use tcmi_reads_extent)",
                         (long long)L, (long long)rs->max_end);
    TCMI_HIP(ctx, hipSetDevice(ctx->device));
    if (!rs->parts.empty()) {                                   // a read set of sub-ranges: every part adds its counts from its own context
        if (zero) {
            TCMI_HIP(ctx, hipMemsetAsync(d_counts, 0, (size_t)ld * TCMI_NCOL * 4, ctx->stream));
            TCMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        for (const tcmi_readset::Part &p : rs->parts) {
            const int rc = tcmi_tally_dev(p.cx, p.rs, L, ld, d_counts, 0);
            if (rc) return tcmi_fail(ctx, rc, "%s", p.cx->err.c_str());
            TCMI_HIP(ctx, hipStreamSynchronize(p.cx->stream));
        }
        return TCMI_OK;
    }
    if (zero) {
        tcmi_prof_begin(ctx, TCMI_K_ZERO);
        TCMI_HIP(ctx, hipMemsetAsync(d_counts, 0, (size_t)ld * TCMI_NCOL * 4, ctx->stream));
        tcmi_prof_end(ctx, TCMI_K_ZERO);
    }
    if (rs->n_piled == 0) return TCMI_OK;
    return tcmi_launch_tally(ctx, rs, L, ld, (int32_t *)d_counts);
}

int tcmi_counts_download(tcmi_ctx *ctx, const void *d_counts, int64_t L, int64_t ld, int32_t *counts)
{
    if (!ctx || !d_counts || !counts || L <= 0 || ld < L) return tcmi_fail(ctx, TCMI_E_ARG, "bad argument");
    TCMI_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<int32_t> planes((size_t)ld * TCMI_NCOL);
    TCMI_HIP(ctx, hipMemcpyAsync(planes.data(), d_counts, planes.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    TCMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int c = 0; c < TCMI_NCOL; ++c) {
        const int32_t *src = planes.data() + (size_t)c * ld;
        for (int64_t p = 0; p < L; ++p) counts[p * TCMI_NCOL + c] = src[p];
    }
    return TCMI_OK;
}

int tcmi_counts_upload(tcmi_ctx *ctx, const int32_t *counts, int64_t L, int64_t ld, void *d_counts)
{
    if (!ctx || !d_counts || !counts || L <= 0 || ld < L) return tcmi_fail(ctx, TCMI_E_ARG, "bad argument");
    TCMI_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<int32_t> planes((size_t)ld * TCMI_NCOL, 0);
    for (int c = 0; c < TCMI_NCOL; ++c)
        for (int64_t p = 0; p < L; ++p) planes[(size_t)c * ld + p] = counts[p * TCMI_NCOL + c];
    TCMI_HIP(ctx, hipMemcpyAsync(d_counts, planes.data(), planes.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    TCMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TCMI_OK;
}

int tcmi_tally(tcmi_ctx *ctx, const tcmi_reads *reads, int64_t L, int32_t *counts)
{
    if (!ctx || !counts) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    if (L <= 0) return tcmi_fail(ctx, TCMI_E_ARG, "L must be positive");
    tcmi_readset *rs = nullptr;
    int rc = tcmi_readset_upload(ctx, reads, &rs);
    if (rc) return rc;
    if (rs->max_end > L) {
        tcmi_readset_free(ctx, rs);
        return tcmi_fail(ctx, TCMI_E_ARG, "L=%lld is smaller than the read extent %lld (use tcmi_reads_extent)",
                         (long long)L, (long long)rs->max_end);
    }
    rc = tcmi_ws_ensure(ctx, L);
    ctx->counts_clean = false;
    if (!rc) rc = tcmi_tally_dev(ctx, rs, L, ctx->ws_ld, ctx->d_counts, 1);
    if (!rc) rc = tcmi_counts_download(ctx, ctx->d_counts, L, ctx->ws_ld, counts);
    tcmi_readset_free(ctx, rs);
    return rc;
}

// ---- call ------------------------------------------------------------------------------------
int tcmi_call_dev(tcmi_ctx *ctx, const void *d_counts, int64_t L, int64_t ld, int32_t mincov, int include_ambig,
                  void *d_plain, void *d_alt, void *d_flags, void *d_events, void *d_event_counts)
{
    if (!ctx || !d_counts || !d_plain || !d_alt || !d_flags) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    if (L <= 0 || ld < L) return tcmi_fail(ctx, TCMI_E_ARG, "need 0 < L <= ld");
    if ((d_events == nullptr) != (d_event_counts == nullptr))
        return tcmi_fail(ctx, TCMI_E_ARG, "d_events and d_event_counts must both be given or both NULL");
    if (reinterpret_cast<uintptr_t>(d_counts) % 4 || reinterpret_cast<uintptr_t>(d_events) % 4 || reinterpret_cast<uintptr_t>(d_event_counts) % 4)
        return tcmi_fail(ctx, TCMI_E_ARG, "d_counts, d_events and d_event_counts must be aligned to 4 bytes");
    TCMI_HIP(ctx, hipSetDevice(ctx->device));
    return tcmi_launch_call(ctx, (int32_t *)const_cast<void *>(d_counts), L, ld, mincov, include_ambig, 0, (uint8_t *)d_plain,
                            (uint8_t *)d_alt, (uint8_t *)d_flags, (int32_t *)d_events, (int32_t *)d_event_counts);
}

int tcmi_call(tcmi_ctx *ctx, const int32_t *counts, int64_t L, int32_t mincov, int include_ambig, uint8_t *plain,
              uint8_t *alt, uint8_t *flags, int32_t *event_idx, int64_t *n_events)
{
    if (!ctx || !counts || !plain || !alt || !flags) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    if (L <= 0) return tcmi_fail(ctx, TCMI_E_ARG, "L must be positive");
    int rc = tcmi_ws_load_counts(ctx, counts, L);
    if (rc) return rc;
    const int64_t ld = ctx->ws_ld, nblk = (L + 255) / 256;
    tcmi_dev_tmp d_ev, d_evc;
    if (event_idx) {
        TCMI_HIP(ctx, d_ev.alloc((size_t)nblk * 256 * 4));
        TCMI_HIP(ctx, d_evc.alloc((size_t)nblk * 4));
    }
    rc = tcmi_call_dev(ctx, ctx->d_counts, L, ld, mincov, include_ambig, ctx->d_plain, ctx->d_alt, ctx->d_flags, d_ev.p, d_evc.p);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(ctx->h_rec, ctx->d_plain, (size_t)ld * 3, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return tcmi_fail(ctx, TCMI_E_HIP, "record download failed: %s", hipGetErrorString(e));
    std::memcpy(plain, ctx->h_rec, (size_t)L);
    std::memcpy(alt, ctx->h_rec + ld, (size_t)L);
    std::memcpy(flags, ctx->h_rec + 2 * ld, (size_t)L);
    if (event_idx) {
        std::vector<int32_t> ev((size_t)nblk * 256), evc((size_t)nblk);
        e = hipMemcpy(ev.data(), d_ev.p, ev.size() * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(evc.data(), d_evc.p, evc.size() * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = tcmi_fail(ctx, TCMI_E_HIP, "event download failed: %s", hipGetErrorString(e));
        int64_t n = 0;
        for (int64_t b = 0; !rc && b < nblk; ++b)
            for (int32_t k = 0; k < evc[(size_t)b]; ++k) event_idx[n++] = ev[(size_t)b * 256 + k];
        if (n_events) *n_events = n;
    }
    return rc;
}

} // extern "C"
