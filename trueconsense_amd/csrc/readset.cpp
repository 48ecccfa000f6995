// readset.cpp — HOST: tcmi_readset_upload.  The device packer is tried first (pack_device.hip); what it declines goes through the host
// packer's stages (host_pack.h: select, plan_chunks, pack_aligned, pack_general), whose arrays are copied into HBM here.
#include <atomic>
#include <chrono>
#include <cstdlib>

#include "host_pack.h"
#include "tcmi_internal.h"

namespace {

struct Up {
    tcmi_ctx *ctx;
    tcmi_readset *rs;
    int operator()(void **d, const void *h, size_t bytes)
    {
        // +256 B slack so 16-byte vector loads around the last elements stay inside the allocation
        hipError_t e = hipMalloc(d, bytes + 256);
        if (e != hipSuccess) return tcmi_fail(ctx, TCMI_E_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        e = hipMemsetAsync((char *)*d + bytes, 0, 256, ctx->stream);
        if (e == hipSuccess && bytes) e = hipMemcpyAsync(*d, h, bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return tcmi_fail(ctx, TCMI_E_HIP, "upload failed: %s", hipGetErrorString(e));
        rs->dev_bytes += (int64_t)bytes;
        return TCMI_OK;
    }
};

int check_reads(tcmi_ctx *ctx, const tcmi_reads *r)
{
    const char *msg;
    const int rc = tcmi_host_check_reads(r, &msg);
    return rc ? tcmi_fail(ctx, rc, "%s", msg) : TCMI_OK;
}

} // namespace

void tcmi_host_packed_free(tcmi_host_packed *p) { delete p; }

extern "C" {

int tcmi_reads_extent(const tcmi_reads *r, int64_t ref_len, int64_t *out_L)
{
    int rc = check_reads(nullptr, r);
    if (rc) return rc;
    if (!out_L) return tcmi_fail(nullptr, TCMI_E_ARG, "out_L is NULL");
    int64_t L = ref_len > 0 ? ref_len : 0;
    const tcmi_layout none;
    for (int64_t i = 0; i < r->n_reads; ++i) {
        int64_t span;
        if (!tcmi_host_piles_up(r, i, &span, none)) continue;
        if (r->pos[i] + span > L) L = r->pos[i] + span;
    }
    *out_L = L;
    return TCMI_OK;
}

int tcmi_readset_free(tcmi_ctx *ctx, tcmi_readset *rs)
{
    if (!rs) return TCMI_OK;
    if (ctx) (void)hipSetDevice(ctx->device);
    for (tcmi_readset::Part &p : rs->parts) (void)tcmi_readset_free(p.cx, p.rs);      // (a read set of sub-ranges: each part with its own context)
    rs->parts.clear();
    if (rs->d_blob) {                                            // device-packed: one allocation holds the aligned set
        if (ctx && ctx->device == rs->device && ctx->blob_pool.size() < 4 && rs->blob_bytes)
            ctx->blob_pool.push_back({rs->d_blob, rs->blob_bytes});   // (stream order: the next user's kernels queue behind this one's)
        else
            (void)hipFree(rs->d_blob);
        rs->d_flenoff = nullptr; rs->d_fseq = nullptr; rs->d_fevent = nullptr; rs->d_fchunk = nullptr; rs->d_fcovrun = nullptr;
    }
    void *ptrs[] = {rs->d_flenoff, rs->d_fseq, rs->d_fevent, rs->d_fchunk, rs->d_fcovrun, rs->d_pos, rs->d_meta,
                    rs->d_lseq, rs->d_cigar, rs->d_seq, rs->d_round_cig, rs->d_round_seq};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    delete rs;
    return TCMI_OK;
}

// One or several BAMs into one read set; BAM b's positions are shifted by b * stride, so that the
// kernels see one long coordinate axis and a single launch tallies the whole batch.
static int upload_impl(tcmi_ctx *ctx, const tcmi_reads *const *batch, int32_t n_batch, int64_t stride, tcmi_readset **out)
{
    if (!ctx || !out || !batch || n_batch < 1) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    *out = nullptr;
    const tcmi_rule_beyond beyond = tcmi_rules_beyond_host(ctx->rules);
    if (beyond == TCMI_RULE_FLOOR)                              // (never a silently unfiltered result)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "the context's base-quality floor is %d (--min-baseq): flat read arrays carry no QUAL and the host packer "
                         "knows no floor; only files decoded on the device are tallied under it", (int)ctx->rules.min_bq);
    if (beyond == TCMI_RULE_PRIMERS)                            // (... nor a silently unmasked one)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "the context holds a primer table of %d primers (--primers): the host packer knows no primer mask; only "
                         "files decoded on the device are tallied under it", (int)ctx->rules.primers->n_primers);
    if (beyond == TCMI_RULE_MATE)                               // (... nor pairs silently counted twice)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "the context's mate-overlap rule is on (--mate-overlap): flat read arrays carry no names and no mate "
                         "fields; only whole files decoded on the device are tallied under it");
    if (beyond == TCMI_RULE_DEDUP)                              // (... nor duplicates silently counted)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "the context's duplicate rule is on (--dedup): flat read arrays carry no names, no mate fields and no "
                         "QUAL; only whole files decoded on the device are tallied under it");
    int rc = TCMI_OK;
    for (int32_t b = 0; b < n_batch; ++b) {
        rc = check_reads(ctx, batch[b]);
        if (rc) return rc;
    }
    TCMI_HIP(ctx, hipSetDevice(ctx->device));
    tcmi_host_pack_opts opt;
    opt.host_threads = ctx->host_threads;
    opt.use_fast = ctx->tally_variant != 1;
    opt.project_reads = ctx->project_reads != 0;
    opt.chunk_stages = ctx->chunk_stages;
    opt.stage_cap = ctx->stage_cap;
    opt.balance = ctx->balance_chunks != 0;
    opt.slots = (int64_t)ctx->n_cu * ctx->wg_per_cu;
    const bool timing = std::getenv("TCMI_UPLOAD_TIMING") != nullptr;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    };
    const auto t0 = now();
    static std::atomic<uint64_t> next_uid{1};

    // ---- default: the BAM-native arrays go to the device as they are and HIP kernels pack them (pack_device.hip) ----
    if (ctx->device_pack && opt.use_fast && opt.project_reads && n_batch == 1) {
        const tcmi_reads *r = batch[0];
        tcmi_readset *rs = new tcmi_readset();
        rs->uid = next_uid.fetch_add(1);
        rs->n_reads = r->n_reads;
        rs->device = ctx->device;
        uint32_t why = 0;
        rc = tcmi_upload_and_pack_on_device(ctx, r, rs, &why);
        if (rc == TCMI_OK) {
            if (timing) std::fprintf(stderr, "[tcmi upload] device pack: %.1f ms (%.1f MB on the device)\n", ms(t0, now()), rs->dev_bytes / 1e6);
            *out = rs;
            return TCMI_OK;
        }
        tcmi_readset_free(ctx, rs);
        if (rc != TCMI_E_UNSUPPORTED) return rc;
        if (timing) std::fprintf(stderr, "[tcmi upload] device pack declined (flags 0x%x): host packer\n", why);
    }

    // ---- the host packer, into the buffers the context keeps between uploads ----
    if (!ctx->host_packed) ctx->host_packed = new tcmi_host_packed();
    tcmi_host_packed &P = *ctx->host_packed;
    struct Trim {                           // big batches do not keep their gigabytes around
        tcmi_ctx *c;
        ~Trim() { if (c->host_packed && c->host_packed->bytes() > ((size_t)768 << 20)) { tcmi_host_packed_free(c->host_packed); c->host_packed = nullptr; } }
    } trim{ctx};
    rc = tcmi_host_select(batch, n_batch, stride, ctx->layout, opt, &P);
    if (rc) return tcmi_fail(ctx, rc, "%s", P.msg);
    const auto t1 = now();
    tcmi_host_plan_chunks(opt, &P);
    rc = tcmi_host_pack_aligned(opt, &P);
    if (rc) return tcmi_fail(ctx, rc, "%s", P.msg);
    const auto t2 = now();
    tcmi_host_pack_general(&P);
    const auto t3 = now();

    const int64_t nf = (int64_t)P.fsel.size(), ng = (int64_t)P.gsel.size();
    tcmi_readset *rs = new tcmi_readset();
    rs->uid = next_uid.fetch_add(1);
    rs->n_reads = P.n_reads_in; rs->n_piled = P.n_piled(); rs->alg_bytes = P.alg; rs->max_end = P.max_end; rs->device = ctx->device;
    rs->n_lay = ctx->layout.n(); rs->ref_ext = P.ref_ext; rs->n_dropped = P.n_dropped; rs->lay_gen = ctx->lay_gen;
    rs->f_reads = nf; rs->f_chunks = (int64_t)P.chunks.size(); rs->f_words = (int64_t)P.f_words;
    rs->f_events = (int64_t)P.f_event.size();
    rs->g_reads = ng; rs->n_rounds = P.n_rounds; rs->n_cigar = P.g_cig; rs->n_seqw = P.g_seqw;
    Up up{ctx, rs};
    if (nf) {
        rc = up((void **)&rs->d_flenoff, P.f_lenoff.data(), (size_t)nf * 4);
        if (!rc && !P.f_event.empty()) rc = up((void **)&rs->d_fevent, P.f_event.data(), P.f_event.size() * 4);
        if (!rc) rc = up((void **)&rs->d_fseq, P.f_seq, P.f_words * 4);
        if (!rc) rc = up((void **)&rs->d_fchunk, P.chunks.data(), P.chunks.size() * sizeof(tcmi_fast_chunk));
        if (!rc && !P.f_covrun.empty()) rc = up((void **)&rs->d_fcovrun, P.f_covrun.data(), P.f_covrun.size() * 4);
    }
    if (!rc && ng) {
        rc = up((void **)&rs->d_pos, P.g_pos.data(), (size_t)ng * 4);
        if (!rc) rc = up((void **)&rs->d_meta, P.g_meta.data(), (size_t)ng * 4);
        if (!rc) rc = up((void **)&rs->d_lseq, P.g_lseq.data(), (size_t)ng * 4);
        if (!rc) rc = up((void **)&rs->d_cigar, P.g_cigar.data(), (size_t)P.g_cig * 4);
        if (!rc) rc = up((void **)&rs->d_seq, P.g_seq.data(), (size_t)P.g_seqw * 4);
        if (!rc) rc = up((void **)&rs->d_round_cig, P.g_round_cig.data(), (size_t)(P.n_rounds + 1) * 8);
        if (!rc) rc = up((void **)&rs->d_round_seq, P.g_round_seq.data(), (size_t)(P.n_rounds + 1) * 8);
    }
    if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = tcmi_fail(ctx, TCMI_E_HIP, "sync after upload failed");
    if (rc) { tcmi_readset_free(ctx, rs); return rc; }
    if (timing)
        std::fprintf(stderr, "[tcmi upload] classify %.1f ms, pack aligned %.1f ms (%d threads), pack general %.1f ms, H2D %.1f ms (%.1f MB)\n",
                     ms(t0, t1), ms(t1, t2), ctx->host_threads, ms(t2, t3), ms(t3, now()), rs->dev_bytes / 1e6);
    *out = rs;
    return TCMI_OK;
}

int tcmi_readset_upload(tcmi_ctx *ctx, const tcmi_reads *r, tcmi_readset **out)
{
    return upload_impl(ctx, &r, 1, 0, out);
}

int tcmi_readset_upload_batch(tcmi_ctx *ctx, const tcmi_reads *const *reads, int32_t n, int64_t stride, tcmi_readset **out)
{
    if (n < 1 || n > 4096 || stride <= 0 || stride % 256) return tcmi_fail(ctx, TCMI_E_ARG, "need 1 <= n <= 4096 and a positive stride that is a multiple of 256");
    if (ctx && ctx->layout.n()) return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "batched uploads do not take a contig layout (tcmi_ctx_set_layout)");
    return upload_impl(ctx, reads, n, stride, out);
}

int tcmi_readset_ref_extents(const tcmi_readset *rs, int32_t n_ref, int64_t *max_end)
{
    if (!rs || n_ref < 0 || (n_ref > 0 && !max_end)) return tcmi_fail(nullptr, TCMI_E_ARG, "null argument");
    if (rs->parts.size() || (size_t)n_ref != rs->ref_ext.size())
        return tcmi_fail(nullptr, TCMI_E_ARG, "the read set holds %zu per-reference extents (uploaded under a layout of that size), not %d",
                         rs->parts.size() ? (size_t)0 : rs->ref_ext.size(), n_ref);
    for (int32_t t = 0; t < n_ref; ++t) max_end[t] = rs->ref_ext[(size_t)t];
    return TCMI_OK;
}

int tcmi_readset_dropped(const tcmi_readset *rs, int64_t *n_dropped)
{
    if (!rs || !n_dropped) return tcmi_fail(nullptr, TCMI_E_ARG, "null argument");
    *n_dropped = rs->n_dropped;
    return TCMI_OK;
}

int tcmi_readset_min_base_quality(const tcmi_readset *rs, int32_t *q)
{
    if (!rs || !q) return tcmi_fail(nullptr, TCMI_E_ARG, "null argument");
    *q = rs->rules.min_bq;
    return TCMI_OK;
}

int tcmi_readset_primers(const tcmi_readset *rs, int32_t *n_primers, int64_t *n_masked_reads)
{
    if (!rs) return tcmi_fail(nullptr, TCMI_E_ARG, "null argument");
    if (n_primers) *n_primers = rs->rules.primers ? rs->rules.primers->n_primers : 0;
    if (n_masked_reads) *n_masked_reads = rs->n_masked;
    return TCMI_OK;
}

int tcmi_readset_mate_overlap(const tcmi_readset *rs, int32_t *on, int64_t *pairs, int64_t *clipped_reads, int64_t *clipped_columns, int64_t *ambiguous)
{
    if (!rs) return tcmi_fail(nullptr, TCMI_E_ARG, "null argument");
    if (on) *on = rs->rules.mate;
    if (pairs) *pairs = rs->mate_stat[0];
    if (clipped_reads) *clipped_reads = rs->mate_stat[1];
    if (clipped_columns) *clipped_columns = rs->mate_stat[2];
    if (ambiguous) *ambiguous = rs->mate_stat[3];
    return TCMI_OK;
}

int tcmi_readset_dedup(const tcmi_readset *rs, int32_t *on, int64_t *templates, int64_t *dup_templates, int64_t *dup_records, int64_t *dup_sets)
{
    if (!rs) return tcmi_fail(nullptr, TCMI_E_ARG, "null argument");
    if (on) *on = rs->rules.dedup;
    if (templates) *templates = rs->dup_stat[0];
    if (dup_templates) *dup_templates = rs->dup_stat[1];
    if (dup_records) *dup_records = rs->dup_stat[2];
    if (dup_sets) *dup_sets = rs->dup_stat[3];
    return TCMI_OK;
}

int tcmi_readset_filtered(const tcmi_readset *rs, int64_t *n_filtered)
{
    if (!rs || !n_filtered) return tcmi_fail(nullptr, TCMI_E_ARG, "null argument");
    *n_filtered = rs->n_filtered;
    return TCMI_OK;
}

int tcmi_readset_info(const tcmi_readset *rs, int64_t *n_reads, int64_t *n_piled, int64_t *alg, int64_t *dev,
                      int64_t *max_end)
{
    if (!rs) return tcmi_fail(nullptr, TCMI_E_ARG, "readset is NULL");
    if (n_reads) *n_reads = rs->n_reads;
    if (n_piled) *n_piled = rs->n_piled;
    if (alg) *alg = rs->alg_bytes;
    if (dev) *dev = rs->dev_bytes;
    if (max_end) *max_end = rs->max_end;
    return TCMI_OK;
}

int tcmi_readset_origin(const tcmi_readset *rs, int32_t *packed_on_device)
{
    if (!rs || !packed_on_device) return tcmi_fail(nullptr, TCMI_E_ARG, "null argument");
    *packed_on_device = rs->packed_on_device;
    return TCMI_OK;
}

int tcmi_readset_sets(const tcmi_readset *rs, int64_t *aligned_reads, int64_t *aligned_chunks, int64_t *general_reads)
{
    if (!rs) return tcmi_fail(nullptr, TCMI_E_ARG, "readset is NULL");
    if (aligned_reads) *aligned_reads = rs->f_reads;
    if (aligned_chunks) *aligned_chunks = rs->f_chunks;
    if (general_reads) *general_reads = rs->g_reads;
    return TCMI_OK;
}

} // extern "C"
