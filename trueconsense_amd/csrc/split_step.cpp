// split_step.cpp — tcmi_split_step: one rank's part of a step of ONE BAM file shared by several GPUs, and the rank's block range
// as sub-ranges side by side.  The joining rule of both is range_join.h.
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <string>
#include <condition_variable>
#include <mutex>
#include <thread>

#include "tcmi_internal.h"
#include "range_join.h"

// A rank's block range [first, first + cnt) as K sub-ranges decoded, packed and tallied SIDE BY SIDE, each on a context of its own (sub-range 0
// on the caller's, the others on helper contexts the caller's context owns: a stream and an arena each) with a host thread of its own
// — the inflate of one sub-range runs under the pack of another, as the many-file runner's contexts overlap files; the tallies add
// into the one matrix (the tally kernel's adds are atomic).  The sub-ranges join like ranks' ranges do: each starts where the one in
// front ends its last record (tcmi_ranges_join).  -> a read set that is the sum of its parts; TCMI_E_UNSUPPORTED: sub-ranges that cannot
// vouch for each other (a sub-range without a record start, a chain that does not join) — the caller decodes the range in one piece.
static int split_sub_ranges(tcmi_ctx *ctx, const tcmi_bamfile *f, int64_t first, int64_t cnt, int K, int64_t L, int64_t ld, void *d_counts,
                            tcmi_readset **out)
{
    *out = nullptr;
    while ((int)ctx->helpers.size() < K - 1) {
        tcmi_ctx *h = nullptr;
        const int rc = tcmi_ctx_create(ctx->device, &h);
        if (rc) return tcmi_fail(ctx, rc, "a helper context for the sub-ranges could not be made");
        ctx->helpers.push_back(h);
    }
    for (tcmi_ctx *h : ctx->helpers) {                          // (the caller's decoder options)
        h->verify_crc = ctx->verify_crc; h->decode_token_mb = ctx->decode_token_mb; h->one_sync = ctx->one_sync; h->mid_wait = ctx->mid_wait;
        h->prefix_kernels = ctx->prefix_kernels; h->h2d_pieces = ctx->h2d_pieces; h->sym_scratch_div = ctx->sym_scratch_div; h->prof = false;
        h->rules = ctx->rules;                                  // (whole: the one caller has refused the mate rule and the duplicate rule, so they are off in them too)
    }
    TCMI_HIP(ctx, hipStreamSynchronize(ctx->stream));            // (the matrix is zero before anybody adds to it)
    std::vector<tcmi_readset *> rs((size_t)K, nullptr);
    std::vector<int> rcs((size_t)K, TCMI_OK);
    std::vector<int64_t> fb((size_t)K + 1);
    for (int k = 0; k <= K; ++k) fb[(size_t)k] = first + cnt * k / K;
    // skewed starts: sub-range k's inflate waits (on the device) for the bgzf_symbols of sub-range k - 1; its thread waits (on the host)
    // until that launch and its event are queued.  A sub-range that fails before its launch lets the next one go all the same.
    static const bool skew = !(std::getenv("TCMI_SPLIT_SKEW") && std::atoi(std::getenv("TCMI_SPLIT_SKEW")) == 0);
    std::mutex mu;
    std::condition_variable cv;
    std::vector<char> queued((size_t)K, 0);
    auto release = [&](int k) { { std::lock_guard<std::mutex> lk(mu); queued[(size_t)k] = 1; } cv.notify_all(); };
    auto cx_of = [&](int k) { return k == 0 ? ctx : ctx->helpers[(size_t)k - 1]; };
    if (skew)
        for (int k = 0; k < K; ++k)
            if (!cx_of(k)->ev_after_sym && hipEventCreateWithFlags(&cx_of(k)->ev_after_sym, hipEventDisableTiming) != hipSuccess)
                return tcmi_fail(ctx, TCMI_E_HIP, "hipEventCreate failed");
    auto work = [&](int k) {
        tcmi_ctx *cx = cx_of(k);
        if (skew) {
            if (k > 0) {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return queued[(size_t)k - 1] != 0; });
                cx->ev_before_sym = cx_of(k - 1)->ev_after_sym;
            }
            cx->after_sym = [&release, k] { release(k); };
        }
        int rc = tcmi_readset_from_bamfile_blocks(cx, f, fb[(size_t)k], fb[(size_t)k + 1] - fb[(size_t)k], &rs[(size_t)k], nullptr);
        if (skew) { cx->after_sym = nullptr; cx->ev_before_sym = nullptr; release(k); }
        if (rc == TCMI_OK && rs[(size_t)k]->max_end > L) rc = tcmi_fail(cx, TCMI_E_ARG, "L=%lld is smaller than the reads' extent %lld", (long long)L, (long long)rs[(size_t)k]->max_end);
        if (rc == TCMI_OK && rs[(size_t)k]->n_piled) rc = tcmi_tally_dev(cx, rs[(size_t)k], L, ld, d_counts, 0);
        if (rc == TCMI_OK && hipStreamSynchronize(cx->stream) != hipSuccess) rc = tcmi_fail(cx, TCMI_E_HIP, "hipStreamSynchronize failed");
        rcs[(size_t)k] = rc;
    };
    {
        // (a thread that cannot be started — std::system_error must not cross the C ABI — has its sub-range done by this one, after its own;
        //  in order: a sub-range waits for the one in front to be queued)
        std::vector<std::thread> th;
        std::vector<int> inline_k;
        for (int k = 1; k < K; ++k) {
            try { th.emplace_back(work, k); }
            catch (const std::exception &) { inline_k.push_back(k); }
        }
        work(0);
        for (int k : inline_k) work(k);                             // (ascending: each waits only for the one in front of it to be queued)
        for (std::thread &t : th) t.join();
    }
    auto drop = [&]() { for (int k = 0; k < K; ++k) if (rs[(size_t)k]) tcmi_readset_free(cx_of(k), rs[(size_t)k]); };
    for (int k = 0; k < K; ++k)
        if (rcs[(size_t)k]) {
            // (a sub-range that failed may have queued work that adds to the matrix; the caller zeroes it again on ITS stream, which has
            //  no order with a helper's: everything queued ends first.  A wait that fails here has nothing to add to the failure at hand)
            for (int j = 0; j < K; ++j) (void)hipStreamSynchronize(cx_of(j)->stream);
            const std::string why = cx_of(k)->err;
            drop();
            return tcmi_fail(ctx, rcs[(size_t)k], "sub-range %d of %d: %s", k, K, why.c_str());
        }
    // the joins: a sub-range behind the first vouches for nothing by itself
    std::vector<int64_t> rg((size_t)K * 4);
    bool plain = true;
    for (int k = 0; k < K; ++k) {
        rg[4 * (size_t)k] = fb[(size_t)k]; rg[4 * (size_t)k + 1] = fb[(size_t)k + 1] - fb[(size_t)k];
        rg[4 * (size_t)k + 2] = rs[(size_t)k]->range_first; rg[4 * (size_t)k + 3] = rs[(size_t)k]->range_next;
        if ((k > 0 && rs[(size_t)k]->range_first < 0) || rs[(size_t)k]->range_next < 0) plain = false;      // (a sub-range that found no record start, or lies inside one record)
    }
    int who = 0; int64_t at = 0, want = 0;
    const char *why = plain ? tcmi_ranges_join(reinterpret_cast<const int64_t (*)[4]>(rg.data()), K, -1, &who, &at, &want) : "a sub-range holds no record start";
    if (why) {
        drop();
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "the sub-ranges of blocks [%lld, %lld) do not join (%s): the range in one piece", (long long)first, (long long)(first + cnt), why);
    }
    tcmi_readset *sum = new tcmi_readset();
    sum->device = ctx->device; sum->packed_on_device = 2;
    sum->range_first = rs[0]->range_first; sum->range_next = rs[(size_t)K - 1]->range_next;
    tcmi_rules_stamp(sum, ctx, true);
    for (int k = 0; k < K; ++k) {
        const tcmi_readset *r = rs[(size_t)k];
        sum->n_reads += r->n_reads; sum->n_piled += r->n_piled; sum->alg_bytes += r->alg_bytes; sum->dev_bytes += r->dev_bytes;
        sum->max_end = std::max(sum->max_end, r->max_end); sum->max_len = std::max(sum->max_len, r->max_len); sum->s_reads += r->s_reads;
        sum->f_reads += r->f_reads; sum->n_filtered += r->n_filtered; sum->n_masked += r->n_masked;
        sum->parts.push_back({cx_of(k), rs[(size_t)k]});
    }
    *out = sum;
    return TCMI_OK;
}

extern "C" {

// One rank's part of a step of ONE BAM file shared by several GPUs (include/tcmi.h): decode + pack + tally its block range, the
// caller's reduce hook, and on rank 0 the call kernel.  Behind the matrix: six words per rank (its range and anchors, in its own
// slot, zeros in the others' — the sum hands rank 0 the table) and one word that counts the ranks that failed.  Every rank enters
// the exchange exactly once, whatever happened to it before — a device that cannot be set, a workspace that cannot be allocated,
// a range that is refused: its share is then zeros + one failure.
int tcmi_split_step(tcmi_ctx *ctx, const tcmi_bamfile *f, int64_t first_block, int64_t n_blocks, int64_t L, int64_t ld, void *d_counts,
                    int32_t mincov, int include_ambig, tcmi_reduce_fn reduce, void *user, int rank, int world, tcmi_readset **rs_out,
                    const uint8_t **plain, const uint8_t **alt, const uint8_t **flags)
{
    if (!ctx || !f || !d_counts || !reduce || !rs_out) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    if (ctx->layout.n()) return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "tcmi_split_step does not take a contig layout (tcmi_ctx_set_layout)");
    if (ctx->rules.mate)                                        // (a record's mate may lie in another rank's range)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "tcmi_split_step does not run under the mate-overlap rule (--mate-overlap): a record's mate may lie in "
                         "another rank's block range");
    if (ctx->rules.dedup)                                       // (... and so may a template's other records)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "tcmi_split_step does not run under the duplicate rule (--dedup): a template's other records may lie in "
                         "another rank's block range");
    if (L <= 0 || ld < L) return tcmi_fail(ctx, TCMI_E_ARG, "need 0 < L <= ld");
    if (world < 1 || rank < 0 || rank >= world) return tcmi_fail(ctx, TCMI_E_ARG, "need 0 <= rank < world");
    *rs_out = nullptr;
    const bool is_root = rank == 0;
    const size_t n_mat = (size_t)ld * TCMI_NCOL, n_words = n_mat + (size_t)TCMI_SPLIT_TAIL_WORDS(world);
    int32_t *const d_all = static_cast<int32_t *>(d_counts);
    tcmi_readset *rs = nullptr;
    int own = TCMI_OK;
    std::string own_err;
    auto note = [&](int code) { own = code; own_err = ctx->err; };
    // (all of these are argument checks of the caller's on every rank alike — the collective has not been entered — or failures of THIS
    // rank, which must not keep it from the exchange)
    if (hipSetDevice(ctx->device) != hipSuccess) note(tcmi_fail(ctx, TCMI_E_HIP, "hipSetDevice(%d) failed", ctx->device));
    if (!own) { const int rc0 = tcmi_ws_ensure(ctx, L); if (rc0) note(rc0); }
    if (!own && hipMemsetAsync(d_counts, 0, n_words * 4, ctx->stream) != hipSuccess) note(tcmi_fail(ctx, TCMI_E_HIP, "hipMemsetAsync of the count matrix failed"));
    int64_t all = 0, inflated = 0;
    (void)tcmi_bamfile_info(f, nullptr, &inflated, &all, nullptr, nullptr, nullptr);
    const int64_t cnt = std::max<int64_t>(0, n_blocks < 0 ? all - first_block : std::min<int64_t>(n_blocks, all - first_block));      // the blocks of the range that the file has
    bool tallied = false;
    if (!own) {                                                 // sub-ranges side by side where the range is large enough (else, or if they do not work out: in one piece)
        static const int sub_env = std::getenv("TCMI_SPLIT_SUB") ? std::atoi(std::getenv("TCMI_SPLIT_SUB")) : 0;
        int K = sub_env > 0 ? sub_env : ctx->split_sub;
        // (auto: a true RANGE of a larger file gains ~ 10 % from three sub-ranges — 2.65 - 2.83 -> 2.42 - 2.54 ms at 4 M reads, 3.9 -> 3.5 - 3.6 ms
        //  at 6.25 M; the WHOLE file as one rank's range — world 1 — is decoded without the range's re-based block table and loses 3 - 8 % to them:
        //  profiles/r06i_split_ab.log, r06j_*)
        const bool whole = first_block == 0 && cnt == all;
        if (K <= 0) K = whole ? 1 : cnt >= 6144 ? 3 : cnt >= 4096 ? 2 : 1;
        K = (int)std::min<int64_t>(std::min(K, 8), std::max<int64_t>(1, cnt / 64));
        if (K > 1 && !ctx->stream_hi) {
            const int rc0 = split_sub_ranges(ctx, f, first_block, cnt, K, L, ld, d_counts, &rs);
            // (whatever kept the sub-ranges from working out — they do not join, a helper context could not be made, a sub-range was
            //  refused — the range in one piece has the last word: it words the refusal, or simply works)
            if (rc0 == TCMI_OK) { tallied = true; ++ctx->stat_split_sub; }
            else if (hipMemsetAsync(d_counts, 0, n_words * 4, ctx->stream) != hipSuccess) note(tcmi_fail(ctx, TCMI_E_HIP, "hipMemsetAsync of the count matrix failed"));
        }
    }
    if (!own && !tallied) { const int rc0 = tcmi_readset_from_bamfile_blocks(ctx, f, first_block, n_blocks, &rs, nullptr); if (rc0) note(rc0); }
    if (!own && rs->max_end > L) note(tcmi_fail(ctx, TCMI_E_ARG, "L=%lld is smaller than the reads' extent %lld", (long long)L, (long long)rs->max_end));
    if (!own && !tallied && rs->n_piled) { const int rc0 = tcmi_tally_dev(ctx, rs, L, ld, d_counts, 0); if (rc0) note(rc0); }
    if (own) {                                                  // this rank's share is zeros + one failure
        static const int32_t one = 1;
        (void)hipMemsetAsync(d_counts, 0, n_words * 4, ctx->stream);
        (void)hipMemcpyAsync(d_all + (n_words - 1), &one, 4, hipMemcpyHostToDevice, ctx->stream);
    } else {
        const int64_t v[3] = {rs->range_first, rs->range_next, 0};
        int32_t *t = ctx->split_tail;
        t[0] = (int32_t)first_block; t[1] = (int32_t)cnt;
        std::memcpy(t + 2, &v[0], 8); std::memcpy(t + 4, &v[1], 8);
        (void)hipMemcpyAsync(d_all + n_mat + (size_t)6 * rank, t, 24, hipMemcpyHostToDevice, ctx->stream);
    }
    const int rrc = reduce(user, d_counts, (int64_t)n_words, (void *)ctx->stream);
    if (rrc) { if (rs) tcmi_readset_free(ctx, rs); return tcmi_fail(ctx, TCMI_E_HIP, "the reduce hook failed (%d)", rrc); }
    int rc = TCMI_OK;
    std::vector<int32_t> tail((size_t)TCMI_SPLIT_TAIL_WORDS(world), 0);
    if (is_root && !own) {
        rc = tcmi_launch_call(ctx, d_all, L, ld, mincov, include_ambig, 0, ctx->h_rec, ctx->h_rec + ctx->ws_ld, ctx->h_rec + 2 * ctx->ws_ld, nullptr, nullptr);
        if (!rc && hipMemcpyAsync(tail.data(), d_all + n_mat, tail.size() * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = tcmi_fail(ctx, TCMI_E_HIP, "copy failed");
    }
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && !rc && !own) rc = tcmi_fail(ctx, TCMI_E_HIP, "hipStreamSynchronize failed");
    ctx->counts_clean = false;
    if (own) { if (rs) tcmi_readset_free(ctx, rs); return tcmi_fail(ctx, own, "%s", own_err.c_str()); }
    if (rc) { tcmi_readset_free(ctx, rs); return rc; }
    const int32_t failed = tail.back();
    if (is_root && failed) { tcmi_readset_free(ctx, rs); return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "%d rank(s) could not decode their range of %s on the device", (int)failed, tcmi_bamfile_path(f)); }
    if (is_root) {
        std::vector<int64_t> rg((size_t)world * 4);
        for (int r = 0; r < world; ++r) {
            const int32_t *t = tail.data() + (size_t)6 * r;
            rg[4 * r] = t[0]; rg[4 * r + 1] = t[1];
            std::memcpy(&rg[4 * r + 2], t + 2, 8); std::memcpy(&rg[4 * r + 3], t + 4, 8);
        }
        int who = 0; int64_t at = 0, want = 0;
        const char *why = tcmi_ranges_join(reinterpret_cast<const int64_t (*)[4]>(rg.data()), world, inflated, &who, &at, &want);
        if (why) {
            tcmi_readset_free(ctx, rs);
            return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "%s: the ranks' block ranges do not join into one chain of alignment records (rank %d %s: offset %lld, expected %lld): host reader",
                             tcmi_bamfile_path(f), who, why, (long long)at, (long long)want);
        }
    }
    *rs_out = rs;
    if (plain) *plain = ctx->h_rec;
    if (alt) *alt = ctx->h_rec + ctx->ws_ld;
    if (flags) *flags = ctx->h_rec + 2 * ctx->ws_ld;
    return TCMI_OK;
}

} // extern "C"
