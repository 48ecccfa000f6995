// array_pipeline.cpp — HOST: many read sets resident in HBM through the hot path with the GPU and the host cores both busy.
//
// BASELINE.json configs[3] ("independent BAMs, one per stream, no collective") as a native batch
// runner: the calling thread enqueues step i+1 (memset + tally + call + D2H of the call records)
// behind step i on one HIP stream, using `n_slots` workspaces, while `n_walkers` host threads turn
// finished records into consensus sequences: insert candidates -> modal tokens (Events.py:5-82),
// then the sequential walk of Sequences.BuildConsensus (walk_records.cpp).
// No Python in the loop, so no GIL between the walkers.  BAM files instead of read sets: pipeline.cpp.
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

#include "walk_records.h"


struct tcmi_pipeline {
    int device = 0;
    std::vector<tcmi_ctx *> slots;
    std::vector<int> slot_busy;                     // 1 from step_begin until the walk has consumed the records
    tcmi_orfs orfs;
    // walker pool
    struct Job { int slot; int64_t item; int b; };
    std::vector<int> slot_jobs;                     // walk jobs still open per slot (a batched item has several)
    int batch = 1;
    int64_t pos_stride = 0;
    std::deque<Job> jobs;
    std::mutex mu;
    std::condition_variable cv_job, cv_done;
    std::vector<std::thread> workers;
    bool stop = false;
    int64_t jobs_open = 0;
    // the run in progress
    int64_t L = 0;
    const tcmi_reads *const *host_reads = nullptr;
    char *out = nullptr;
    int64_t stride = 0;
    int64_t *out_len = nullptr;
    int32_t *status = nullptr;
    std::string err;
};

namespace {

int walk_item(tcmi_pipeline *p, int slot, int64_t item_in, int b)
{
    const int64_t item = item_in * p->batch + b;               // output index
    const int64_t shift = (int64_t)b * p->pos_stride;           // BAM b's slice of every record plane
    tcmi_ctx *c = p->slots[(size_t)slot];
    const int64_t L = p->L, ld = c->ws_ld;
    const uint8_t *flags = c->h_rec + 2 * ld + shift;
    std::vector<int64_t> cand;
    tcmi_insert_candidates(flags, L, cand);
    return tcmi_walk_records(c->h_rec + shift, c->h_rec + ld + shift, flags, L, cand, p->host_reads ? p->host_reads[item] : nullptr, nullptr,
                             p->orfs, p->out + item * p->stride, p->stride, &p->out_len[item], (long long)item);
}

void worker_main(tcmi_pipeline *p)
{
    for (;;) {
        tcmi_pipeline::Job job;
        {
            std::unique_lock<std::mutex> lk(p->mu);
            p->cv_job.wait(lk, [&] { return p->stop || !p->jobs.empty(); });
            if (p->jobs.empty()) return;
            job = p->jobs.front();
            p->jobs.pop_front();
        }
        const int rc = walk_item(p, job.slot, job.item, job.b);
        {
            std::lock_guard<std::mutex> lk(p->mu);
            if (p->status) p->status[job.item * p->batch + job.b] = rc;
            if (--p->slot_jobs[(size_t)job.slot] == 0) p->slot_busy[(size_t)job.slot] = 0;
            --p->jobs_open;
        }
        p->cv_done.notify_all();
    }
}

// the first slot context whose answer to tcmi_rules_beyond_host is `rule`, or null.  Asked in the order of that function's
// precedence: once no slot answers with a rule in front of `rule`, every slot that has `rule` answers with it.
const tcmi_ctx *first_slot_with(const tcmi_pipeline *p, tcmi_rule_beyond rule)
{
    for (const tcmi_ctx *c : p->slots)
        if (tcmi_rules_beyond_host(c->rules) == rule) return c;
    return nullptr;
}

// what a slot context may not carry: the array pipeline runs read sets uploaded from flat arrays, and its steps fill no table
int refuse_slot_settings(tcmi_pipeline *p)
{
    if (const tcmi_ctx *c = first_slot_with(p, TCMI_RULE_FLOOR))    // (read sets uploaded from flat arrays: they know no base-quality floor)
        return tcmi_fail(p->slots[0], TCMI_E_UNSUPPORTED, "a slot context's base-quality floor is %d (--min-baseq): the array pipeline runs read sets "
                         "uploaded from flat arrays, which carry no QUAL", (int)c->rules.min_bq);
    if (first_slot_with(p, TCMI_RULE_PRIMERS))                      // (... and no primer mask)
        return tcmi_fail(p->slots[0], TCMI_E_UNSUPPORTED, "a slot context holds a primer table (--primers): the array pipeline runs read sets uploaded "
                         "from flat arrays, which the host packer packs without a primer mask");
    if (first_slot_with(p, TCMI_RULE_MATE))                         // (... and no names or mate fields)
        return tcmi_fail(p->slots[0], TCMI_E_UNSUPPORTED, "a slot context's mate-overlap rule is on (--mate-overlap): the array pipeline runs read sets uploaded "
                         "from flat arrays, which carry no names and no mate fields");
    if (first_slot_with(p, TCMI_RULE_DEDUP))                        // (... and no QUAL to score a template by)
        return tcmi_fail(p->slots[0], TCMI_E_UNSUPPORTED, "a slot context's duplicate rule is on (--dedup): the array pipeline runs read sets uploaded "
                         "from flat arrays, which carry no names, no mate fields and no QUAL");
    for (const tcmi_ctx *c : p->slots)                          // (... and no variant table: nobody would fetch its records)
        if (tcmi_var_table_on(c))
            return tcmi_fail(p->slots[0], TCMI_E_UNSUPPORTED, "a slot context carries a variant table setting (--variant-table, tcmi_ctx_set_variants): the array "
                             "pipeline's steps compute none; use tcmi_step or the file runner");
    for (const tcmi_ctx *c : p->slots)                          // (... and no amplicon table, likewise)
        if (tcmi_iv_table_on(c))
            return tcmi_fail(p->slots[0], TCMI_E_UNSUPPORTED, "a slot context carries an amplicon table setting (--amplicon-table, tcmi_ctx_set_intervals): the array "
                             "pipeline's steps compute none; use tcmi_step or the file runner");
    return TCMI_OK;
}

// item `item`'s step failed with `rc` on `slot`: its outputs are empty, the run's first error keeps the context's words
void item_failed(tcmi_pipeline *p, int64_t item, int slot, int rc, int *first_err)
{
    for (int b = 0; b < p->batch; ++b) { p->status[item * p->batch + b] = rc; p->out_len[item * p->batch + b] = 0; }
    if (!*first_err) { *first_err = rc; p->err = tcmi_last_error(p->slots[(size_t)slot]); }
}

// every step is queued: wait for the walkers, then the run's first error — a step's before a walk's
int finish_run(tcmi_pipeline *p, int64_t n_items, int first_err)
{
    {
        std::unique_lock<std::mutex> lk(p->mu);
        p->cv_done.wait(lk, [&] { return p->jobs_open == 0; });
    }
    if (first_err) return tcmi_fail(nullptr, first_err, "%s", p->err.c_str());
    for (int64_t i = 0; i < n_items * p->batch; ++i)
        if (p->status[i]) return tcmi_fail(nullptr, p->status[i], "item %lld: the consensus walk failed (status %d)", (long long)i, p->status[i]);
    return TCMI_OK;
}

} // namespace

extern "C" {

int tcmi_pipeline_create(int device, int n_slots, int n_walkers, tcmi_pipeline **out)
{
    if (!out || n_slots < 1 || n_slots > 64 || n_walkers < 1 || n_walkers > 256)
        return tcmi_fail(nullptr, TCMI_E_ARG, "need 1..64 slots and 1..256 walkers");
    *out = nullptr;
    tcmi_pipeline *p = new tcmi_pipeline();
    p->device = device;
    for (int s = 0; s < n_slots; ++s) {
        tcmi_ctx *c = nullptr;
        // one stream for all workspaces: slot 0 owns it
        const int rc = s == 0 ? tcmi_ctx_create(device, &c) : tcmi_ctx_create_on_stream(device, tcmi_ctx_stream(p->slots[0]), &c);
        if (rc) {
            for (size_t k = p->slots.size(); k-- > 0;) tcmi_ctx_destroy(p->slots[k]);
            delete p;
            return rc;
        }
        p->slots.push_back(c);
    }
    p->slot_busy.assign((size_t)n_slots, 0);
    p->slot_jobs.assign((size_t)n_slots, 0);
    for (int w = 0; w < n_walkers; ++w) p->workers.emplace_back(worker_main, p);
    *out = p;
    return TCMI_OK;
}

int tcmi_pipeline_destroy(tcmi_pipeline *p)
{
    if (!p) return TCMI_OK;
    {
        std::lock_guard<std::mutex> lk(p->mu);
        p->stop = true;
    }
    p->cv_job.notify_all();
    for (auto &t : p->workers) t.join();
    for (size_t k = p->slots.size(); k-- > 0;) tcmi_ctx_destroy(p->slots[k]);    // slot 0 owns the stream: last
    delete p;
    return TCMI_OK;
}

int tcmi_pipeline_set_orfs(tcmi_pipeline *p, int32_t n_orf, const int64_t *start, const int64_t *end, const uint8_t *is_plus)
{
    return tcmi_orfs_assign(p ? &p->orfs : nullptr, n_orf, start, end, is_plus);
}

tcmi_ctx *tcmi_pipeline_ctx(tcmi_pipeline *p, int slot)
{
    return (p && slot >= 0 && slot < (int)p->slots.size()) ? p->slots[(size_t)slot] : nullptr;
}

int tcmi_pipeline_run_batched(tcmi_pipeline *p, int64_t n_items, const tcmi_readset *const *readsets, int32_t batch,
                              int64_t pos_stride, const tcmi_reads *const *host_reads, int64_t L, int32_t mincov,
                              int include_ambig, char *out_cons, int64_t stride, int64_t *out_len, int32_t *status)
{
    if (!p || n_items < 0 || (n_items > 0 && (!readsets || !out_cons || !out_len || !status)) || stride < L + 1)
        return tcmi_fail(nullptr, TCMI_E_ARG, "bad argument (stride must be >= L + 1 + inserted bases)");
    if (batch < 1 || (batch > 1 && (pos_stride < L || pos_stride % 256)))
        return tcmi_fail(nullptr, TCMI_E_ARG, "bad batch / position stride");
    if (const int rc = refuse_slot_settings(p)) return rc;
    p->batch = batch;
    p->pos_stride = batch > 1 ? pos_stride : 0;
    const int64_t L_gpu = batch > 1 ? (int64_t)batch * pos_stride : L;   // positions one step covers
    p->L = L; p->host_reads = host_reads; p->out = out_cons; p->stride = stride; p->out_len = out_len; p->status = status;
    const int n_slots = (int)p->slots.size();
    int64_t submitted = 0;
    int first_err = TCMI_OK;
    // Ride-along call (option defer_call of slot 0): the call of step k is carried by the tally launch of step k + 1,
    // so a step is ONE launch; the last step of the queue (or one nobody followed) launches its call on its own.
    const bool defer = p->slots[0]->defer_call != 0;
    int pending_slot = -1;
    for (int64_t waited = 0; waited < n_items; ++waited) {
        // keep the stream fed: queue every step whose workspace is free
        while (submitted < n_items && submitted - waited < n_slots) {
            const int slot = (int)(submitted % n_slots);
            {
                std::unique_lock<std::mutex> lk(p->mu);
                if (p->slot_busy[(size_t)slot]) {
                    if (submitted > waited) break;               // something is already in flight: come back later
                    p->cv_done.wait(lk, [&] { return !p->slot_busy[(size_t)slot]; });
                }
                p->slot_busy[(size_t)slot] = 1;
            }
            const int rc = defer ? tcmi_step_begin_deferred(p->slots[(size_t)slot], readsets[submitted], L_gpu, mincov, include_ambig,
                                                            pending_slot >= 0 ? p->slots[(size_t)pending_slot] : nullptr)
                                 : tcmi_step_begin(p->slots[(size_t)slot], readsets[submitted], L_gpu, mincov, include_ambig, 0);
            if (defer && !rc) pending_slot = slot;
            if (rc) {
                item_failed(p, submitted, slot, rc, &first_err);
                std::lock_guard<std::mutex> lk(p->mu);
                p->slot_busy[(size_t)slot] = 2;                  // nothing queued for this item
            }
            ++submitted;
        }
        const int slot = (int)(waited % n_slots);
        bool queued;
        {
            std::lock_guard<std::mutex> lk(p->mu);
            queued = p->slot_busy[(size_t)slot] == 1;
            if (!queued) p->slot_busy[(size_t)slot] = 0;
        }
        if (!queued) continue;
        if (slot == pending_slot) pending_slot = -1;             // nobody followed it: tcmi_step_end launches its call
        const int rc = tcmi_step_end(p->slots[(size_t)slot], nullptr, nullptr, nullptr, nullptr, nullptr);
        if (rc) {
            item_failed(p, waited, slot, rc, &first_err);
            std::lock_guard<std::mutex> lk(p->mu);
            p->slot_busy[(size_t)slot] = 0;
            continue;
        }
        {
            std::lock_guard<std::mutex> lk(p->mu);
            p->slot_jobs[(size_t)slot] = batch;
            for (int b = 0; b < batch; ++b) p->jobs.push_back({slot, waited, b});
            p->jobs_open += batch;
        }
        p->cv_job.notify_all();
    }
    return finish_run(p, n_items, first_err);
}

int tcmi_pipeline_run(tcmi_pipeline *p, int64_t n_items, const tcmi_readset *const *readsets,
                      const tcmi_reads *const *host_reads, int64_t L, int32_t mincov, int include_ambig,
                      char *out_cons, int64_t stride, int64_t *out_len, int32_t *status)
{
    return tcmi_pipeline_run_batched(p, n_items, readsets, 1, 0, host_reads, L, mincov, include_ambig, out_cons, stride,
                                     out_len, status);
}

} // extern "C"
