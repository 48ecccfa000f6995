// pipeline.cpp — HOST: the file runner.  BAM FILES -> FASTA text: the whole command line of the reference (TrueConsense.py:212-264)
// for many inputs, with the GPU and the host cores both busy.  Three stages on their own threads, consecutive BAMs overlapping:
//   read   HOST: file bytes into pinned memory + BGZF block table + BAM header (tcmi_bamfile_read)
//   gpu    one thread per context (stream + device arena): H2D of the compressed bytes, HIP inflate / record chain / pack,
//          tally + call, call records into the item's buffer; a file the device decoder declines is decoded by the host
//          reader (tcmi_bam_load) and packed from its flat arrays
//   walk   HOST: insert tokens when a candidate exists (decodes the BAM on the host then: the decoded reads never left the
//          device), the sequential consensus walk, ">name mincov=N\n<consensus>\n" (Outputs.py:182-183); for --batch also the
//          sample's other output files (outputs_text.cpp)
// No Python in the loop, so no GIL between the walkers.  The walk itself and what the array pipeline (array_pipeline.cpp) shares
// with this runner: walk_records.h.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "walk_records.h"

struct tcmi_filerunner {
    int device = 0, n_readers = 2, n_walkers = 2, host_threads = 8;
    std::vector<tcmi_ctx *> ctxs;
    tcmi_orfs orfs;
    // what the VCF / GFF writers of tcmi_filerunner_run_files need besides the walk (tcmi_filerunner_set_outputs)
    std::string ref_id, ref_seq, vcf_head, gff_head;
    std::vector<std::string> gff_cols;              // per GFF row: source, type, score, strand, phase, attributes
};

namespace {

struct FileItem {
    tcmi_bamfile *file = nullptr;       // after the read stage
    std::vector<uint8_t> rec;           // plain | alt | flags, L each, after the gpu stage
    int64_t L = 0;
    int state = 0;                      // 0 nothing, 1 read, 2 records ready, 3 done
    int rc = TCMI_OK;
    std::string err;
    bool on_device = false;
    std::vector<int64_t> cand;          // the insert candidates of rec's flags
    tcmi_tokens pre;                    // their tokens, resolved on the device while the decoded stream was still resident
    std::vector<int32_t> cov;           // files mode: the coverage column (VCF, coverage TSV)
    std::vector<tcmi_variant> var;      // files mode: the step's variant records, for a sample whose table is wanted
};

struct OutFiles {                       // per item; an entry may be NULL (not wanted)
    const char *const *fasta, *const *vcf, *const *gff, *const *doc;
    const char *const *table;           // the variant table (tcmi_filerunner_run_files_table); n_variants: its records per item, or NULL
    int64_t *n_variants;
    int64_t n_intervals;                // the amplicon table (tcmi_filerunner_run_files_stats): item i's records go to stats[i * n_intervals ...)
    tcmi_interval_stat *stats;
    bool wants(const char *const *list, int64_t i) const { return list && list[i]; }
};

// One call of the runner: what the caller passed and what its three stages share.
struct FileRun {
    tcmi_filerunner *r = nullptr;
    int64_t n = 0;
    const char *const *paths = nullptr, *const *names = nullptr;
    tcmi_bamfile *const *resident = nullptr;        // files already read (and, with tcmi_bamfile_to_device, already in HBM): the caller's
    int64_t ref_len = 0;
    int32_t mincov = 0;
    int include_ambig = 0, device_decode = 1;
    // out_text: n * stride bytes, text i at out_text + i * stride, out_len[i] bytes (stride >= ref_len + inserted bases + name + 32)
    char *out_text = nullptr;
    int64_t stride = 0, *out_len = nullptr;
    int32_t *status = nullptr;
    const OutFiles *files = nullptr;                // files mode: the texts go to files, not to out_text
    std::vector<FileItem> items;
    std::mutex mu;
    std::condition_variable cv;
    std::atomic<int64_t> next_read{0}, next_gpu{0}, next_walk{0};
    int64_t n_done = 0;                             // (under mu) items finished: bounds how far the readers run ahead
    int64_t window = 0;
    double sec[4] = {0, 0, 0, 0};                   // busy seconds summed over the items: read, upload (decode + pack), step, walk
    int64_t on[2] = {0, 0};                         // items decoded on the device / by the host reader
};

double seconds_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// the item has reached `state`: tell the stages that wait for it
template <class Book>
void advance(FileRun &q, FileItem &it, int state, Book book)
{
    {
        std::lock_guard<std::mutex> lk(q.mu);
        it.state = state;
        book();
    }
    q.cv.notify_all();
}

void wait_for(FileRun &q, const FileItem &it, int state)
{
    std::unique_lock<std::mutex> lk(q.mu);
    q.cv.wait(lk, [&] { return it.state >= state; });
}

// ---- read ------------------------------------------------------------------------------------------------------------------
void read_stage(FileRun &q)
{
    for (;;) {
        const int64_t i = q.next_read.fetch_add(1);
        if (i >= q.n) return;
        {
            std::unique_lock<std::mutex> lk(q.mu);
            q.cv.wait(lk, [&] { return i < q.n_done + q.window; });
        }
        const auto t0 = std::chrono::steady_clock::now();
        FileItem &it = q.items[(size_t)i];
        if (q.resident) it.file = q.resident[i];
        else if (q.device_decode) {
            // (several readers: two copy threads a file — with one, a reader needs 1.0 - 1.4 ms for a 7.7 MB file and three readers run
            //  close to the GPU's 0.42 ms per file: on a slower host the file leg fell to 55 - 66 M positions/s where two threads gave
            //  63 - 69 M, three turns each, profiles/r06l_read_threads_ab.log)
            it.rc = tcmi_bamfile_read_threads(q.paths[i], q.r->n_readers > 1 ? 2 : 0, &it.file);
            if (it.rc) it.err = tcmi_last_error(nullptr);
        }
        const double dt = seconds_since(t0);
        advance(q, it, 1, [&] { q.sec[0] += dt; });
    }
}

// ---- gpu -------------------------------------------------------------------------------------------------------------------
// one item on its way through a context: the read set, and where the step left its records (the context's buffers)
struct GpuStep {
    tcmi_readset *rs = nullptr;
    tcmi_host_reads host;               // the fallback's reads
    std::string host_err;               // ... and its words: it fails without a context
    bool want_cov = false;
    bool stepped = false;               // the device path queues decode, pack, tally and call back to back: ONE wait per file
    const uint8_t *pl = nullptr, *al = nullptr, *fl = nullptr;
    const int32_t *planes = nullptr;
    int64_t ld = 0, L = 0;
};

// a file that left the device path under a setting the host packer does not know: `flag` as the command line spells it
int refuse_host_packer(tcmi_ctx *ctx, const char *path, const std::string &flag, const char *unknown, bool was_read)
{
    const std::string why = was_read ? ctx->err : std::string("it was not read for the device decoder");
    return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "%s: %s needs the device path (the host packer knows no %s), which this file left: %s", path,
                     flag.c_str(), unknown, why.c_str());
}

// decode on the device and step there — or refuse — or let the host reader take the file: then s.rs is uploaded and not yet stepped
int gpu_decode(FileRun &q, tcmi_ctx *ctx, int64_t i, GpuStep &s)
{
    FileItem &it = q.items[(size_t)i];
    int rc = TCMI_E_UNSUPPORTED;
    if (it.file) {
        rc = tcmi_bamfile_step(ctx, it.file, q.ref_len, q.mincov, q.include_ambig, &s.rs, &s.L, &s.pl, &s.al, &s.fl, s.want_cov ? &s.planes : nullptr, &s.ld);
        it.on_device = s.stepped = rc == TCMI_OK;
        if (rc == TCMI_E_NOMEM) rc = TCMI_E_UNSUPPORTED;         // (a file whose decode does not fit the device's memory: the host reader streams it)
    }
    if (rc != TCMI_E_UNSUPPORTED) return rc;
    // ... but not under a base-quality floor: its packer knows none; nor under a primer table: its packer knows no mask; nor under the
    // mate-overlap rule: its packer joins no mates; nor under the duplicate rule: its packer finds no duplicate templates
    const tcmi_rule_beyond beyond = tcmi_rules_beyond_host(ctx->rules);
    if (beyond == TCMI_RULE_FLOOR) return refuse_host_packer(ctx, q.paths[i], "--min-baseq " + std::to_string((int)ctx->rules.min_bq), "base-quality floor", it.file != nullptr);
    if (beyond == TCMI_RULE_PRIMERS) return refuse_host_packer(ctx, q.paths[i], "--primers", "primer mask", it.file != nullptr);
    if (beyond == TCMI_RULE_MATE) return refuse_host_packer(ctx, q.paths[i], "--mate-overlap", "mate join", it.file != nullptr);
    if (beyond == TCMI_RULE_DEDUP) return refuse_host_packer(ctx, q.paths[i], "--dedup", "duplicate templates", it.file != nullptr);
    rc = s.host.load(q.paths[i], q.r->host_threads, ctx->rules.flt);   // (the context's read filter)
    if (rc) s.host_err = tcmi_last_error(nullptr);
    else rc = tcmi_readset_upload(ctx, &s.host.reads, &s.rs);
    return rc;
}

// the step of a read set that came from the host reader
int gpu_step_fallback(FileRun &q, tcmi_ctx *ctx, GpuStep &s)
{
    int64_t max_end = 0;
    tcmi_readset_info(s.rs, nullptr, nullptr, nullptr, nullptr, &max_end);
    s.L = std::max<int64_t>({q.ref_len, max_end, 1});
    return tcmi_step(ctx, s.rs, s.L, q.mincov, q.include_ambig, &s.pl, &s.al, &s.fl, s.want_cov ? &s.planes : nullptr, &s.ld);
}

// what the step left in the context's buffers, into the item: the coverage column, the variant records, the interval records (one
// slot each, where the run wants it), then the call records and their insert candidates
int gpu_copy_slots(FileRun &q, tcmi_ctx *ctx, int64_t i, const GpuStep &s)
{
    FileItem &it = q.items[(size_t)i];
    const OutFiles *f = q.files;
    const int64_t L = it.L = s.L;
    if (s.want_cov) it.cov.assign(s.planes + (size_t)TCMI_COV * s.ld, s.planes + (size_t)TCMI_COV * s.ld + L);
    if (f && f->wants(f->table, i)) {                            // the step's variant records, next to its call records
        const tcmi_variant *vr = nullptr;
        int64_t nv = 0;
        if (const int rc = tcmi_step_variants(ctx, &vr, &nv)) return rc;
        it.var.assign(vr, vr + nv);
    }
    if (f && f->stats) {                                         // ... and its amplicon records (one writer per item: no lock)
        const tcmi_interval_stat *ir = nullptr;
        int64_t ni = 0;
        if (const int rc = tcmi_step_intervals(ctx, &ir, &ni)) return rc;
        if (ni != f->n_intervals)
            return tcmi_fail(ctx, TCMI_E_ARG, "%s: the step computed %lld interval records, the run asked for %lld", q.paths[i], (long long)ni, (long long)f->n_intervals);
        std::memcpy(f->stats + (size_t)i * (size_t)ni, ir, (size_t)ni * sizeof(tcmi_interval_stat));
    }
    it.rec.resize((size_t)L * 3);
    std::memcpy(it.rec.data(), s.pl, (size_t)L);
    std::memcpy(it.rec.data() + L, s.al, (size_t)L);
    std::memcpy(it.rec.data() + 2 * L, s.fl, (size_t)L);
    tcmi_insert_candidates(s.fl, L, it.cand);
    return TCMI_OK;
}

// insert candidates of a BAM the device decoded: their tokens are voted on now, from the stream that is still resident in this
// context's arena (Events.py:47-82 without the reads ever reaching the host)
void gpu_vote(tcmi_ctx *ctx, const GpuStep &s, FileItem &it)
{
    if (!it.on_device || it.cand.empty()) return;
    int32_t st = 0;
    // pysam's defaults for AlignmentFile.pileup(), as walk_records.cpp passes them to the host sweep
    const int rt = tcmi_tokens_grow(ctx, it.cand.size(), it.pre, [&](char *text, int64_t cap) {
        return tcmi_readset_modal_tokens(ctx, s.rs, (int32_t)it.cand.size(), it.cand.data(), 13, 0x4 | 0x100 | 0x200 | 0x400, 1, 8000, 1, text, cap,
                                         it.pre.off.data(), it.pre.cnt.data(), &st);
    });
    // (anything the device path declines — megabytes of long insertions, an overlap it cannot resolve —
    // is left to the walker's host sweep, which words the refusal if it is one)
    it.pre.valid = rt == TCMI_OK && !(st & TCMI_TOKENS_OVERLAP_UNKNOWN);
}

void gpu_item(FileRun &q, tcmi_ctx *ctx, int64_t i, double *t_up, double *t_step)
{
    FileItem &it = q.items[(size_t)i];
    GpuStep s;
    s.want_cov = q.files && (q.files->wants(q.files->vcf, i) || q.files->wants(q.files->doc, i));
    const auto t0 = std::chrono::steady_clock::now();
    int rc = gpu_decode(q, ctx, i, s);
    *t_up = seconds_since(t0);
    const auto t1 = std::chrono::steady_clock::now();
    if (!rc && !s.stepped) rc = gpu_step_fallback(q, ctx, s);
    if (!rc) rc = gpu_copy_slots(q, ctx, i, s);
    if (!rc) gpu_vote(ctx, s, it);
    *t_step = seconds_since(t1);
    if (rc) { it.rc = rc; it.err = s.host_err.empty() ? tcmi_last_error(ctx) : s.host_err; }
    if (s.rs) tcmi_readset_free(ctx, s.rs);
}

void gpu_stage(FileRun &q, tcmi_ctx *ctx)
{
    for (;;) {
        const int64_t i = q.next_gpu.fetch_add(1);
        if (i >= q.n) return;
        FileItem &it = q.items[(size_t)i];
        wait_for(q, it, 1);
        double t_up = 0, t_step = 0;
        if (!it.rc) gpu_item(q, ctx, i, &t_up, &t_step);
        if (it.file && !q.resident) tcmi_bamfile_free(it.file);
        it.file = nullptr;
        advance(q, it, 2, [&] {
            q.sec[1] += t_up; q.sec[2] += t_step;
            if (!it.rc) q.on[it.on_device ? 0 : 1] += 1;
        });
    }
}

// ---- walk ------------------------------------------------------------------------------------------------------------------
// files mode: the four writers of Outputs.WriteOutputs / Coverage.BuildCoverage, in the reference's order: coverage TSV
// (TrueConsense.py:243-245), corrected GFF, VCF, FASTA — and the variant table in front of the FASTA.  fasta: the walk's text
int write_outputs(FileRun &q, int64_t i, const char *name, const tcmi_walk_extra &extra, const std::string &fasta)
{
    const FileItem &it = q.items[(size_t)i];
    const tcmi_filerunner *r = q.r;
    const OutFiles *f = q.files;
    std::string text, why;
    int rc = TCMI_OK;
    if (f->wants(f->doc, i)) { tcmi_coverage_tsv_text(it.cov.data(), it.L, text); rc = tcmi_write_file(f->doc[i], text, why); }
    if (!rc && f->wants(f->gff, i)) { tcmi_gff_text(r->gff_head, r->gff_cols, name, extra.new_start, extra.new_end, text); rc = tcmi_write_file(f->gff[i], text, why); }
    if (!rc && f->wants(f->vcf, i)) {
        rc = tcmi_vcf_text(r->vcf_head, r->ref_id, r->ref_seq, extra.cons_noinsert, it.cov.data(), it.L, q.mincov, extra.ins, text, why);
        if (!rc) rc = tcmi_write_file(f->vcf[i], text, why);
    }
    if (!rc && f->wants(f->table, i)) {
        text.assign(it.var.size() * (r->ref_id.size() + 96) + 1, '\0');
        int64_t tl = 0;
        rc = tcmi_variants_text(it.var.data(), (int64_t)it.var.size(), r->ref_id.c_str(), 0, reinterpret_cast<const uint8_t *>(r->ref_seq.data()),
                                (int64_t)r->ref_seq.size(), &text[0], (int64_t)text.size(), &tl);
        if (rc) return tcmi_fail(nullptr, rc, "%s: the variant records do not fit the reference of tcmi_filerunner_set_outputs", q.paths[i]);
        text.resize((size_t)tl);
        text.insert(0, TCMI_VARIANTS_HEADER);
        rc = tcmi_write_file(f->table[i], text, why);
        if (!rc && f->n_variants) f->n_variants[i] = (int64_t)it.var.size();
    }
    if (!rc && f->wants(f->fasta, i)) rc = tcmi_write_file(f->fasta[i], fasta, why);
    return rc ? tcmi_fail(nullptr, rc, "%s", why.c_str()) : TCMI_OK;     // (the writers know no tcmi_fail: their words, kept here)
}

void walk_item(FileRun &q, int64_t i)
{
    FileItem &it = q.items[(size_t)i];
    const OutFiles *f = q.files;
    const int64_t L = it.L;
    const uint8_t *pl = it.rec.data(), *al = pl + L, *fl = pl + 2 * L;
    tcmi_host_reads host;
    int rc = TCMI_OK;
    const bool sweep = !it.cand.empty() && !it.pre.valid;    // insert tokens that were not resolved on the device need the reads on the host
    // (the contexts' read filter — the caller sets the same one on all of them: the sweep sees passing records only)
    if (sweep) rc = host.load(q.paths[i], q.r->host_threads, q.r->ctxs[0]->rules.flt);
    const char *nm = q.names && q.names[i] ? q.names[i] : "sample";
    std::string own;                                         // files mode: the FASTA text lives here
    int64_t room = q.stride;
    char *dst = q.out_text ? q.out_text + i * q.stride : nullptr;
    if (f) { room = L + (int64_t)std::strlen(nm) + (1 << 16); own.resize((size_t)room); dst = &own[0]; }
    const int head = std::snprintf(dst, (size_t)room, ">%s mincov=%d\n", nm, (int)q.mincov);
    int64_t len = 0;
    tcmi_walk_extra extra;
    const bool want_extra = f && (f->wants(f->vcf, i) || f->wants(f->gff, i));
    if (!rc && (head < 0 || head + 2 >= room)) rc = tcmi_fail(nullptr, TCMI_E_ARG, "output stride too small");
    if (!rc) rc = tcmi_walk_records(pl, al, fl, L, it.cand, sweep ? &host.reads : nullptr, &it.pre, q.r->orfs, dst + head, room - head - 1, &len,
                                    (long long)i, want_extra ? &extra : nullptr);
    if (!rc) { dst[head + len] = '\n'; q.out_len[i] = head + len + 1; }
    if (!rc && f) { own.resize((size_t)q.out_len[i]); rc = write_outputs(q, i, nm, extra, own); }
    if (rc) { it.rc = rc; it.err = tcmi_last_error(nullptr); }
    std::vector<uint8_t>().swap(it.rec);
}

void walk_stage(FileRun &q)
{
    for (;;) {
        const int64_t i = q.next_walk.fetch_add(1);
        if (i >= q.n) return;
        FileItem &it = q.items[(size_t)i];
        wait_for(q, it, 2);
        const auto t0 = std::chrono::steady_clock::now();
        q.out_len[i] = 0;
        if (!it.rc) walk_item(q, i);
        q.status[i] = it.rc;
        const double dt = seconds_since(t0);
        advance(q, it, 3, [&] { ++q.n_done; q.sec[3] += dt; });
    }
}

// ---- one call ----------------------------------------------------------------------------------------------------------------
// stage_seconds[4], decoded_on[2] (either may be NULL): q.sec, q.on.  -> the first failing item's code, worded "path: its words"
int run(FileRun &q, double *stage_seconds, int64_t *decoded_on)
{
    tcmi_filerunner *r = q.r;
    const int64_t n = q.n;
    if (!r || n < 0 || (n > 0 && ((!q.paths && !q.resident) || !q.status || (!q.files && (!q.out_text || !q.out_len))))) return tcmi_fail(nullptr, TCMI_E_ARG, "null argument");
    std::vector<const char *> own_paths;
    if (q.resident) {
        for (int64_t i = 0; i < n; ++i) {
            if (!q.resident[i]) return tcmi_fail(nullptr, TCMI_E_ARG, "null file");
            own_paths.push_back(tcmi_bamfile_path(q.resident[i]));
        }
        q.paths = own_paths.data();
    }
    std::vector<int64_t> len_store;
    if (!q.out_len) { len_store.assign((size_t)n, 0); q.out_len = len_store.data(); }
    q.items = std::vector<FileItem>((size_t)n);
    q.window = (int64_t)r->n_readers + (int64_t)r->ctxs.size() + r->n_walkers + 2;
    std::vector<std::thread> th;
    for (int k = 0; k < r->n_readers; ++k) th.emplace_back(read_stage, std::ref(q));
    for (auto *c : r->ctxs) th.emplace_back(gpu_stage, std::ref(q), c);
    for (int k = 0; k < r->n_walkers; ++k) th.emplace_back(walk_stage, std::ref(q));
    for (auto &t : th) t.join();
    if (stage_seconds) for (int k = 0; k < 4; ++k) stage_seconds[k] = q.sec[k];
    if (decoded_on) { decoded_on[0] = q.on[0]; decoded_on[1] = q.on[1]; }
    for (int64_t i = 0; i < n; ++i)
        if (q.items[(size_t)i].rc) return tcmi_fail(nullptr, q.items[(size_t)i].rc, "%s: %s", q.paths[i], q.items[(size_t)i].err.c_str());
    return TCMI_OK;
}

// the arguments every entry point passes on as they are
void common_args(FileRun &q, tcmi_filerunner *r, int64_t n, const char *const *names, int64_t ref_len, int32_t mincov, int include_ambig, int32_t *status)
{
    q.r = r; q.n = n; q.names = names; q.ref_len = ref_len; q.mincov = mincov; q.include_ambig = include_ambig; q.status = status;
}

} // namespace

extern "C" {

int tcmi_filerunner_create(int device, int n_readers, int n_gpu, int n_walkers, int host_decode_threads, tcmi_filerunner **out)
{
    if (!out || n_readers < 1 || n_readers > 64 || n_gpu < 1 || n_gpu > 16 || n_walkers < 1 || n_walkers > 64)
        return tcmi_fail(nullptr, TCMI_E_ARG, "need 1..64 readers, 1..16 gpu contexts, 1..64 walkers");
    *out = nullptr;
    tcmi_filerunner *r = new tcmi_filerunner();
    r->device = device; r->n_readers = n_readers; r->n_walkers = n_walkers; r->host_threads = host_decode_threads > 0 ? host_decode_threads : 8;
    for (int k = 0; k < n_gpu; ++k) {
        tcmi_ctx *c = nullptr;
        const int rc = tcmi_ctx_create(device, &c);
        if (rc) {
            for (auto *x : r->ctxs) tcmi_ctx_destroy(x);
            delete r;
            return rc;
        }
        r->ctxs.push_back(c);
    }
    *out = r;
    return TCMI_OK;
}

int tcmi_filerunner_destroy(tcmi_filerunner *r)
{
    if (!r) return TCMI_OK;
    for (auto *c : r->ctxs) tcmi_ctx_destroy(c);
    delete r;
    return TCMI_OK;
}

int tcmi_filerunner_set_orfs(tcmi_filerunner *r, int32_t n_orf, const int64_t *start, const int64_t *end, const uint8_t *is_plus)
{
    return tcmi_orfs_assign(r ? &r->orfs : nullptr, n_orf, start, end, is_plus);
}

tcmi_ctx *tcmi_filerunner_ctx(tcmi_filerunner *r, int k) { return (r && k >= 0 && k < (int)r->ctxs.size()) ? r->ctxs[(size_t)k] : nullptr; }

int tcmi_filerunner_run(tcmi_filerunner *r, int64_t n, const char *const *paths, const char *const *names, int64_t ref_len,
                        int32_t mincov, int include_ambig, int device_decode, char *out_text, int64_t stride, int64_t *out_len,
                        int32_t *status, double *stage_seconds, int64_t *decoded_on)
{
    FileRun q;
    common_args(q, r, n, names, ref_len, mincov, include_ambig, status);
    q.paths = paths; q.device_decode = device_decode; q.out_text = out_text; q.stride = stride; q.out_len = out_len;
    return run(q, stage_seconds, decoded_on);
}

// ... of files that were read before (tcmi_bamfile_read) and stay the caller's: the read stage has nothing to do.  With their bytes
// in HBM (tcmi_bamfile_to_device) the GPU stage starts from device memory — no PCIe copy inside the run.
int tcmi_filerunner_run_resident(tcmi_filerunner *r, int64_t n, tcmi_bamfile *const *files, const char *const *names, int64_t ref_len,
                                 int32_t mincov, int include_ambig, char *out_text, int64_t stride, int64_t *out_len, int32_t *status,
                                 double *stage_seconds, int64_t *decoded_on)
{
    if (!files && n > 0) return tcmi_fail(nullptr, TCMI_E_ARG, "null argument");
    FileRun q;
    common_args(q, r, n, names, ref_len, mincov, include_ambig, status);
    q.resident = files; q.out_text = out_text; q.stride = stride; q.out_len = out_len;
    return run(q, stage_seconds, decoded_on);
}

// What the VCF and GFF writers need besides a sample's walk: the reference (first FASTA record: id and sequence, Outputs.py:108-113),
// the complete VCF header text (Outputs.py:115-127: date, command line and reference path are the caller's), the GFF header text
// and, per GFF row, its columns other than seqid / start / end: source, type, score, strand, phase, attributes (6 strings per row,
// the attributes folded as Outputs.py:32-58 folds them).
int tcmi_filerunner_set_outputs(tcmi_filerunner *r, const char *ref_id, const char *ref_seq, const char *vcf_head, const char *gff_head,
                                int32_t n_rows, const char *const *row_cols)
{
    if (!r || !ref_id || !ref_seq || !vcf_head || !gff_head || n_rows < 0 || (n_rows > 0 && !row_cols)) return tcmi_fail(nullptr, TCMI_E_ARG, "null argument");
    if ((size_t)n_rows != r->orfs.size()) return tcmi_fail(nullptr, TCMI_E_ARG, "%d GFF rows, %zu ORFs set", (int)n_rows, r->orfs.size());
    r->ref_id = ref_id; r->ref_seq = ref_seq; r->vcf_head = vcf_head; r->gff_head = gff_head;
    r->gff_cols.clear();
    for (int32_t k = 0; k < 6 * n_rows; ++k) r->gff_cols.emplace_back(row_cols[k] ? row_cols[k] : "");
    return TCMI_OK;
}

// BAM files -> the command line's four output FILES per sample (TrueConsense.py:212-264 with -o, -vcf, -ogff, -doc), same stages
// and overlap as tcmi_filerunner_run; the walker threads also write the VCF, the corrected GFF and the coverage TSV (no Python
// per sample).  Any of vcf / gff / doc, or single entries of them, may be NULL.  tcmi_filerunner_set_outputs first.
int tcmi_filerunner_run_files(tcmi_filerunner *r, int64_t n, const char *const *paths, const char *const *names, const char *const *fasta,
                              const char *const *vcf, const char *const *gff, const char *const *doc, int64_t ref_len, int32_t mincov,
                              int include_ambig, int device_decode, int32_t *status, double *stage_seconds, int64_t *decoded_on)
{
    if (!r || !fasta) return tcmi_fail(nullptr, TCMI_E_ARG, "null argument");
    if ((vcf || gff) && r->gff_cols.size() != 6 * r->orfs.size()) return tcmi_fail(nullptr, TCMI_E_ARG, "tcmi_filerunner_set_outputs first");
    const OutFiles f = {fasta, vcf, gff, doc, nullptr, nullptr, 0, nullptr};
    FileRun q;
    common_args(q, r, n, names, ref_len, mincov, include_ambig, status);
    q.paths = paths; q.device_decode = device_decode; q.files = &f;
    return run(q, stage_seconds, decoded_on);
}

// ... and per sample (an array or an entry may be NULL) its variant table: the runner's contexts carry the setting (tcmi_ctx_set_variants
// through tcmi_filerunner_ctx, the same on all of them), the GPU stage copies the step's records next to the call records, the walker
// writes the file with tcmi_variants_text — REGION and REF from tcmi_filerunner_set_outputs' reference.  A sample that went to the
// host-reader fallback gets its table too: its step goes through tcmi_step.  n_variants (may be NULL): the records written per sample.
int tcmi_filerunner_run_files_table(tcmi_filerunner *r, int64_t n, const char *const *paths, const char *const *names, const char *const *fasta,
                                    const char *const *vcf, const char *const *gff, const char *const *doc, const char *const *table, int64_t ref_len,
                                    int32_t mincov, int include_ambig, int device_decode, int32_t *status, double *stage_seconds, int64_t *decoded_on,
                                    int64_t *n_variants)
{
    return tcmi_filerunner_run_files_stats(r, n, paths, names, fasta, vcf, gff, doc, table, ref_len, mincov, include_ambig, device_decode, status,
                                           stage_seconds, decoded_on, n_variants, 0, nullptr);
}

// ... and the amplicon table's records: the runner's contexts carry the setting (tcmi_ctx_set_intervals, the same n_intervals on all of
// them), the GPU stage copies the step's records into stats[i * n_intervals ...).  A sample that went to the host-reader fallback gets
// its records too: its step goes through tcmi_step.  The table's text is the caller's (tcmi_amplicons_text).
int tcmi_filerunner_run_files_stats(tcmi_filerunner *r, int64_t n, const char *const *paths, const char *const *names, const char *const *fasta,
                                    const char *const *vcf, const char *const *gff, const char *const *doc, const char *const *table, int64_t ref_len,
                                    int32_t mincov, int include_ambig, int device_decode, int32_t *status, double *stage_seconds, int64_t *decoded_on,
                                    int64_t *n_variants, int64_t n_intervals, tcmi_interval_stat *stats)
{
    if (!r || !fasta) return tcmi_fail(nullptr, TCMI_E_ARG, "null argument");
    if ((vcf || gff || table) && r->gff_cols.size() != 6 * r->orfs.size()) return tcmi_fail(nullptr, TCMI_E_ARG, "tcmi_filerunner_set_outputs first");
    bool any = false;
    for (int64_t i = 0; table && i < n; ++i) any = any || table[i];
    if (any && r->ref_seq.empty())                              // (the rows' REGION and REF; the GFF rows above may be none at all)
        return tcmi_fail(nullptr, TCMI_E_ARG, "a variant table is asked for: tcmi_filerunner_set_outputs (the reference's id and sequence) first");
    for (const tcmi_ctx *c : r->ctxs)
        if (any && !tcmi_var_table_on(c)) return tcmi_fail(nullptr, TCMI_E_ARG, "a variant table is asked for: tcmi_ctx_set_variants on every context of the runner first");
    for (int64_t i = 0; n_variants && i < n; ++i) n_variants[i] = 0;
    if (n_intervals < 0 || (n_intervals > 0) != (stats != nullptr)) return tcmi_fail(nullptr, TCMI_E_ARG, "n_intervals and stats go together");
    for (const tcmi_ctx *c : r->ctxs)
        if (stats && (!tcmi_iv_table_on(c) || tcmi_iv_table_n(c) != n_intervals))
            return tcmi_fail(nullptr, TCMI_E_ARG, "amplicon records are asked for: tcmi_ctx_set_intervals with %lld intervals on every context of the runner first", (long long)n_intervals);
    if (stats && n > 0) std::memset(stats, 0, (size_t)n * (size_t)n_intervals * sizeof(tcmi_interval_stat));
    const OutFiles f = {fasta, vcf, gff, doc, table, n_variants, n_intervals, stats};
    FileRun q;
    common_args(q, r, n, names, ref_len, mincov, include_ambig, status);
    q.paths = paths; q.device_decode = device_decode; q.files = &f;
    return run(q, stage_seconds, decoded_on);
}

} // extern "C"
