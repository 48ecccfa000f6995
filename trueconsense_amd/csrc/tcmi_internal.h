// tcmi_internal.h — shared between the translation units of libtcmi.so (not installed).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <functional>
#include <memory>
#include <vector>

#include "../../include/tcmi.h"
#include "variants_rule.h"           // the variant table's rule (GPU-free; shared with the host checks)
#include "readset_layout.h"          // tcmi_layout, the packed read set (TCMI_F_* / TCMI_P_*, tcmi_fast_chunk), the chunk geometry
#include "pack_caps.h"               // the device packer's decline flags, capacities and arena scratch (GPU-free; shared with the host checks)

// checks n_ref / shift / slot_len (slots in ascending order, disjoint, below TCMI_F_EVPOS) and fills *out; TCMI_OK or TCMI_E_ARG
int tcmi_layout_build(int32_t n_ref, const int64_t *shift, const int64_t *slot_len, tcmi_layout *out, char *msg, size_t msg_cap);

// ---- read filter (tcmi_ctx_set_read_filter, tcmi_bam_filter) ------------------------------------------------------------
// A record passes iff mapq >= min_mapq, (flag & require) == require, (flag & exclude) == 0; a failing record is ignored wherever an
// unmapped one is.  The one rule of the kernels (pack_device.h: passes) and of the host reader's compaction (bam_reader.cpp).
struct tcmi_read_filter {
    uint32_t min_mapq, require, exclude;
};
static inline bool tcmi_filter_on(const tcmi_read_filter &f) { return (f.min_mapq | f.require | f.exclude) != 0; }
static inline bool tcmi_filter_pass(const tcmi_read_filter &f, uint32_t flag, uint32_t mapq)
{
    return mapq >= f.min_mapq && (flag & f.require) == f.require && (flag & f.exclude) == 0;
}
// ... as the kernels take it, two uniform words of their arguments (pk_index has no scalar register to spare): the flag bits that are
// tested and the value they must have — (flag & mask) == want with mask = require | exclude, want = require — and the MAPQ bound; a
// filter that requires and excludes the same bit passes nothing: MAPQ bound 256.  No filter: both words 0.
struct tcmi_filter_words {
    uint32_t flags;                 // mask | want << 16
    uint32_t min_mapq;
};
static inline tcmi_filter_words tcmi_filter_pack(const tcmi_read_filter &f)
{
    tcmi_filter_words w;
    w.flags = ((f.require | f.exclude) & 0xFFFFu) | ((f.require & 0xFFFFu) << 16);
    w.min_mapq = (f.require & f.exclude) ? 256u : f.min_mapq;
    return w;
}
// the argument check of both entry points: TCMI_OK and *out filled, or TCMI_E_ARG (worded on `ctx`)
int tcmi_read_filter_build(tcmi_ctx *ctx, int32_t min_mapq, uint32_t require_flags, uint32_t exclude_flags, tcmi_read_filter *out);

// ---- amplicon primer mask (tcmi_ctx_set_primers; primer_table.h compiles the table) ----------------------------------------
// The compiled table on the device, shared by the context that set it, its sub-range helper contexts and every read set built under
// it (tally_stream_kernel masks a read set's long reads at tally time): freed with its last owner.  seg: int32 [3 * (n_head + n_tail)],
// the head list as a[n_head] | b[n_head] | v[n_head] (a binary search walks one dense array), the tail list behind it likewise.
struct tcmi_primer_dev {
    int32_t *seg = nullptr;
    int32_t n_head = 0, n_tail = 0, n_primers = 0;
    ~tcmi_primer_dev() { if (seg) (void)hipFree(seg); }
};
// ... as the kernels take it: a trailing kernel argument / the tail of FusedArgs (tcmi_pack_src is full).  No table: all zero.
// clip (tcmi_ctx_set_mate_overlap; null: the setting is off): per record of the decoded stream, the columns at its head that its mate
// counts (mate_join.hip) — it travels with the table because it masks the same tokens, a head_end of its own.
struct tcmi_primer_tab {
    const int32_t *seg;
    int32_t n_head, n_tail;
    const uint32_t *clip;
};
static inline tcmi_primer_tab tcmi_primer_args(const std::shared_ptr<const tcmi_primer_dev> &p)
{
    tcmi_primer_tab t = {nullptr, 0, 0, nullptr};
    if (p) { t.seg = p->seg; t.n_head = p->n_head; t.n_tail = p->n_tail; }
    return t;
}

// ---- the read rules ------------------------------------------------------------------------------------------------------
// Which tokens of a BAM reach the count matrix: the read filter (tcmi_ctx_set_read_filter), the base-quality floor
// (tcmi_ctx_set_min_base_quality; 0: none), the primer table (tcmi_ctx_set_primers; null: none) and the mate-overlap rule
// (tcmi_ctx_set_mate_overlap; 0: off) and the duplicate rule (tcmi_ctx_set_dedup; 0: off).  One record on the context (what its next read set is built under) and one on every read set
// (what it was built under); tcmi_rules_stamp hands it from the one to the other, tcmi_rules_args to the kernels' arguments.
struct tcmi_read_rules {
    tcmi_read_filter flt = {0, 0, 0};
    int32_t min_bq = 0;
    std::shared_ptr<const tcmi_primer_dev> primers;
    int32_t mate = 0;
    int32_t dedup = 0;
};
// the first rule that is beyond the host packer and the flat arrays of struct tcmi_reads (no QUAL, no mask, no names): the entry
// points that lead there refuse under it, each in its own words, the floor before the table before the mate rule before the duplicate rule
// (the filter they know)
enum tcmi_rule_beyond { TCMI_RULE_NONE = 0, TCMI_RULE_FLOOR, TCMI_RULE_PRIMERS, TCMI_RULE_MATE, TCMI_RULE_DEDUP };
static inline tcmi_rule_beyond tcmi_rules_beyond_host(const tcmi_read_rules &r)
{
    return r.min_bq > 0 ? TCMI_RULE_FLOOR : r.primers ? TCMI_RULE_PRIMERS : r.mate ? TCMI_RULE_MATE : r.dedup ? TCMI_RULE_DEDUP : TCMI_RULE_NONE;
}
// ... as the kernels take the filter and the floor: `flt` and `min_bq` of tcmi_pack_src and of the one-sync packer's arguments
template <class Args> static inline void tcmi_rules_args(Args &a, const tcmi_read_rules &r) { a.flt = tcmi_filter_pack(r.flt); a.min_bq = (uint32_t)r.min_bq; }

struct tcmi_readset;
static inline tcmi_primer_tab tcmi_mask_args(const tcmi_readset *rs);   // the table and the clip a read set was built under (below)

struct tcmi_readset {
    uint64_t uid = 0;           // unique per upload (graphs are cached against it, not the pointer)
    int64_t n_reads = 0;        // as handed in
    int64_t n_piled = 0;        // kept on device (aligned + general)
    int64_t alg_bytes = 0;      // sum over kept reads of 12 + 4*n_cigar + ceil(l_qseq/2)
    int64_t dev_bytes = 0;
    int64_t max_end = 0;        // max end position (exclusive) of a kept read
    int32_t max_len = 0;        // device-packed sets: the longest reference span of a kept read (0: not recorded)
    int device = -1;
    int packed_on_device = 0;   // 1: pack_device.hip built the aligned set (everything below lives in d_blob)
    // device-decoded read sets: the inflated stream and the packer's index stay in the context's arena until its next upload
    // (arena_epoch tells): the insert-token kernel reads qualities, inserted bases, names and mate fields from there
    const uint8_t *d_stream = nullptr;
    const uint64_t *d_rec_off = nullptr;
    const uint32_t *d_cidx = nullptr;
    const int32_t *d_cpos = nullptr;
    // uploaded under a contig layout: its size, the device table (tally_stream_kernel shifts the long reads with it) and the kept
    // reads' max end per reference, in the reference's own coordinates (tcmi_readset_ref_extents)
    int32_t n_lay = 0;
    const int32_t *d_lay = nullptr;
    uint64_t lay_gen = 0;           // the context's layout generation at the upload (the device table is rewritten by the next layout)
    std::vector<int64_t> ref_ext;
    int64_t n_dropped = 0;          // mapped reads on references without a slot (tcmi_readset_dropped)
    // built from a device-decoded record stream: the rules this set was built under — the kernels that walk the resident stream
    // afterwards apply them whatever the context is set to later (stream_src, tcmi_mask_args) — and what the build made of them:
    // the records that failed the filter (tcmi_readset_filtered); under any of the other three the aligned set's third plane, d_fdrop: one
    // word per {lo, hi} pair of d_fseq (index = word / 2), bit b set when that read's token on that column is skipped; the kept reads
    // with a non-empty head or tail mask (tcmi_readset_primers); under the mate rule d_clip [n_reads], in the context's arena beside
    // the stream (arena_epoch tells), and the join's four counters (tcmi_readset_mate_overlap); under the duplicate rule d_clip likewise
    // (a duplicate's clip is its span), d_dup [n_reads] beside it (tcmi_readset_duplicates) and dedup.hip's four counters
    tcmi_read_rules rules;
    int64_t n_filtered = 0;
    int64_t n_masked = 0;
    const uint32_t *d_clip = nullptr;
    int64_t mate_stat[4] = {0, 0, 0, 0};    // pairs, clipped reads, clipped columns, ambiguous records
    const uint8_t *d_dup = nullptr;
    int64_t dup_stat[4] = {0, 0, 0, 0};     // templates, duplicate templates, duplicate records, duplicate sets
    const uint32_t *d_gen_idx = nullptr;   // records of reads too long for the packed set (s_reads of them): tally_stream_kernel walks them in the stream
    int64_t s_reads = 0;
    // a read set of a block RANGE of a file (tcmi_readset_from_bamfile_blocks): where its first record starts when the range began
    // in the middle of the file (nothing in front of it vouches for that start), and where the first record behind the range starts —
    // offsets into the WHOLE file's inflated stream, -1: none.  The range in front must end where this one starts
    // (tcmi_readset_range_anchors; tcmi_split_step sums the differences along with the counts).
    int64_t range_first = -1, range_next = -1;
    uint64_t arena_epoch = 0;
    // the one-sync file path (bam_device.hip, tcmi_bamfile_step): the packer's totals have not been read back yet — f_chunks and
    // f_events hold the CAPACITIES, the tally kernel takes the real counts from here ({n_chunks, n_events} in the context's arena)
    const uint32_t *d_dev_counts = nullptr;
    char *d_blob = nullptr;     // one allocation holding d_flenoff | d_fseq | d_fchunk | d_fcovrun | d_fevent
    size_t blob_bytes = 0;
    // aligned set
    int64_t f_reads = 0, f_chunks = 0, f_words = 0, f_events = 0;
    uint32_t *d_flenoff = nullptr; // [f_reads] the packed header words
    uint32_t *d_fseq = nullptr; // [f_words]
    uint32_t *d_fevent = nullptr;// [f_events] position | TCMI_F_EV_*: tokens that are not plain A/C/G/T bases
    tcmi_fast_chunk *d_fchunk = nullptr;   // [f_chunks]
    uint32_t *d_fcovrun = nullptr;         // coverage runs of all chunks (tcmi_fast_chunk::run0 / n_runs)
    uint32_t *d_fdrop = nullptr;           // [f_words / 2] the drop plane (a floor, a primer table or the mate rule; in d_blob behind the events)
    // general set
    int64_t g_reads = 0, n_rounds = 0, n_cigar = 0, n_seqw = 0;
    int32_t *d_pos = nullptr;   // [g_reads]
    uint32_t *d_meta = nullptr; // [g_reads] flag<<16 | n_cigar
    int32_t *d_lseq = nullptr;  // [g_reads]
    uint32_t *d_cigar = nullptr;// [n_cigar]
    uint32_t *d_seq = nullptr;  // [n_seqw] 8 bases per word, base i at bits [4(i%8), +4), raw BAM codes
    int64_t *d_round_cig = nullptr; // [n_rounds+1]
    int64_t *d_round_seq = nullptr; // [n_rounds+1]
    // A rank's block range decoded as several SUB-RANGES side by side (tcmi_split_step, "split_sub"): this read set is then only the
    // sum of its parts — each a read set of its own on a context of its own (its decoded stream lives in that context's arena) — in
    // file order.  It answers tcmi_readset_info / _range_anchors / _ins_entries / tcmi_tally_dev / tcmi_readset_free.
    struct Part { tcmi_ctx *cx; tcmi_readset *rs; };
    std::vector<Part> parts;
};

static inline tcmi_primer_tab tcmi_mask_args(const tcmi_readset *rs)
{
    tcmi_primer_tab t = tcmi_primer_args(rs->rules.primers);
    t.clip = rs->rules.mate || rs->rules.dedup ? rs->d_clip : nullptr;
    return t;
}

struct tcmi_ride {                  // a finished matrix waiting for its call (see tally_common.h, call_other_tile)
    int32_t *counts; int64_t ld, L; int32_t mincov; int amb; uint8_t *plain, *alt, *flags; bool taken;
};

struct tcmi_host_packed;                 // what the host packer made of the last upload, its buffers kept between calls (host_pack.h)
void tcmi_host_packed_free(tcmi_host_packed *p);
struct tcmi_dev_arena {                  // grow-only device scratch of a context (freed with it): the BAM decoder's and the packers' temporaries (api.cpp)
    char *base = nullptr;
    size_t cap = 0, used = 0;
};

// ---- the per-step tables (tables.cpp): settings of a context under which every tcmi_step_begin launches the table's kernels between
// the tally and the call (both only read the matrix), their records going to pinned memory the setting owns, fetched after
// tcmi_step_end.  on: the setting is set; in_step: the step under way (step_L > 0) computes the table; valid: the last ended step did.
// release(): the setting's buffers, for the setter that replaces the setting (nothing queued uses them any more) and for teardown.
// The variant table (variants.hip): a device copy of the reference on the matrix's axis and the rule; h_rec holds 5 * n_ref records,
// n of them valid.  Kept from setting to setting and shared with tcmi_variants_dev, grow-only: d_scr, blk_base | blk_cnt of the
// launches for scr_blocks workgroups, and h_tot (pinned), the totals the scan kernel writes, [0] a step's, [1] tcmi_variants_dev's.
struct tcmi_var_table {
    bool on = false, in_step = false, valid = false;
    tcmi_var_rule rule = {0, 1, 1, 0};
    uint8_t *d_ref = nullptr;
    int64_t n_ref = 0, n = 0;
    tcmi_variant *h_rec = nullptr;
    char *d_scr = nullptr;
    int64_t scr_blocks = 0;
    unsigned long long *h_tot = nullptr;
    void release() { if (d_ref) (void)hipFree(d_ref); if (h_rec) (void)hipHostFree(h_rec); d_ref = nullptr; h_rec = nullptr; n_ref = 0; on = valid = false; }
};
// The amplicon table (intervals.hip): a device copy of n intervals (d_iv: the starts, then the ends) and the bound; h_rec holds n records.
struct tcmi_iv_table {
    bool on = false, in_step = false, valid = false;
    int64_t n = 0;
    int32_t min_depth = 0;
    int64_t *d_iv = nullptr;
    tcmi_interval_stat *h_rec = nullptr;
    void release() { if (d_iv) (void)hipFree(d_iv); if (h_rec) (void)hipHostFree(h_rec); d_iv = nullptr; h_rec = nullptr; n = 0; on = valid = false; }
};

struct tcmi_ctx {
    int device = -1;
    tcmi_host_packed *host_packed = nullptr;
    tcmi_dev_arena dev_arena;
    uint64_t arena_epoch = 0;        // bumped whenever the arena is handed out anew
    // device-packed read sets hand their allocation back when they are freed; the next upload of a similar size takes it
    // (hipMalloc + hipFree cost more than the pack kernels, and hipFree waits for the device)
    struct Blob { char *p; size_t bytes; };
    std::vector<Blob> blob_pool;
    // the contig layout of tcmi_ctx_set_layout (host form) and its device table {shift[n], end[n], ext[n]} (int32): one grow-only
    // buffer, rewritten by every layout; lay_gen counts the rewrites (a read set's long reads need the table it was uploaded under)
    tcmi_layout layout;
    int32_t *d_lay = nullptr;
    size_t d_lay_cap = 0;
    uint64_t lay_gen = 0;
    // scratch of tcmi_readset_modal_tokens (columns, ranges, entries): device + pinned host, grow-only
    char *tok_dev = nullptr, *tok_host = nullptr;
    size_t tok_dev_cap = 0, tok_host_cap = 0;
    // scratch that the counting calls over the record stream share (stream_count.h; tcmi_readset_amplicon_reads: the compiled table, the
    // counters; tcmi_readset_strand_counts and tcmi_readset_link_counts: the columns, the counters; tcmi_readset_indel_events: the columns,
    // the totals, the keyed table, the event list and its text; tcmi_readset_evidence_counts: the columns, the counters): device, grow-only; its host side is h_pin.  Every such call waits for
    // the stream before it returns.
    char *count_dev = nullptr;
    size_t count_dev_cap = 0;
    // small read-backs of the cold path (block verdicts, packer totals) land in pinned memory of the context: a copy into pageable
    // memory makes the runtime pin and unpin the destination's pages on every call
    char *h_pin = nullptr;
    size_t h_pin_cap = 0;
    char *h_desc = nullptr;          // pinned: the re-based block table of a block range on its way to the device (bam_device.hip: decode_enqueue)
    size_t h_desc_cap = 0;
    // the read rules (above; their four setters): they govern the read sets built from device-decoded record streams.  The flat-array
    // entry points refuse under a floor, a table or the mate rule (tcmi_rules_beyond_host); block ranges and tcmi_split_step refuse
    // under the mate rule too (a mate may lie outside)
    tcmi_read_rules rules;
    tcmi_var_table var;              // tcmi_ctx_set_variants
    tcmi_iv_table iv;                // tcmi_ctx_set_intervals
    int verify_crc = 1;              // the device decoder checks the BGZF CRC-32 of every block
    int64_t stat_one_sync_taken = 0, stat_one_sync_declined = 0, stat_one_sync_retried = 0, stat_last_decline = 0;     // tcmi_ctx_stat
    int64_t stat_h2d_piped = 0;      // decodes whose compressed bytes crossed PCIe in pieces, ahead of the inflate kernels (bam_device.hip: decode_enqueue)
    int64_t stat_dup[4] = {0, 0, 0, 0};      // dedup.hip's counters, likewise (tcmi_ctx_stat "dedup_templates", ...)
    int64_t stat_mate[4] = {0, 0, 0, 0};     // the mate join's counters, summed over the read sets this context built (tcmi_ctx_stat "mate_pairs", ...)
    int64_t stat_split_sub = 0;      // tcmi_split_step calls whose range went through sub-ranges
    int64_t stat_decode_batched = 0; // files the device decoder took in batches of blocks (tcmi_ctx_stat "decode_batched")
    // tcmi_readset_indel_events (indel_events.hip): log2 of the device table's first size and the bits of an insertion's hash that are
    // kept (options "indel_slots", "indel_hash_bits", for tests); attempts that started over with a larger table / the next seed
    int indel_slots = 15, indel_hash_bits = 34;
    int64_t stat_indel_grown = 0, stat_indel_retried = 0;
    int32_t split_tail[6] ={0, 0, 0, 0, 0, 0};   // tcmi_split_step: this rank's slot of the range table on its way to the device (the copy is asynchronous)
    uint32_t rec_bytes_seen = 0;     // mean record size of the last file this context decoded (sizes the next file's arrays when the file's own first blocks say nothing)
    int64_t decode_token_mb = 4096;  // bam_device.hip decode_enqueue: the token scratch's size; files that need more are decoded in batches of blocks
    int prefix_kernels = 0;          // pk_index / pk_place take the sums in front of a block from scan launches: 0 = from 16 384 blocks on, 1 = always, -1 = never
    int mid_wait = 0;                // 1: the one-sync path waits once more, behind the decode kernels (bam_device.hip: fast_enqueue); default since round 5: ONE wait per file
    int one_sync = 1;                // device-decoded files take the one-sync path (pk_index + pk_place + pk_pack) first; 0: the several-kernel path only
    int device_pack = 1;             // tcmi_readset_upload packs on the device when the input allows it
    int n_cu = 256;                  // compute units of the device
    int wg_per_cu = TCMI_P_WAVES;    // resident workgroups per CU of the tally kernel (its register budget)
    int balance_chunks = 1;          // size the chunks so that their number is a multiple of the resident workgroups
    hipStream_t stream = nullptr;
    bool own_stream = true;
    // Two streams per context (TCMI_STREAM_SPLIT, api.cpp ctx_create): the inflate kernels of a file stay on `stream_lo`, everything
    // behind them (pk_index .. pk_report: short kernels that triple in duration next to a chip full of bgzf_copy workgroups) goes to
    // `stream_hi` — a higher priority, or compute units of its own.  `stream` is the one the launches use at the moment.
    // tcmi_split_step: a rank's block range is decoded as `split_sub` sub-ranges side by side (0 = auto: a true range of a larger file: three from 6 144 blocks on, two
    // from 4 096; the whole file: one), the first on this context, the others on helper contexts this one owns (a stream and an arena each)
    int split_sub = 0;
    std::vector<tcmi_ctx *> helpers;
    // ... started one behind the other: a sub-range's first inflate kernel waits for the bgzf_symbols of the sub-range in front (an event), so
    // that the sub-ranges run skewed — symbols of k + 1 under copy of k under pack of k - 1 — instead of in step (bgzf_copy.hip:
    // tcmi_bgzf_decode_launch records `ev_after_sym` and calls `after_sym` once per decode)
    int sym_scratch_div = 1;         // option "sym_scratch_div" (tests): bgzf_symbols' lanes park 1 / n of their share before they overflow (pass B)
    int h2d_pieces = 0;              // option "h2d_pieces": 0 / -1 = one copy (default), n = n pieces
    hipStream_t copy_stream = nullptr;           // H2D of a large file's / range's compressed bytes in pieces (decode_enqueue)
    std::vector<hipEvent_t> ev_piece;
    hipEvent_t ev_before_sym = nullptr, ev_after_sym = nullptr;
    std::function<void()> after_sym;
    hipStream_t stream_lo = nullptr, stream_hi = nullptr;
    hipEvent_t ev_split = nullptr;
    hipEvent_t step_done = nullptr;  // recorded at the end of tcmi_step_begin
    std::string err;
    // profiling
    bool prof = false;
    struct Pending { int k; hipEvent_t a, b; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> ev_pool;
    double prof_ms[TCMI_K_NKERNELS] = {};
    int64_t prof_n[TCMI_K_NKERNELS] = {};
    // workspace of tcmi_step / host-buffer conveniences
    int64_t ws_L = 0, ws_ld = 0;
    int32_t *d_counts = nullptr;
    uint8_t *d_plain = nullptr, *d_alt = nullptr, *d_flags = nullptr;
    uint8_t *h_rec = nullptr;       // pinned: plain | alt | flags, each ws_ld bytes
    int32_t *h_counts = nullptr;    // pinned [7][ws_ld]
    int64_t step_L = 0;             // > 0 between tcmi_step_begin and tcmi_step_end
    bool step_counts = false;
    bool counts_clean = false;      // the workspace matrix was left zeroed by the last call kernel
    // ride-along call (pipeline): the call of this context's step has not been launched yet; the next step on the
    // stream (another workspace) carries it in its tally launch (tcmi_step_begin_deferred / tcmi_step_flush)
    int defer_call = 1;             // pipeline: the call of step k rides in the tally launch of step k + 1
    bool call_pending = false;
    int64_t pend_L = 0;
    int32_t pend_mincov = 0;
    int pend_amb = 0;
    struct tcmi_ride *ride = nullptr;            // set around a tally launch that may carry another context's call
    int prof_every = 1;             // tcmi_step_begin: every n-th step is launched directly and bracketed with events
    int64_t step_tick = 0;
    bool prof_open = false, prof_mute = false;
    int tally_variant = 0;          // 0 = aligned reads through the fast kernel; 1 = every read through the CIGAR-walk kernel
    int rounds_per_wg = 0;          // 0 = auto
    int host_threads = 8;           // threads tcmi_readset_upload packs with
    int stage_cap = 0;              // upper bound on the reads per stage (0 = fill the LDS buffer)
    int chunk_stages = 0;           // stages per chunk, 0 = default (up to 8)
    int project_reads = 1;          // reads with indels / skips go to the fast kernel projected onto the reference
};

// A read set that is about to be built takes its context's rules: the one place they are copied.  from_stream false: flat arrays
// (tcmi_pack_src::mode 0) carry no MAPQ, no QUAL and no names — no rule applies, and their entry points have refused the three
// that would have to.
static inline void tcmi_rules_stamp(tcmi_readset *rs, const tcmi_ctx *ctx, bool from_stream) { rs->rules = from_stream ? ctx->rules : tcmi_read_rules(); }

int tcmi_fail(tcmi_ctx *ctx, int code, const char *fmt, ...);
void *tcmi_ctx_pinned(tcmi_ctx *ctx, size_t bytes);             // >= bytes of the context's pinned scratch (grow-only; nullptr: no memory)
#define TCMI_HIP(ctx, call)                                                                   \
    do {                                                                                      \
        hipError_t e__ = (call);                                                              \
        if (e__ != hipSuccess)                                                                \
            return tcmi_fail((ctx), TCMI_E_HIP, "%s failed: %s (%s:%d)", #call,               \
                             hipGetErrorString(e__), __FILE__, __LINE__);                     \
    } while (0)

// a temporary device allocation of a host-buffer convenience: freed on every way out
struct tcmi_dev_tmp {
    void *p = nullptr;
    tcmi_dev_tmp() = default;
    tcmi_dev_tmp(const tcmi_dev_tmp &) = delete;
    tcmi_dev_tmp &operator=(const tcmi_dev_tmp &) = delete;
    ~tcmi_dev_tmp() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
};
// what api.cpp, tables.cpp, step.cpp and split_step.cpp call of each other stays out of the library's symbol table
#define TCMI_LOCAL __attribute__((visibility("hidden")))
// the workspace of tcmi_step and the host-buffer conveniences (api.cpp): _ensure makes it hold L positions (grow-only); _load_counts
// makes it large enough and loads a host [L][7] matrix into it
TCMI_LOCAL int tcmi_ws_ensure(tcmi_ctx *ctx, int64_t L);
TCMI_LOCAL int tcmi_ws_load_counts(tcmi_ctx *ctx, const int32_t *counts, int64_t L);
// the tables in a step (tables.cpp): _enqueue launches whatever is on over the workspace matrix; _step_begin marks what the step that
// begins computes (nothing: a ride-along step); _step_end publishes what the step that ends (step_L still set) computed; _release
// frees all the tables own; the rest: what the refusals of the pipeline and the runner ask
TCMI_LOCAL int tcmi_tables_enqueue(tcmi_ctx *ctx, int64_t L);
TCMI_LOCAL void tcmi_tables_step_begin(tcmi_ctx *ctx, bool ride_along);
TCMI_LOCAL void tcmi_tables_step_end(tcmi_ctx *ctx);
TCMI_LOCAL void tcmi_tables_release(tcmi_ctx *ctx);
TCMI_LOCAL bool tcmi_var_table_on(const tcmi_ctx *ctx);
TCMI_LOCAL bool tcmi_iv_table_on(const tcmi_ctx *ctx);
TCMI_LOCAL int64_t tcmi_iv_table_n(const tcmi_ctx *ctx);

// profiling brackets (no-ops unless enabled)
void tcmi_prof_begin(tcmi_ctx *ctx, int k);
void tcmi_prof_end(tcmi_ctx *ctx, int k);

// what the device packer reads (device pointers)
struct tcmi_pack_src {
    // mode 0: flat arrays (struct tcmi_reads on the device)
    const int32_t *pos; const uint16_t *flag; const int32_t *l_qseq; const int32_t *tid;
    const uint64_t *cigar_off; const uint32_t *cigar; const uint64_t *seq_off; const uint8_t *seq;
    // mode 1: the inflated BAM stream and the offset of every record's block_size field (bam_device.hip)
    const uint8_t *stream; const uint64_t *rec_off;
    int64_t n;
    int32_t mode, pos_shift;
    // a contig layout (tcmi_ctx_set_layout; n_lay = 0: none, reference 0 at pos_shift): lay[t] = shift of reference t (< 0: dropped),
    // lay[n_lay + t] = the end of its slot; lay_ext[t]: the kept reads' max end on reference t, in its own coordinates (atomicMax)
    const int32_t *lay; int32_t *lay_ext; int32_t n_lay;
    // the read filter (mode 1; zero for flat arrays, which carry no MAPQ)
    tcmi_filter_words flt;
    // the base-quality floor (mode 1; in what was the struct's tail padding: no kernel's argument offsets move)
    uint32_t min_bq;
};
static_assert(sizeof(tcmi_pack_src) == 128, "min_bq sits in the tail padding");
// one read on one insert-candidate column, as the device kernel hands it to the host (ins_entries.hip -> insert_tokens.cpp)
struct tcmi_dev_entry {
    uint64_t key;               // packed token (insert_tokens.cpp)
    uint64_t name_hash;         // FNV-1a of the read name
    uint32_t j;                 // the read's place in file order (compacted index)
    int32_t pos, end, mpos, isize, l_qseq;
    uint16_t flag;
    uint8_t qual;
    uint8_t bits;               // base code | on_base << 4 | mate on another reference << 5 | insertion too long for the key << 6 (its bases lie in
                                // the call's text buffer: key bits 8-39 where, bits 40-62 how many) | << 7: that buffer was full
    int32_t qref;               // deletion / ref-skip token: reference position of the matched base whose quality is tested, or -1
};
// "does read `idx` have a matched base on reference position `ref`, which, with what quality?" — asked for the other mate of an
// overlapping pair (insert_tokens.cpp); answered from the host arrays or by a kernel over the resident stream
struct tcmi_probe_req { int64_t idx; int32_t ref; };
struct tcmi_probe_res { uint8_t matched, base, qual; };
typedef std::function<int(const std::vector<tcmi_probe_req> &, std::vector<tcmi_probe_res> &)> tcmi_prober;
int tcmi_modal_from_dev_entries(int32_t n_pos, const tcmi_dev_entry *ents, const int64_t *ent_off, const int32_t *ent_cnt,
                                int32_t min_base_quality, int64_t max_depth, int ignore_overlaps, const tcmi_prober *prober, char *tokens,
                                int64_t tokens_cap, int64_t *token_off, int64_t *n_tokens, int32_t *status_flags, const uint8_t *long_text = nullptr,
                                size_t long_bytes = 0);
extern "C" int tcmi_bamfile_read_threads(const char *path, int read_threads, tcmi_bamfile **out);   // (bamfile.cpp; 0 = by size)
// device packer (pack_device.hip): struct tcmi_reads -> device -> packed read set; TCMI_E_UNSUPPORTED + *why when the
// input needs the host packer
int tcmi_upload_and_pack_on_device(tcmi_ctx *ctx, const tcmi_reads *r, tcmi_readset *rs, uint32_t *why);
int tcmi_pack_on_device(tcmi_ctx *ctx, const void *pack_src, tcmi_readset *rs, uint32_t *why);
// The one-sync file path (bam_device.hip: tcmi_bamfile_step, tcmi_readset_from_bamfile): everything behind bgzf_copy —
// record index, the chain of records across the blocks, classification, prefix sums, bit planes (pk_index, pk_place), chunk planning
// (pk_pack) — queued on the context's stream from CAPACITIES instead of counts read back; _finish, once the stream has been
// waited for, checks what was deferred (block verdicts, chain, capacities, packer flags) and fills the read set in, or says that
// the file must take the several-kernel path (TCMI_E_UNSUPPORTED: nothing of the job may be used then).
struct tcmi_fused_job {
    // in: device pointers into the context's arena (bgzf_copy)
    const uint8_t *d_stream = nullptr;
    uint64_t stream_len = 0;
    const void *d_desc = nullptr;       // BlockDesc [n_blocks]
    const uint32_t *d_slot = nullptr, *d_nrec = nullptr, *d_first = nullptr, *d_stat = nullptr;
    const int32_t *d_over = nullptr;
    int64_t n_blocks = 0, n_own = 0;
    int ranged = 0;
    uint32_t rec_hint = 0;              // mean size of the file's first records (< 36: none)   } what the capacities are worked out
    bool safe_caps = false;             // sized as the arena was reserved, not from the hint     } from: pack_caps.h pk_one_sync_caps
    int64_t len_bound = 0;              // positions the reads may reach (chunk capacity)         }
    // out (enqueue)
    PkCaps caps = {};                   // what the arrays are sized for
    char *h_pin = nullptr;              // pinned: PackTotals | per-block partials (filled by the copies queued behind the kernels)
    void *d_tot = nullptr;
    uint64_t *d_rec = nullptr;
    uint32_t *c_idx = nullptr, *gen_idx = nullptr;
    int32_t *c_pos = nullptr;
    const void *d_blk_alg = nullptr, *d_blk_end = nullptr;
    const void *d_mate_cnt = nullptr;   // the mate join's four counters (null: the setting is off); the report brings them along
    const void *d_dup_cnt = nullptr;    // dedup.hip's four counters, likewise
};
int tcmi_pack_fused_enqueue(tcmi_ctx *ctx, tcmi_fused_job *job, tcmi_readset *rs);
int tcmi_pack_fused_report(tcmi_ctx *ctx, tcmi_fused_job *job);     // queue it LAST (behind the tally and the call, if any): then wait, then _finish
int tcmi_pack_fused_finish(tcmi_ctx *ctx, tcmi_fused_job *job, tcmi_readset *rs, uint32_t *why);
// The mate join (mate_join.hip) between the packers' classification and their plane kernels, on ctx->stream: the table zeroed, the two
// launches, nothing waited for.  n >= 0: the record count; n < 0 (the one-sync packer): the kernels take it from what pk_index left —
// rec_base[n_blocks - 1] + the last block's own records — and count nothing while *flags has a bit of `ovf` (the index is incomplete then).
struct tcmi_mate_job {
    tcmi_pack_src src;                  // the stream, the record index, the filter, the layout (which records are kept: kept_span)
    uint64_t stream_len;
    int64_t n;
    uint32_t rec_cap;                   // the grid and the table are sized from it
    const uint32_t *rec_base, *n_rec;
    int32_t n_blocks, n_own;
    const uint32_t *flags;
    uint32_t ovf;
    unsigned long long *table;          // [slots + 4] {tag << 32 | record + 1}, slots = tcmi_mate_slots(rec_cap); behind them the four
                                        // counters (tcmi_mate_counters): one memset zeroes both
    uint32_t *clip;                     // out [rec_cap]
    // with the duplicate rule (null / 1 without): every record of a pair receives its mate's record index + 1, every other record below
    // the record count 0; apply == 0 (the duplicate rule without the mate rule): the join runs for mate_idx alone — clip[] is written
    // as zeros and the counters stay 0
    uint32_t *mate_idx;                 // out [rec_cap]
    int32_t apply;
};
// (the table's and clip[]'s arena bytes: pack_caps.h)
static inline const unsigned long long *tcmi_mate_counters(const tcmi_mate_job &job) { return job.table + tcmi_mate_slots(job.rec_cap); }
// The duplicate rule (dedup.hip) behind the join, inside its profiling bracket: ends[] per record, the templates' table, the verdicts.
// table: {tag << 32 | claimant leader + 1} [slots] | best [slots] (64 bits) | the four counters | the templates per slot [slots]
// (32 bits), slots = tcmi_mate_slots(rec_cap): one memset zeroes all of it (pack_caps.h: tcmi_dup_table_bytes).
struct tcmi_dup_end;
struct tcmi_dedup_job {
    tcmi_dup_end *ends;                 // [rec_cap]
    uint32_t *slot_of;                  // [rec_cap] a leader's slot
    uint8_t *dup;                       // out [rec_cap] 0 / 1
    unsigned long long *table;
};
static inline const unsigned long long *tcmi_dup_counters(const tcmi_mate_job &job, const tcmi_dedup_job &d) { return d.table + 2 * tcmi_mate_slots(job.rec_cap); }
// (dedup: null without the duplicate rule)
int tcmi_mate_join_enqueue(tcmi_ctx *ctx, const tcmi_mate_job &job, const tcmi_dedup_job *dedup = nullptr);
void tcmi_dedup_launch(tcmi_ctx *ctx, const tcmi_mate_job &job, const tcmi_dedup_job &dedup, unsigned grid, uint32_t slot_mask);

// the context's device arena (api.cpp): _reserve hands it out anew, `bytes` large (whatever lived in it is gone: arena_epoch tells);
// _take carves the next piece, 256-byte aligned — the packers sum a list's pieces against `cap` before they take them (pack_caps.h: PkScratch)
int tcmi_arena_reserve(tcmi_ctx *ctx, size_t bytes);
void *tcmi_arena_take(tcmi_ctx *ctx, size_t bytes);
// kernels (tally.hip / call.hip)
int tcmi_launch_tally(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t L, int64_t ld, int32_t *d_counts);
int tcmi_launch_tally_fast(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t L, int64_t ld, int32_t *d_counts);
// pipeline-internal: a step whose call kernel rides in the NEXT step's tally launch (step.cpp)
int tcmi_step_begin_deferred(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t L, int32_t mincov, int include_ambig, tcmi_ctx *prev);
int tcmi_step_flush(tcmi_ctx *ctx);
int tcmi_launch_call(tcmi_ctx *ctx, int32_t *d_counts, int64_t L, int64_t ld, int32_t mincov,
                     int include_ambig, int clean, uint8_t *d_plain, uint8_t *d_alt, uint8_t *d_flags,
                     int32_t *d_events, int32_t *d_event_counts);

// the variant table's three launches (variants.hip) on the context's stream, over min(L, n_ref) > 0 positions; blk_cnt / blk_base:
// ceil(min(L, n_ref) / 256) words each; total: a word the host can read once the stream has been waited for
struct tcmi_var_job {
    const int32_t *counts; int64_t L, ld;
    const uint8_t *ref; int64_t n_ref;
    tcmi_var_rule rule;
    uint32_t *blk_cnt; unsigned long long *blk_base, *total;
    tcmi_variant *records; int64_t cap;
};
int tcmi_launch_variants(tcmi_ctx *ctx, const tcmi_var_job &job);

// the amplicon table's launch (intervals.hip) on the context's stream: one workgroup per interval, 0 < n <= 65 536 checked intervals
struct tcmi_iv_job {
    const int32_t *counts; int64_t L, ld;
    int64_t n; const int64_t *start, *end;
    int32_t min_depth;
    tcmi_interval_stat *records;
};
int tcmi_launch_intervals(tcmi_ctx *ctx, const tcmi_iv_job &job);

static inline int64_t tcmi_round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
