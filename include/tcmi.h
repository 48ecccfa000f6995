/*
 * tcmi.h — C ABI of the MI355X-native consensus hot path (libtcmi.so).
 *
 * The reference (RIVM-bioinformatics/TrueConsense, pure Python) has no FFI; the
 * seam this library replaces is three Python call sites:
 *
 *   BuildIndex(bamfile, ref)                       TrueConsense/indexing.py:75-154
 *   ListInserts(iDict, mincov, bam)                TrueConsense/Events.py:5-44
 *   BuildConsensus(mincov, iDict, GFFdict, ...)    TrueConsense/Sequences.py:168-322
 *
 * Everything here is plain C: pointers, sizes, int status codes.  No torch or
 * HIP types appear in a signature (streams / device buffers are `void*`).
 * All entry points return 0 on success or a negative TCMI_E_* code; the text of
 * the last failure is available from tcmi_last_error().  Nothing throws or
 * aborts across this boundary.
 *
 * Threading: one context per device/stream; contexts are independent; a single
 * context is not thread-safe.  Host-only entry points (tcmi_consensus_walk, tcmi_modal_tokens,
 * tcmi_bam_*) are re-entrant and need no GPU; tcmi_bamfile_read needs the HIP runtime (pinned memory).
 */
#ifndef TCMI_H
#define TCMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TCMI_ABI_VERSION 5

/* ---- status codes ------------------------------------------------------- */
#define TCMI_OK            0
#define TCMI_E_NODEVICE   (-1)  /* no usable HIP device / HIP runtime error at init */
#define TCMI_E_HIP        (-2)  /* HIP runtime call failed                         */
#define TCMI_E_ARG        (-3)  /* bad argument (null pointer, negative size, ...) */
#define TCMI_E_NOMEM      (-4)
#define TCMI_E_FORMAT     (-5)  /* malformed BAM / BGZF input                      */
#define TCMI_E_IO         (-6)
#define TCMI_E_KEYERROR   (-7)  /* reference would raise KeyError (walk past the last position,
                                   Sequences.py:47 via :214/:282); *err_pos = missing key */
#define TCMI_E_ZERODIV    (-8)  /* reference would raise ZeroDivisionError (Events.py:102) */
#define TCMI_E_UNSUPPORTED (-9)

/* ---- count-matrix column order (indexing.py:134) ------------------------ */
enum { TCMI_COV = 0, TCMI_A = 1, TCMI_T = 2, TCMI_C = 3, TCMI_G = 4, TCMI_X = 5, TCMI_I = 6,
       TCMI_NCOL = 7 };

/* ---- per-position flags produced by the call kernel --------------------- */
#define TCMI_F_LOWCOV   0x01u  /* cov < mincov                      Sequences.py:191        */
#define TCMI_F_PRIMX    0x02u  /* primary nucleotide is X           Sequences.py:199,277    */
#define TCMI_F_MINDEL   0x04u  /* (X/cov)*100 >= 15, cov != 0       Events.py:85-106        */
#define TCMI_F_INSCAND  0x08u  /* insert candidate                  Events.py:29-36         */
#define TCMI_F_COVGT    0x10u  /* cov > mincov (strict)             Sequences.py:311, ORFs.py:142 */
#define TCMI_F_COVZERO  0x20u  /* cov == 0                          Events.py:102 (division) */
#define TCMI_F_AMBIG    0x40u  /* IsAmbiguous() true                Ambig.py:179-228        */
/* a position is an "event" (needs the sequential host walk) when it carries one of: */
#define TCMI_EVENT_MASK (TCMI_F_PRIMX | TCMI_F_MINDEL | TCMI_F_INSCAND)

/* ---- reads as flat host arrays (what a BAM reader yields) --------------- */
/* BAM field meaning per SAM spec §4.2.  Offsets are element counts.          */
typedef struct tcmi_reads {
    int64_t         n_reads;
    const int32_t  *pos;        /* [n] 0-based leftmost reference position               */
    const uint16_t *flag;       /* [n] BAM FLAG                                          */
    const int32_t  *l_qseq;     /* [n] query length (0 when SEQ is '*')                  */
    const uint64_t *cigar_off;  /* [n+1] offsets into cigar[]                             */
    const uint32_t *cigar;      /* BAM encoding len<<4|op, ops MIDNSHP=X                 */
    const uint64_t *seq_off;    /* [n+1] byte offsets into seq[]                          */
    const uint8_t  *seq;        /* BAM 4-bit packed "=ACMGRSVTWYHKDBN", high nibble first */
    const uint8_t  *qual;       /* optional, Σ l_qseq bytes (offsets = prefix of l_qseq) or NULL */
    const int32_t  *tid;        /* optional [n] reference id; reads with tid<0 never pile up */
    /* optional accelerators for the insert-token sweep (tcmi_modal_tokens); zero / NULL = not given */
    const uint64_t *qual_off;   /* [n+1] offsets into qual[] (= prefix sums of l_qseq)                  */
    int64_t sorted_max_span;    /* > 0 promises: reads ascend by pos (unplaced reads last) and no read
                                   spans more reference positions than this; lets the sweep visit only
                                   the reads around each candidate position (tcmi_bam_reads fills it)   */
    /* optional mate fields and read names (SAM spec §4.2 next_refID, next_pos, tlen, read_name): what pysam's default
     * pileup needs to find overlapping mates (ignore_overlaps, Events.py:66); NULL = not given                         */
    const int32_t  *next_tid;   /* [n] */
    const int32_t  *next_pos;   /* [n] */
    const int32_t  *tlen;       /* [n] */
    const uint64_t *name_off;   /* [n+1] offsets into names[] */
    const char     *names;      /* read names, no terminators */
} tcmi_reads;

typedef struct tcmi_ctx tcmi_ctx;          /* one per device + stream            */
typedef struct tcmi_readset tcmi_readset;  /* reads resident in HBM              */

/* ---- library / context -------------------------------------------------- */
int         tcmi_abi_version(void);
const char *tcmi_last_error(const tcmi_ctx *ctx);  /* ctx may be NULL: last error of this thread */
int         tcmi_device_count(int *out_count);     /* 0 devices is not an error                  */

int  tcmi_ctx_create(int device, tcmi_ctx **out);  /* fails with TCMI_E_NODEVICE without a GPU    */
/* A context on a stream the caller owns (a hipStream_t; NULL = the default stream; e.g. torch's
 * current stream, or the
 * stream of another tcmi_ctx: two contexts on one stream give two workspaces whose launches
 * run back to back, so steps can be queued ahead without overlapping each other).            */
int  tcmi_ctx_create_on_stream(int device, void *stream, tcmi_ctx **out);
int  tcmi_ctx_destroy(tcmi_ctx *ctx);
int  tcmi_ctx_sync(tcmi_ctx *ctx);                 /* wait for the context's stream               */
void *tcmi_ctx_stream(tcmi_ctx *ctx);              /* the hipStream_t all launches go to          */
/* options (tcmi_readset_upload reads the packing ones, the launches the others):
 *   "tally_variant"  0 = reads take the bit-plane kernel (default), 1 = every read takes the CIGAR-walk kernel
 *                    (an independent implementation the tests cross-check with)
 *   "project_reads"  1 = reads with indels / ref-skips are projected onto the reference when they are packed and
 *                    take the bit-plane kernel (default); 0 = they take the CIGAR-walk kernel
 *   "device_pack"    1 = tcmi_readset_upload copies the BAM-native arrays to the device and packs them there
 *                    (pack_device.hip; default; needs reads sorted by position and entries of <= 512 positions,
 *                    anything else takes the host packer); 0 = always pack on the host
 *   "verify_crc"     1 = the device decoder checks every BGZF block's CRC-32 (in bgzf_copy's flush; default, as htslib does);
 *                    0 = ISIZE, stream termination and the record chain only
 *   "one_sync"       1 = a file decoded on the device takes the one-sync path first (pk_index + pk_place + pk_pack: record index,
 *                    record chain, classification, places and planes without a host round trip; capacities instead of counts read back; default), 0 = only the
 *                    several-kernel path with its three waits (the path that words every refusal; the tests cross-check the two)
 *   "mid_wait"       0 = ONE wait of the host per file (default since round 5: with the CRC taken in bgzf_copy's flush — a kernel less
 *                    per file — eight contexts measured 69.3 - 70.0 M positions/s against 68.4 - 69.4 with the second wait, three turns
 *                    each on one box), 1 = the one-sync path waits a second time, behind the decode kernels (round 4's default)
 *   "prefix_kernels" the one-sync path's kernels need, per BGZF block, the records / kept reads / plane words in front of it: 0 = every
 *                    workgroup adds them up for itself below 16 384 blocks and three one-workgroup scan launches do it from there on
 *                    (the sums are quadratic in the blocks; default), 1 = always the scan launches, -1 = never
 *   "decode_token_mb" the device decoder's token scratch, MiB (default 4096): a file whose BGZF blocks need more (tokens take 3 - 10
 *                    times the inflated bytes while a block is decoded) is decoded in batches of blocks that share the scratch —
 *                    the inflated stream stays whole
 *   "sym_scratch_div" (tests) bgzf_symbols' speculating lanes park 1 / n of their share of the token scratch: lanes overflow and their blocks
 *                    are decoded once more in order (pass B), which must cut the stream into the same tokens; default 1
 *   "h2d_pieces"     n >= 2: compressed bytes that come from host memory cross PCIe in n pieces of whole blocks on a copy stream of the
 *                    context's, each piece's blocks inflated as soon as it has arrived; 0 (default): one copy in front of the decoder —
 *                    on these boxes (46 GB/s) pieces lose: 4.5 ms against 3.97 ms for a 6.25 M-read range, DESIGN 7
 *   "split_sub"      tcmi_split_step: a rank's block range is decoded, packed and tallied as this many SUB-RANGES side by side — the first on
 *                    this context, the others on helper contexts it owns (a stream, an arena and a host thread each), so that the inflate of
 *                    one sub-range runs under the pack of another; the sub-ranges must join like ranks' ranges, else the range is taken in
 *                    one piece.  0 = auto (default: for a true range of a larger file 3 from 6 144 blocks on, 2 from 4 096, else 1 — the whole file as
 *                    one range is taken in one piece: measured), 1 = never, up to 8
 *   "chunk_stages"   stages per chunk of the bit-plane kernel: 0 = default (up to 8, capped by "balance_chunks"), or 1..8
 *   "balance_chunks" chunk_stages = 0: size the chunks so that a launch has a multiple of
 *                    (compute units x "wg_per_cu", default 4) of them (default 1)
 *   "stage_cap"      upper bound on the reads per stage (0 = fill the LDS stage buffer; for experiments)
 *   "host_threads"   threads the host packer uses (default min(16, cores))
 *   "rounds_per_wg"  CIGAR-walk kernel: rounds of 256 reads per workgroup (0 = auto)
 *   "defer_call"     (read from the pipeline's first workspace) 1 = tcmi_pipeline_run attaches the call of step k to
 *                    the tally launch of step k + 1 — one launch per step (default); 0 = tally launch + call launch
 *   "profile_every"  with profiling enabled, every n-th tcmi_step_begin has its kernels bracketed by events,
 *                    the others go out unmeasured (default 1) */
int  tcmi_ctx_set_option(tcmi_ctx *ctx, const char *key, int value);
/* ---- several contigs on one coordinate axis (a BAM aligned to a multi-record reference) ----------------------------------
 * tcmi_ctx_set_layout: from now on every upload of the context (tcmi_readset_upload, tcmi_readset_from_bamfile[_blocks],
 * tcmi_bamfile_step) piles reference t's reads up at pos + shift[t] instead of refusing them: reference t owns the positions
 * [shift[t], shift[t] + slot_len[t]) of the count matrix, and the tally, the call and the step see one axis.  shift[t] < 0: the
 * reads of reference t are dropped, like unmapped reads.  The slots of the kept references must ascend in reference order and not
 * overlap (a file sorted by (tid, pos) then stays sorted on the axis) and end below 2^29.  A kept read that ends past its slot is
 * refused (TCMI_E_UNSUPPORTED), never tallied into the next slot.  n_ref = 0: no layout (reference 0 only, the default).
 * Under a layout, tcmi_bamfile_step takes its two-call path, tcmi_readset_modal_tokens / tcmi_readset_ins_entries return
 * TCMI_E_UNSUPPORTED (use tcmi_modal_tokens_layout), and tcmi_readset_upload_batch / tcmi_split_step return TCMI_E_UNSUPPORTED.
 * The context keeps one device table, rewritten by every call with n_ref > 0: a read set with reads longer than 512 positions
 * must be stepped before another layout is set (else TCMI_E_UNSUPPORTED), as before the context's next upload.          */
int  tcmi_ctx_set_layout(tcmi_ctx *ctx, int32_t n_ref, const int64_t *shift, const int64_t *slot_len);
/* per reference, the kept reads' max end (exclusive, in the reference's own coordinates; 0: no read) of a read set uploaded
 * under a layout of n_ref references (tcmi_reads_extent of that reference's reads alone) */
int  tcmi_readset_ref_extents(const tcmi_readset *rs, int32_t n_ref, int64_t *max_end);
/* mapped reads of a read set uploaded under a layout whose reference has no slot (shift < 0): dropped, not tallied */
int  tcmi_readset_dropped(const tcmi_readset *rs, int64_t *n_dropped);
/* ---- read filter (additive: the reference tallies every mapped record, indexing.py:100 stepper="nofilter") ---------------
 * A record PASSES iff mapq >= min_mapq, (flag & require_flags) == require_flags and (flag & exclude_flags) == 0 — samtools view
 * -q / -f / -F; MAPQ is a plain number (255 is not special).  A record that fails is ignored wherever an unmapped record (FLAG
 * 0x4) is ignored: it is not kept, raises no refusal of its own (second reference, far position, slot overrun, long read from
 * flat arrays, CG:B tag), is not counted as dropped under a layout, takes no part in the order asked of kept reads and gives no
 * insert-candidate entry — every result equals the unfiltered result for the file without the failing records.  It is still a
 * link of the record chain, and a structurally broken record still condemns the file.  min_mapq outside 0..255 or a flag word
 * above 0xFFFF: TCMI_E_ARG.  The default 0, 0, 0 passes everything.
 *   tcmi_ctx_set_read_filter  from now on governs every read set the context builds from a record stream decoded on the device
 *                     (tcmi_readset_from_bamfile[_blocks], tcmi_bamfile_step, tcmi_split_step and its sub-range helper contexts,
 *                     the file runner's contexts: tcmi_filerunner_ctx — the runner's host-reader fallbacks apply the filter of
 *                     its contexts too).  The read set remembers the filter it was built under: tcmi_readset_modal_tokens and
 *                     tcmi_readset_ins_entries apply it beside their flag_filter whatever the context is set to later.  Flat
 *                     arrays (tcmi_readset_upload[_batch], tcmi_tally, tcmi_modal_tokens[_layout]) carry no MAPQ and are taken
 *                     as given: whoever built them filters them (tcmi_bam_filter).
 *   tcmi_readset_filtered     records of the file / block range that failed the filter the read set was built under */
int  tcmi_ctx_set_read_filter(tcmi_ctx *ctx, int32_t min_mapq, uint32_t require_flags, uint32_t exclude_flags);
int  tcmi_readset_filtered(const tcmi_readset *rs, int64_t *n_filtered);
/* ---- base-quality floor (additive: the reference piles up with min_base_quality = 0, indexing.py:100) --------------------
 * A pileup TOKEN — one read on one reference column — is SKIPPED iff its quality is below q (samtools mpileup -Q, pysam's
 * pileup_base_qual_skip): a matched base is tested with its own QUAL byte, a deletion or ref-skip token with the QUAL byte of the
 * next query base (the query index at which the D / N operation starts); a query index at or beyond l_seq has quality 0 (SEQ "*",
 * a SEQ shorter than the CIGAR, a D / N with no base behind it); a record without QUAL (bytes 0xFF) has quality 255 and is never
 * skipped.  A skipped token is absent from its column: nothing for coverage, A/T/C/G, X, or I (the insertion mark belongs to the
 * token in front of the insertion).  Nothing else about the read changes: the piled-up count, the extent and the per-reference
 * extents are those of the unfiltered reads, and a column whose tokens are all skipped is a zero row.  The qualities are tested as
 * the file stores them: pysam's overlap rewrite of mate pairs (ignore_overlaps) is NOT modelled (tcmi_ctx_set_mate_overlap removes
 * the overlap by position instead).  q outside 0..255: TCMI_E_ARG;
 * q = 0 (the default) is no floor and takes the same kernels as before.
 *   tcmi_ctx_set_min_base_quality  from now on governs every read set the context builds from a record stream decoded on the
 *                     device (tcmi_readset_from_bamfile[_blocks], tcmi_bamfile_step, tcmi_split_step and its sub-range helper
 *                     contexts, the file runner's contexts: tcmi_filerunner_ctx), and with it the count matrix and everything
 *                     derived from it.  It does not touch the insert-candidate sweeps (tcmi_readset_modal_tokens and the like keep
 *                     their own min_base_quality argument).  While q > 0 whatever would tally WITHOUT the floor refuses with
 *                     TCMI_E_UNSUPPORTED instead: the flat-array entry points (tcmi_readset_upload[_batch], tcmi_tally,
 *                     tcmi_pipeline_run[_batched]: flat arrays carry no QUAL) and the file runner's host-reader fallback (the host
 *                     packer knows no floor; the message says why the file left the device path).
 *   tcmi_readset_min_base_quality  the floor the read set was built under, whatever the context is set to later */
int  tcmi_ctx_set_min_base_quality(tcmi_ctx *ctx, int32_t q);
int  tcmi_readset_min_base_quality(const tcmi_readset *rs, int32_t *q);
/* ---- amplicon primer mask (additive: what `ivar trim` / `samtools ampliconclip` do to the BAM in front of other callers) ------
 * A primer is (start, end, reverse): 0-based, end-exclusive, on the count matrix's axis (under a contig layout: shifted by its
 * contig's slot); reverse 0 is a '+' (left) primer, 1 a '-' (right) primer.  A kept read has a first column p = POS (+ its contig's
 * shift) and a last column q = p + the CIGAR's reference length - 1 (soft and hard clips do not count).  With slack s:
 *   head mask   head_end = the largest `end` over the '+' primers with start - s <= p < end (none: p); tokens on columns
 *               c < head_end are masked
 *   tail mask   tail_start = the smallest `start` over the '-' primers with start <= q < end + s (none: q + 1); tokens on columns
 *               c >= tail_start are masked
 * Both apply to every kept read whatever its own strand (a read-through mate carries the opposite primer at its 3' end); a '+'
 * primer never masks a tail and a '-' primer never a head.  A masked token is SKIPPED exactly as one below the base-quality floor
 * is — absent from its column: nothing for coverage, A/T/C/G, X or I —, per column and whatever the token is: a deletion that
 * crosses the mask's edge loses only its masked columns, and the insertion mark goes iff the token in front of the insertion is
 * masked.  Nothing else about the read changes: the piled-up count, the extent and the per-reference extents are the unmasked
 * reads', and a read masked from end to end is piled up and adds nothing.  Together with a floor a token is skipped if either rule
 * skips it; without a floor (q = 0) a query index at or beyond l_seq is NOT skipped outside the mask.
 *   tcmi_ctx_set_primers   compiles the table (n = 0 clears it; TCMI_E_ARG: n above 65 536, start < 0, end <= start, a coordinate
 *                     at or above 2^29, reverse not 0 / 1, slack outside 0..1000) and from now on governs every read set the
 *                     context builds from a record stream decoded on the device — the entry points the floor governs, sub-range
 *                     helper contexts included —, and with it the count matrix and everything derived from it.  It does NOT
 *                     touch the insert-candidate sweeps' own region pileup (tcmi_readset_modal_tokens and kin: a masked read still
 *                     votes on an insert candidate inside a primer site).  A read set REMEMBERS the table it was built under (it
 *                     shares the device copy: its long reads are masked at tally time); changing or clearing the context's table
 *                     later does not change it.  While a table is set whatever would tally WITHOUT it refuses with
 *                     TCMI_E_UNSUPPORTED and a message naming --primers: the flat-array entry points, the array pipeline, the
 *                     file runner's host-reader fallback (the host packer knows no mask).  No table: the kernels of before.
 *   tcmi_readset_primers   the size of the table the read set was built under and its kept reads with a non-empty head or tail mask
 *   tcmi_primers_compile   (GPU-free) the two segment lists the kernels search, as {a, b, v} triples sorted by a: a read whose p
 *                     (q) lies in [a, b) of a head (tail) segment has head_end (tail_start) v; seg_cap: room per list, in
 *                     segments (2 n - 1 suffice); msg (may be NULL) receives the words of a TCMI_E_ARG */
int  tcmi_ctx_set_primers(tcmi_ctx *ctx, int32_t n, const int64_t *start, const int64_t *end, const int32_t *reverse, int32_t slack);
int  tcmi_readset_primers(const tcmi_readset *rs, int32_t *n_primers, int64_t *n_masked_reads);
int  tcmi_primers_compile(int32_t n, const int64_t *start, const int64_t *end, const int32_t *reverse, int32_t slack, int32_t seg_cap,
                          int32_t *head, int32_t *n_head, int32_t *tail, int32_t *n_tail, char *msg, int64_t msg_cap);
/* ---- mate overlap (additive: what samtools mpileup does by default to the two mates of a pair, and so ivar) -----------------------
 * A read pair whose mates cover shared columns is one molecule: under this setting it counts ONCE there.  The rule is exact, integer
 * only, and does not depend on the order of the file (csrc/mate_rule.h holds its text).  It concerns the KEPT records of a device-
 * decoded stream (mapped, through the read filter, consistent, on a reference that piles up, reference span > 0):
 *   eligible   FLAG has 0x1 and 0x2, none of 0x8 / 0x100 / 0x800, exactly one of 0x40 / 0x80; next_refID == refID; next_pos >= 0
 *   key        (read name without its NUL, refID, min(pos, next_pos), max(pos, next_pos)); the eligible records of one key are a group
 *   pair       a group of exactly two records a, b with a.next_pos == b.pos, b.next_pos == a.pos, one 0x40 and the other 0x80.  Every
 *              other group is unjoined (one record, three or more — those records count as `ambiguous` —, two firsts, ...).  Strand
 *              plays no part.
 *   loser      of a pair, the record with the larger pos; at equal pos the one with 0x80.  The other is the winner.
 *   clip       with [p, q] a record's first and last column: clip(loser) = max(0, min(q_winner, q_loser) - p_loser + 1), 0 for every
 *              other record.  p_loser >= p_winner: the shared columns are a prefix of the loser.
 *   effect     the loser's tokens on its first `clip` columns are skipped exactly as primer-masked tokens are: its head_end becomes
 *              max(the primer table's head_end, p + clip).  Everything said of a masked column above holds (no coverage, letter, X or
 *              I; a D / N op across the edge loses only its clipped columns; the I mark goes iff the token in front of the insertion
 *              is skipped; a record clipped from end to end is piled up and adds nothing; the piled-up count, the extent and the
 *              per-reference extents are unchanged).  The floor and the primer table combine with it by OR.
 * Deviations from htslib's tweak_overlap_quality, on purpose: qualities are NOT summed; the winner is chosen by position, not by
 * quality; a column where the winner's own token is below the floor or primer-masked gets nothing from the template; the insert-
 * candidate sweeps' region pileup (tcmi_readset_modal_tokens and kin) keeps its own overlap handling (ignore_overlaps) and is not
 * touched.
 *   tcmi_ctx_set_mate_overlap   on = 0 / 1 (anything else: TCMI_E_ARG); from now on governs the read sets the floor governs.  A read
 *                     set REMEMBERS the setting and, while its decoded stream is resident, the clips: the stream-walking calls
 *                     (strand counts, link counts, indel events, evidence counts, the long reads' tally) count under the rule.
 *                     While on, whatever would tally WITHOUT the rule, or where a mate may lie outside what is decoded, refuses with
 *                     TCMI_E_UNSUPPORTED and a message naming --mate-overlap: tcmi_split_step and its sub-range helpers, a block
 *                     RANGE of a file (tcmi_readset_from_bamfile_blocks on less than the whole file), the flat-array entry points,
 *                     the array pipeline, the file runner's host-reader fallback.  An unsorted file is fine.  Off: the launches of
 *                     before.
 *   tcmi_readset_mate_overlap   the setting the read set was built under and the join's counters: pairs, records with clip > 0, the
 *                     sum of the clips, records of ambiguous groups (any pointer may be NULL) */
int  tcmi_ctx_set_mate_overlap(tcmi_ctx *ctx, int32_t on);
int  tcmi_readset_mate_overlap(const tcmi_readset *rs, int32_t *on, int64_t *pairs, int64_t *clipped_reads, int64_t *clipped_columns,
                               int64_t *ambiguous);
/* ---- duplicate templates (additive: what samtools markdup / Picard MarkDuplicates do in a pass of their own) -----------------------
 * Under this setting the records of a duplicate template add nothing to the count matrix.  The rule is exact and integer only; which
 * templates exist does not depend on the order of the file, only the stated tie-break does (csrc/dedup_rule.h holds its text).  It
 * concerns the KEPT records of a device-decoded stream (mapped, through the read filter, consistent, on a reference that piles up,
 * reference span > 0):
 *   examined   kept records without FLAG 0x100 / 0x800: secondary and supplementary records are never duplicates and never stand
 *              for a template (samtools' default)
 *   end        of a record: (refID, u5, rev).  rev is FLAG 0x10; u5 the unclipped 5' coordinate on the record's own reference, not
 *              the shifted axis: forward pos - (sum of leading S and H lengths), reverse pos + span - 1 + (sum of trailing S and H
 *              lengths).  u5 is signed and may be negative (kept in 32 bits, saturating).
 *   score      of a record: the sum of its QUAL bytes >= 15 (Picard's SUM_OF_BASE_QUALITIES); a byte of 0xFF is a missing quality
 *              and adds nothing, so a QUAL of all 0xFF scores 0, as l_seq == 0 does; saturates at 2^32 - 1
 *   templates  a pair is exactly a pair of the mate join above (group of two, eligible, the pair test) — whether or not the mate
 *              rule is on; every other examined record is a fragment (unpaired, mate unmapped or filtered away, not proper, a
 *              member of an ambiguous group, ...).  A pair's leader is its record with the lower record index; a fragment leads
 *              itself.  A pair's score is the sum of both records' scores, saturating likewise.
 *   key        fragment (F, refID, u5, rev); pair (P, refID, end_a, end_b) with the two ends ordered by (u5, rev) — which end is
 *              read 1 plays no part.  Fragments and pairs never share a key.
 *   winner     of the templates of one key the highest score wins, at equal score the template whose leader has the lowest record
 *              index.  Every other template of the key is a duplicate, and all its records — both mates of a pair — are.
 *   effect     clip[i] = max(clip[i], span(i)) for a duplicate record: it is clipped from end to end, and everything said of that
 *              under the mate rule holds (piled up, adds nothing; the piled-up count, the extent and the per-reference extents are
 *              unchanged).  It combines with the floor, the primer table, the read filter and the mate rule by OR; with the mate
 *              rule also on a surviving pair still gets its overlap clip.
 * Deviations from samtools markdup and Picard MarkDuplicates, on purpose: pairs are only the join's pairs, which requires 0x2; a
 * fragment does not lose to a pair that has an end at its place (both tools let it); there is no optical-distance rule; the mate's end
 * is taken from the mate's own record, not from an MC tag; nothing is written back, there is no marked BAM; the insert-candidate
 * sweeps' region pileup (tcmi_readset_modal_tokens and kin) keeps its own pileup and is not touched, exactly as under the mate rule.
 *   tcmi_ctx_set_dedup   on = 0 / 1 (anything else: TCMI_E_ARG); from now on governs the read sets the floor governs.  A read set
 *                     REMEMBERS the setting and, while its decoded stream is resident, the verdicts: the stream-walking calls count
 *                     under the rule.  While on, whatever would tally WITHOUT the rule, or where a template's other records may lie
 *                     outside what is decoded, refuses with TCMI_E_UNSUPPORTED and a message naming --dedup: the entry points that
 *                     refuse under the mate rule.  tcmi_readset_amplicon_reads asks only which records are kept and counts
 *                     duplicates as before.  Off: the launches of before.
 *   tcmi_readset_dedup   the setting the read set was built under and the counters: examined templates, duplicate templates,
 *                     duplicate records, keys with at least two templates (any pointer may be NULL)
 *   tcmi_readset_duplicates   one byte per record of the stream, 1: a duplicate, into out[cap] (cap >= the records, else
 *                     TCMI_E_ARG), *n the records; on the context that holds the stream, while it is resident: TCMI_E_UNSUPPORTED
 *                     once another upload happened there, or when the read set was built without the rule */
int  tcmi_ctx_set_dedup(tcmi_ctx *ctx, int32_t on);
int  tcmi_readset_dedup(const tcmi_readset *rs, int32_t *on, int64_t *templates, int64_t *dup_templates, int64_t *dup_records,
                        int64_t *dup_sets);
int  tcmi_readset_duplicates(tcmi_ctx *ctx, const tcmi_readset *rs, uint8_t *out, int64_t cap, int64_t *n);
/* ---- variant table (additive: what `ivar variants` reports; the reference has only the consensus and its -vcf) ---------------
 * Every non-reference allele of a position at or above a frequency, with its depth, taken from the count matrix where it lies.
 * All arithmetic is integer.  With the matrix (plane order TCMI_COV..TCMI_I), a reference byte string ref[0..n_ref) on the
 * matrix's axis, min_af = num / den as a reduced fraction (0 <= num <= den, 1 <= den <= 1 000 000), min_alt_depth in 1..2^31-1
 * and min_depth in 0..2^31-1:
 *   position p (0-based) gives NO record when p >= n_ref, when ref[p] is not one of ACGTacgt (N, IUPAC codes, the zero bytes of a
 *   contig layout's guard, columns beyond the FASTA) or when cov < max(min_depth, 1);
 *   otherwise allele a of A, T, C, G, X, I that is not the upper-cased reference base gives one record iff
 *   count[a] >= min_alt_depth and count[a] * den >= num * cov (64-bit products; an exact tie is in).
 * X and I are never the reference allele: at most 5 records per position.  Records ascend by position, then by allele in plane
 * order A, T, C, G, X, I; the order is part of the contract (no atomics take part: every run gives the same bytes).
 * X is per column (a read that deletes this column); I is the insertion mark on the token IN FRONT of the insertion: the table says
 * how many reads, not which bases (those come from the insert-candidate sweeps, with their own filters).
 *   tcmi_variants_dev   the matrix and the reference are the caller's device pointers; d_counts as for tcmi_call_dev (4-byte aligned,
 *                     any ld >= L) and only read; d_ref may be NULL when n_ref = 0.  d_records: room for `cap` records, aligned
 *                     to 4 bytes, device or pinned host memory.  *n_found = the records the rule yields, whatever cap is; when
 *                     *n_found > cap the first cap records are written, nothing behind them, and the call returns TCMI_E_ARG (as
 *                     tcmi_readset_ins_entries does with its buffers); cap = 0 with d_records = NULL only counts.  Waits for the
 *                     context's stream.
 *   tcmi_variants       host convenience, shaped like tcmi_call: rows [L][7] and a host reference in, host records out
 *   tcmi_ctx_set_variants   ref == NULL clears the setting; else the context keeps a device copy of ref[0..n_ref) and from now on
 *                     every step it queues through tcmi_step_begin (tcmi_step, tcmi_bamfile_step on both of its routes) launches
 *                     the table's three kernels behind the tally and in front of the call kernel (which may zero the matrix); the
 *                     records go to pinned memory of the context sized 5 * n_ref, which cannot overflow.  While a setting is in force the
 *                     array pipeline (tcmi_pipeline_run[_batched], whose steps ride along) refuses with TCMI_E_UNSUPPORTED and a
 *                     message naming --variant-table, never skipping the table silently.  tcmi_split_step is not governed: its
 *                     matrix is the caller's (tcmi_variants_dev / tcmi_variants).  No setting: exactly the launches of before.
 *   tcmi_step_variants  the records of the last step that was ended, valid until the context's next step; TCMI_E_ARG when that step
 *                     computed none
 *   tcmi_variants_text  HOST, re-entrant, no GPU (and no error text: the code says it all): the ONE writer of the table's rows.
 *                     Per record "REGION<TAB>POS<TAB>REF<TAB>ALT<TAB>ALT_DP<TAB>TOTAL_DP<TAB>ALT_FREQ<NL>": POS = pos - pos_offset + 1,
 *                     REF = ref[pos] upper-cased (ref on the records' axis, n_ref bytes), ALT = the base letter, '*' for X, '+' for I,
 *                     ALT_FREQ = ALT_DP / TOTAL_DP as a double printed with %.6f.  The header line (TCMI_VARIANTS_HEADER) is the
 *                     caller's.  *len = the bytes the rows take.  text = NULL with cap = 0 is the sizing call: TCMI_OK and
 *                     *len.  With a buffer, TCMI_E_ARG when the rows take more than cap (nothing useful is written; *len says how
 *                     much).  Always TCMI_E_ARG for a record that does not fit the arguments (pos outside [pos_offset, n_ref),
 *                     allele outside 1..6, cov <= 0).
 * Argument errors are TCMI_E_ARG: den outside 1..10^6, num outside 0..den, min_alt_depth < 1, min_depth < 0, negative sizes. */
typedef struct tcmi_variant { int32_t pos /* 0-based */, allele /* TCMI_A..TCMI_I */, count, cov; } tcmi_variant;
#define TCMI_VARIANTS_HEADER "REGION\tPOS\tREF\tALT\tALT_DP\tTOTAL_DP\tALT_FREQ\n"
int  tcmi_variants_dev(tcmi_ctx *ctx, const void *d_counts, int64_t L, int64_t ld, const void *d_ref, int64_t n_ref, int64_t num, int64_t den,
                       int32_t min_alt_depth, int32_t min_depth, void *d_records, int64_t cap, int64_t *n_found);
int  tcmi_variants(tcmi_ctx *ctx, const int32_t *counts, int64_t L, const uint8_t *ref, int64_t n_ref, int64_t num, int64_t den,
                   int32_t min_alt_depth, int32_t min_depth, tcmi_variant *records, int64_t cap, int64_t *n_found);
int  tcmi_ctx_set_variants(tcmi_ctx *ctx, const uint8_t *ref, int64_t n_ref, int64_t num, int64_t den, int32_t min_alt_depth, int32_t min_depth);
int  tcmi_step_variants(tcmi_ctx *ctx, const tcmi_variant **records, int64_t *n);
int  tcmi_variants_text(const tcmi_variant *records, int64_t n, const char *region, int64_t pos_offset, const uint8_t *ref, int64_t n_ref,
                        char *text, int64_t cap, int64_t *len);
/* ---- amplicon table (additive: what `samtools ampliconstats` reports as FDEPTH / FPCOV; the reference has only the coverage TSV) ----
 * Order statistics of the matrix's coverage plane (TCMI_COV; no other plane is read) over n intervals [start[i], end[i]) of the
 * matrix's axis, 0 <= start <= end <= 2^29, n <= 65 536, and a bound min_depth >= 0.  Intervals may overlap, nest, repeat, be empty
 * and come in any order.  A position p >= L has depth 0; nothing at or beyond L is read (the padding [L, ld) may hold anything).
 * Depths are compared as signed int32.  One 32-byte record per interval, in the order given; an empty interval gives
 * {0, 0, 0, -1, 0, 0, 0}.  All arithmetic is integer and no atomics on memory take part: every run gives the same bytes.
 *   tcmi_interval_stats_dev  the matrix, the interval arrays (int64) and the records are the caller's device pointers; d_counts as for
 *                     tcmi_call_dev (4-byte aligned, any ld >= L) and only read; d_records: 4-byte aligned, device or pinned host
 *                     memory, room for n records; d_start and d_end: 8-byte aligned (TCMI_E_ARG otherwise).  The intervals are checked on the host (the call downloads them: 16 bytes
 *                     each).  Waits for the context's stream.  n = 0 does nothing.
 *   tcmi_interval_stats      host convenience, shaped like tcmi_variants: rows [L][7] and host intervals in, host records out
 *   tcmi_ctx_set_intervals   n = 0 clears the setting; else the context keeps a device copy of the intervals and from now on every
 *                     step it queues through tcmi_step_begin (tcmi_step, tcmi_bamfile_step on both of its routes) launches the
 *                     kernel behind the tally and in front of the call kernel (which may zero the matrix), beside the variant
 *                     table's launches; the records go to pinned memory of the context sized n, and tcmi_step_end's one wait
 *                     covers them.  While a setting is in force the array pipeline (tcmi_pipeline_run[_batched]) refuses with
 *                     TCMI_E_UNSUPPORTED and a message naming --amplicon-table.  tcmi_split_step is not governed: its matrix is
 *                     the caller's (tcmi_interval_stats_dev / tcmi_interval_stats).  No setting: exactly the launches of before.
 *   tcmi_step_intervals      the records of the last step that was ended, valid until the context's next step or setting;
 *                     TCMI_E_ARG when that step computed none
 *   tcmi_amplicons_text      HOST, re-entrant, no GPU (and no error text: the code says it all): the ONE writer of the table's rows.
 *                     Per record "SAMPLE REGION AMPLICON POOL START END LEN MEAN MEDIAN MIN MIN_POS BELOW", tab-separated:
 *                     AMPLICON = names[i], POOL = pools[i], START = start[i] - pos_offset + 1 (start: the intervals' starts on the
 *                     records' axis), END = START + LEN - 1 (inclusive), LEN = n, MEAN = sum / n as a double printed with %.2f,
 *                     MIN_POS = min_pos - pos_offset + 1.  An empty interval prints END = START - 1, LEN 0, NA for MEAN, MEDIAN,
 *                     MIN and MIN_POS, BELOW 0.  The header line (TCMI_AMPLICONS_HEADER) is the caller's.  Sizing call, short
 *                     buffer and *len as for tcmi_variants_text.  TCMI_E_ARG for a record that does not fit the arguments
 *                     (start[i] < pos_offset, n < 0, n > 0 with min_pos outside [start[i], start[i] + n)).
 * TCMI_INTERVAL_STAGE: the columns of an interval the kernel stages in LDS (a longer one is selected from memory); for tests.
 * Argument errors are TCMI_E_ARG: n outside 0..65 536, start < 0, end < start, end > 2^29, min_depth < 0, negative sizes. */
typedef struct tcmi_interval_stat {
    int64_t sum;                      /* of the depths; int64: 2^31-1 times thousands of columns */
    int32_t n;                        /* end - start */
    int32_t min, min_pos;             /* the smallest depth and the FIRST position that has it */
    int32_t median;                   /* the LOWER median: the ((n-1)/2)-th smallest, exact */
    int32_t below;                    /* positions with depth < min_depth */
    int32_t reserved;                 /* 0 */
} tcmi_interval_stat;
#define TCMI_AMPLICONS_HEADER "SAMPLE\tREGION\tAMPLICON\tPOOL\tSTART\tEND\tLEN\tMEAN\tMEDIAN\tMIN\tMIN_POS\tBELOW\n"
#define TCMI_INTERVAL_STAGE 4096
int  tcmi_interval_stats_dev(tcmi_ctx *ctx, const void *d_counts, int64_t L, int64_t ld, int64_t n, const void *d_start, const void *d_end,
                             int32_t min_depth, void *d_records);
int  tcmi_interval_stats(tcmi_ctx *ctx, const int32_t *counts, int64_t L, int64_t n, const int64_t *start, const int64_t *end,
                         int32_t min_depth, tcmi_interval_stat *records);
int  tcmi_ctx_set_intervals(tcmi_ctx *ctx, int64_t n, const int64_t *start, const int64_t *end, int32_t min_depth);
int  tcmi_step_intervals(tcmi_ctx *ctx, const tcmi_interval_stat **records, int64_t *n);
int  tcmi_amplicons_text(const tcmi_interval_stat *records, int64_t n, const char *sample, const char *region, const char *const *names,
                         const char *const *pools, const int64_t *start, int64_t pos_offset, char *text, int64_t cap, int64_t *len);
/* ---- amplicon reads (additive: what `samtools ampliconstats` reports as FREADS; the reference has nothing like it) ----------------
 * How many RECORDS of a device-decoded read set belong to which amplicon of a primer scheme, counted by one HIP kernel over the
 * inflated record stream the read set left resident on its context.  The count matrix cannot say this: a column's depth does not say
 * which amplicon its reads came from.  All arithmetic is integer; the sums are the same in every run.
 *   amplicon i     four numbers on the count matrix's axis (under a contig layout: shifted by its contig's slot): fs[i] the smallest
 *                  LEFT start, le[i] the largest LEFT end, rs[i] the smallest RIGHT start, fe[i] the largest RIGHT end, with
 *                  fs < le, rs < fe, fs < fe (le > rs, overlapping primers, is legal).  With slack s in 0..1000 its widened extent
 *                  is a = fs - s (may be negative), b = fe + s.  Amplicons may overlap, nest and repeat.
 *   kept record    exactly what the device packer keeps: not FLAG 0x4, passes the read filter the read set was built under, its
 *                  reference has a slot (shift >= 0), pos >= 0, a consistent record, a reference span > 0.  Its first column is
 *                  p = pos + shift, its last q = p + (the M, D, N, =, X lengths) - 1.  Records are counted, not templates; a long
 *                  read that the packed set leaves out counts once.  The primer mask and the base-quality floor skip tokens, not
 *                  reads: they do not enter.
 *   containment    the read is contained in amplicon i iff a_i <= p and q < b_i.  In exactly one amplicon i: records[i].reads += 1,
 *                  and records[i].full += 1 iff also p < le_i and q >= rs_i (it starts in the left primer zone and ends in the right
 *                  one).  In two or more: records[n].reads += 1 (ambiguous; two identical amplicons make all their reads ambiguous).
 *                  In none: records[n + 1].reads += 1 (unassigned).  records[n].full = records[n + 1].full = 0.
 *   invariant      the sum of all n + 2 `reads` equals the number of kept records.
 *   tcmi_readset_amplicon_reads   records: host, room for n + 2.  The read set must have been decoded on the device and its stream must
 *                  still be resident on this context — no other upload since (the same arena epoch), the same device, the same
 *                  layout generation —, else TCMI_E_UNSUPPORTED with words that name the cause.  Long reads and contig layouts are
 *                  supported (the kernel reads the stream, not the packed set).  A read set of sub-ranges (tcmi_split_step,
 *                  "split_sub") answers with the sum over its parts, each counted on its own context.  Waits for the stream.  The
 *                  scratch is the context's, grow-only.
 *   tcmi_amplicon_reads_compile   (GPU-free) the int32 table the kernel searches, 6 n words, six dense arrays one behind the other:
 *                  a[n] the widened starts ascending (ties in the order given); bmax[n], idx[n], b2[n]: of the first k + 1 sorted
 *                  amplicons the largest b, the index (in the order given) of the first that has it, and the second largest b
 *                  counted with multiplicity (INT32_MIN for k = 0); le[n], rs[n] in the order given.  Lookup (p, q): k = the number
 *                  of a <= p; none iff k = 0 or bmax[k - 1] <= q; ambiguous iff k >= 2 and b2[k - 1] > q; else idx[k - 1].
 *                  table_cap: room in words; msg (may be NULL) receives the words of a TCMI_E_ARG.
 * TCMI_AMPLICON_READS_LDS: the amplicons whose table and counters a workgroup stages in LDS (16 KiB: eight workgroups per compute
 * unit); a larger table is searched, and counted, in memory; for tests.
 * Argument errors are TCMI_E_ARG: n outside 1..65 536, a coordinate outside [0, 2^29], the inequalities above, slack outside 0..1000. */
typedef struct tcmi_amplicon_reads { int64_t reads, full; } tcmi_amplicon_reads;
#define TCMI_AMPLICON_READS_LDS 512
int  tcmi_readset_amplicon_reads(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t n, const int64_t *fs, const int64_t *le, const int64_t *rs_,
                                 const int64_t *fe, int32_t slack, tcmi_amplicon_reads *records /* host, n + 2 */);
int  tcmi_amplicon_reads_compile(int64_t n, const int64_t *fs, const int64_t *le, const int64_t *rs_, const int64_t *fe, int32_t slack,
                                 int32_t *table, int64_t table_cap, char *msg, int64_t msg_cap);
/* ---- strand counts (additive: what `ivar variants` reports as REF_RV / ALT_RV; the reference has nothing like it) -------------------
 * The count matrix's seven planes at given columns, split by the strand of the record (FLAG 0x10), counted by one HIP kernel over the
 * inflated record stream a device-decoded read set left resident on its context.  The matrix sums the strands and the packed read set
 * does not keep the flag: the strand lives in the records only.  All arithmetic is integer; the sums are the same in every run.
 *   columns        c_0 < c_1 < ... < c_{n-1} on the count matrix's axis (under a contig layout: shifted by the contig's slot), each in
 *                  [0, 2^29), n in 1..2^20.
 *   fwd[k], rev[k] for k in plane order TCMI_COV..TCMI_I: the value the count matrix would hold at (k, c_i) had the read set been built
 *                  from the same records minus those with FLAG 0x10 set (fwd), minus those with it clear (rev) - under the read
 *                  filter, the base-quality floor, the primer table and the contig layout the read set REMEMBERS, whatever the
 *                  context is set to later.  The token rule is the count matrix's: a matched base counts by its letter; a deleted
 *                  column counts X unless it is the last column of a deletion with an insertion behind it; the I mark goes to the
 *                  last reference column in front of an insertion, iff that token is not skipped; M, =, X, D and N count coverage;
 *                  the floor and the primer mask skip tokens per column as described above.  Every kept record takes part (what
 *                  tcmi_readset_amplicon_reads calls kept), packed reads and long reads alike.  A column nobody covers gives zeros.
 *   invariant      fwd[k] + rev[k] equals the count matrix a step tallies from the read set, at (k, c_i), on all seven planes.
 *   tcmi_readset_strand_counts   records: host, room for n; pos = c_i, reserved = 0.  Residency as for tcmi_readset_amplicon_reads:
 *                  decoded on the device, the same arena epoch, device and layout generation, else TCMI_E_UNSUPPORTED with words that
 *                  name the cause.  A read set of sub-ranges answers with the sum over its parts, each counted on its own context.  A
 *                  read set without a kept record gives zero records and TCMI_OK.  Waits for the stream.  The scratch is the
 *                  context's, grow-only.
 *   tcmi_strand_verdict   HOST, GPU-free, exact integers.  0 PASS, 1 BIAS, 2 LOW.  LOW iff tot_fwd < min_strand_depth or
 *                  tot_rev < min_strand_depth.  Else with x = alt_fwd * tot_rev, y = alt_rev * tot_fwd (the two strand frequencies
 *                  cross-multiplied), lo = min(x, y), hi = max(x, y): BIAS iff lo * den < hi * num (an exact tie is PASS; num = 0
 *                  never gives BIAS).  The products take more than 64 bits: they are formed in 128.  TCMI_E_ARG for a negative
 *                  count and the range errors below.
 *   tcmi_variants_strand_text   HOST, re-entrant, no GPU: the writer of --variant-strand's rows.  The first seven fields of a row are
 *                  byte for byte tcmi_variants_text's for the record; behind them REF_FWD REF_REV (the plane of the upper-cased
 *                  reference base), ALT_FWD ALT_REV (the record's allele), TOTAL_FWD TOTAL_REV (coverage) and STRAND = PASS, BIAS
 *                  or LOW.  strand[0..n_cols): the counts at the records' distinct positions, ascending.  TCMI_E_ARG when
 *                  strand[j].pos is not the records' j-th distinct position (or n_cols is not their number), and when a record has
 *                  alt_fwd + alt_rev != count or tot_fwd + tot_rev != cov: the two kernels disagree, no table is written.  Sizing
 *                  call, short buffer and *len as for tcmi_variants_text.  The header line (TCMI_VARIANTS_STRAND_HEADER) is the
 *                  caller's.
 * TCMI_STRAND_LDS: the columns whose list and counters a workgroup stages in LDS (15 KiB: ten workgroups per compute unit by LDS);
 * a longer list is searched, and counted, in memory; for tests.
 * Range errors are TCMI_E_ARG: min_strand_depth < 1, den outside 1..10^6, num outside 0..den. */
typedef struct tcmi_strand_counts { int32_t fwd[7], rev[7]; int32_t pos, reserved /* 0 */; } tcmi_strand_counts;   /* 64 bytes */
#define TCMI_STRAND_LDS 256
#define TCMI_VARIANTS_STRAND_HEADER "REGION\tPOS\tREF\tALT\tALT_DP\tTOTAL_DP\tALT_FREQ\tREF_FWD\tREF_REV\tALT_FWD\tALT_REV\tTOTAL_FWD\tTOTAL_REV\tSTRAND\n"
int  tcmi_readset_strand_counts(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t n, const int64_t *cols /* host */,
                                tcmi_strand_counts *records /* host, n */);
int  tcmi_strand_verdict(int32_t alt_fwd, int32_t alt_rev, int32_t tot_fwd, int32_t tot_rev, int32_t min_strand_depth, int64_t num, int64_t den);
int  tcmi_variants_strand_text(const tcmi_variant *records, int64_t n, const tcmi_strand_counts *strand, int64_t n_cols, /* the records' distinct positions, ascending */
                               int32_t min_strand_depth, int64_t num, int64_t den, const char *region, int64_t pos_offset,
                               const uint8_t *ref, int64_t n_ref, char *text, int64_t cap, int64_t *len);
/* ---- link counts (additive: are two nearby alleles on the same molecules?  the reference has nothing like it) ----------------------
 * For pairs of nearby queried columns, the number of kept records by the class of their token at the first column AND at the second,
 * counted by one HIP kernel over the inflated record stream a device-decoded read set left resident on its context.  The count matrix
 * forgets which read a token came from: every row of the variant table stands alone, and only the records can say whether two minority
 * alleles are one haplotype (cis), two populations (trans) or a multi-nucleotide change inside a codon.  All arithmetic is integer;
 * the sums are the same in every run.  RECORDS are counted, not templates: the two mates of a pair are two records, each with its own
 * columns, as for tcmi_readset_amplicon_reads.
 *   columns        c_0 < c_1 < ... < c_{n-1} on the count matrix's axis (under a contig layout: shifted by the contig's slot), each in
 *                  [0, 2^29); k neighbours in 1..7; n >= 1 and n * k <= 2^17.
 *   records        host, room for n * k.  records[i * k + d - 1] (d in 1..k) is the pair (c_i, c_{i+d}): a = c_i, b = c_{i+d},
 *                  reserved = 0; b = -1 and j all zero when i + d >= n.
 *   class          of a kept record at a column: 0 no token (the column lies outside the record's columns [p, q], the token is masked
 *                  by the primer table or lies below the base-quality floor); 1..4 a matched base counted on plane A, T, C, G; 5 a
 *                  deleted column that counts X; 6 a token that counts coverage and none of the planes 1..5 (an N or ambiguity
 *                  nibble, a query index past SEQ, a reference skip, a deletion's last column with an insertion behind it).  The
 *                  token rule is the count matrix's, as for tcmi_readset_strand_counts, under the read filter, the floor, the primer
 *                  table and the layout the read set REMEMBERS.  The I mark takes no part.
 *   j[x][y]        the kept records with class x at a and class y at b.  j[0][0] is always 0.
 *   invariant      for every pair with b >= 0: sum_y j[x][y] is the count matrix at (plane x, a) for x in 1..5 and cov minus the planes
 *                  1..5 at a for x = 6; the column sums sum_x j[x][y] are the same at b.
 *   tcmi_readset_link_counts   residency, sub-ranges, an empty read set, the wait and the scratch as for tcmi_readset_strand_counts.
 *   tcmi_link_phase   HOST, GPU-free, exact integers.  0 CIS, 1 TRANS, 2 MIXED, 3 NONE, 4 LOW.  LOW iff span < min_depth.  Else with
 *                  m = min(both + only_a, both + only_b): NONE iff m = 0; CIS iff both * den >= num * m; TRANS iff
 *                  both * den <= (den - num) * m; else MIXED.  num / den lies in (1/2, 1], so CIS and TRANS exclude each other.  The
 *                  counts stay below 2^31 and den at or below 10^6: the products fit 64 bits.  TCMI_E_ARG for a negative count and
 *                  the range errors below.
 *   tcmi_variants_links_text   HOST, re-entrant, no GPU: the writer of --variant-links' rows, one per pair of variant records (r1, r2)
 *                  where r2's position is among the next k distinct positions behind r1's and both alleles are in planes A..X ('+'
 *                  records are not linked: the I mark says that an insertion follows, not which).  All records of one call are one
 *                  region.  links[0 .. n_cols * k): the link counts at the records' distinct positions, ascending.  Row:
 *                  REGION POS_A REF_A ALT_A POS_B REF_B ALT_B SPAN BOTH ONLY_A ONLY_B NEITHER PHASE, alleles spelled as
 *                  tcmi_variants_text spells them; with A, B the two alleles' planes SPAN = sum_{x,y >= 1} j[x][y] (the records with a
 *                  token at both columns), BOTH = j[A][B], ONLY_A = sum_{y >= 1, y != B} j[A][y], ONLY_B = sum_{x >= 1, x != A}
 *                  j[x][B], NEITHER = SPAN - BOTH - ONLY_A - ONLY_B, PHASE = tcmi_link_phase's word.  TCMI_E_ARG, and no text, when
 *                  links[jx * k + d - 1].a is not the jx-th distinct position or .b not the (jx + d)-th (behind the last one: -1 or
 *                  any column beyond it, the next region's), when n_cols is not the number of distinct positions, and when the
 *                  invariant fails against a record's count or cov in any pair with b >= 0 its position takes part in: the two
 *                  kernels disagree, no table is written.  Sizing call, short buffer and *len as for tcmi_variants_text.  The header
 *                  line (TCMI_VARIANTS_LINKS_HEADER) is the caller's.
 * TCMI_LINKS_LDS: the pairs (n * k) whose counters, with the columns, a workgroup stages in LDS (80 x 49 counters + 80 columns = 16 000
 * bytes: ten workgroups per compute unit by LDS, eight by the launch shape); more pairs are counted with atomics in memory; for tests.
 * Range errors are TCMI_E_ARG: min_depth < 1, den outside 1..10^6, num > den or 2 * num <= den. */
typedef struct tcmi_link_counts { int32_t j[7][7]; int32_t a, b /* -1: no such pair */, reserved /* 0 */; } tcmi_link_counts;   /* 208 bytes */
#define TCMI_LINKS_LDS 80
#define TCMI_VARIANTS_LINKS_HEADER "REGION\tPOS_A\tREF_A\tALT_A\tPOS_B\tREF_B\tALT_B\tSPAN\tBOTH\tONLY_A\tONLY_B\tNEITHER\tPHASE\n"
int  tcmi_readset_link_counts(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t n, const int64_t *cols /* host */, int32_t k,
                              tcmi_link_counts *records /* host, n * k */);
int  tcmi_link_phase(int32_t both, int32_t only_a, int32_t only_b, int32_t span, int32_t min_depth, int64_t num, int64_t den);
int  tcmi_variants_links_text(const tcmi_variant *records, int64_t n, const tcmi_link_counts *links, int64_t n_cols, /* the records' distinct positions, ascending */
                              int32_t k, int32_t min_depth, int64_t num, int64_t den, const char *region, int64_t pos_offset,
                              const uint8_t *ref, int64_t n_ref, char *text, int64_t cap, int64_t *len);
/* ---- indel events (additive: what `ivar variants` prints as +ACG / -3; the reference has nothing like it) ----------------------------
 * The variant table's '+' row says how many records carry the insertion mark, not which bases; its '*' rows are single deleted columns.
 * Here every insertion and every deletion is ONE event with its length and, for an insertion, its bases — counted by three HIP
 * launches over the inflated record stream a device-decoded read set left resident on its context, in a keyed table on the device
 * (the keys are not known before the records are read).  All arithmetic is integer and every result is the same in every run.
 *   columns        c_0 < c_1 < ... < c_{n-1} on the count matrix's axis, each in [0, 2^29), n in 1..2^20, with cov[i] >= 0 the count
 *                  matrix's coverage at c_i (the variant records' cov).
 *   event          of a kept record (what tcmi_readset_amplicon_reads calls kept) at a queried column c, under the read filter, the
 *                  base-quality floor, the primer table and the layout the read set REMEMBERS:
 *                  INS (kind 1)  iff the record's token at c carries the I mark, i.e. exactly when it adds 1 to the count matrix's I
 *                      plane at c.  len = the inserted bases: those of the I ops behind the op that holds c, up to the next op that is
 *                      neither I nor P when an I op follows directly, up to the next reference-consuming op when a P op follows (S ops
 *                      between consume query, H and P do not) — htslib's rule, the count matrix's.  The bases are those ops' query
 *                      nibbles in CIGAR order; a query index at or beyond l_seq (SEQ '*') reads as nibble 15, 'N'.  Two insertions
 *                      are the same event iff len and every nibble are equal: IUPAC codes are not merged.
 *                  DEL (kind 2)  iff the op that holds c is a D op, c is its first column, and the record's token at c is counted at
 *                      all (not masked by the primer table, not below the floor: a D token is tested at the query index at which its op
 *                      starts).  len = that op's length.  ONE D OP IS ONE EVENT: adjacent D ops ("3D2D", which no aligner writes) are
 *                      two events, at their own first columns.  A record may give both at one column ("1D" followed by "I").
 *   totals         per queried column ins_total, del_total: the events of each kind anchored there, reported or not.
 *   invariant      ins_total[i] equals the count matrix's I plane at c_i.  For deletions only del_total[i] <= cov[i] holds: a "1D" + I
 *                  token counts I and not X, a primer mask may cut a deletion behind its first column (its later columns are '*' rows
 *                  without an event), and a column inside a longer deletion counts X without anchoring one.
 *   reported       an event with `count` records on a column of coverage cov iff cov >= max(min_depth, 1), count >= min_alt_depth and
 *                  count * den >= num * cov (64-bit products, an exact tie is in): the variant table's rule.  The rule is applied on
 *                  the device: only reported events are downloaded.  tcmi_indel_passes is its GPU-free twin (1 / 0, TCMI_E_ARG for
 *                  a negative count or coverage and the range errors below).
 *   tcmi_readset_indel_events   events: host, room for cap; text: host, room for text_cap letters, one per inserted base from
 *                  "=ACMGRSVTWYHKDBN"; totals: host, room for n (pos = c_i).  The events come in THE order (pos, kind, len, bases):
 *                  every run gives the same bytes.  An INS event's bases are text[text_off .. text_off + len); a DEL's text_off is
 *                  -1.  *n_found and *text_len always say how much there is; when either exceeds its capacity nothing is written to
 *                  events or text and the call returns TCMI_E_ARG, except for the sizing call (events = text = NULL, cap =
 *                  text_cap = 0), which returns TCMI_OK.  totals are written either way.  Residency, an empty read set (zero events,
 *                  TCMI_OK) and the scratch as for tcmi_readset_strand_counts; a read set of sub-ranges is counted part by part, each
 *                  on its own context without the rule, equal events are merged on the host and the rule is applied there.  Waits for
 *                  the stream once per attempt and once for the download.
 *   exactness      an insertion's key in the table is a 34-bit hash of its length and bases; a second pass over the records compares
 *                  every insertion with its slot's representative (the first record, in file order, that claimed it).  When two
 *                  different insertions of one column share a key the call starts over with the next of four seeds, then fails with
 *                  TCMI_E_UNSUPPORTED; when the table (2^"indel_slots" slots, default 2^15) overflows or a probe runs 64 steps it
 *                  starts over eight times as large, up to 2^24 slots, then fails with TCMI_E_UNSUPPORTED.  A returned result is
 *                  therefore always exact.  Options, for tests: "indel_slots" (4..24), "indel_hash_bits" (0..34, the rest of the hash
 *                  is zero); counters: "indel_table_grown", "indel_hash_retried".
 *   tcmi_indel_hash   HOST: the hash of an insertion, nibbles one code (0..15) per byte, bits in 0..34.
 *   tcmi_indels_text   HOST, re-entrant, no GPU: the one writer of --indel-table's rows.  All events of one call are one region.  Row:
 *                  REGION POS TYPE LEN SEQ COUNT TOTAL_DP FREQ.  TYPE is INS or DEL.  POS of an INS is the 1-based position of the
 *                  base in front of the insertion (the '+' row's POS), of a DEL the first deleted base (the first '*' row's POS).  SEQ
 *                  of an INS are the inserted bases, of a DEL the deleted reference bases, upper-cased, N beyond the reference.  FREQ =
 *                  COUNT / TOTAL_DP as a double printed with %.6f.  totals[0..n_cols): the totals at the distinct positions of the
 *                  '*' and '+' records among `records`, ascending.  TCMI_E_ARG, and no text, when totals[j].pos is not the j-th such
 *                  position (or n_cols is not their number); when a '+' record's count is not ins_total at its position or
 *                  del_total exceeds a record's cov there (the stream kernels and the matrix's disagree); when an event lies on no
 *                  such position, its cov is not the records', its count exceeds its kind's total, its bases lie outside text or
 *                  are no such letters, or the events are not in THE order.  Sizing call, short buffer and *len as for
 *                  tcmi_variants_text.  The header line (TCMI_INDELS_HEADER) is the caller's.
 * TCMI_INDEL_LDS: the columns whose list and totals a workgroup stages in LDS (6 KiB); a longer list is searched, and its totals are
 * counted, in memory; for tests.
 * Range errors are TCMI_E_ARG: den outside 1..10^6, num outside 0..den, min_alt_depth < 1, min_depth < 0, a negative cov. */
typedef struct tcmi_indel_event { int32_t pos, kind /* 1 INS, 2 DEL */, len, count, cov, reserved /* 0 */; int64_t text_off /* INS: into text; DEL: -1 */; } tcmi_indel_event;   /* 32 bytes */
typedef struct tcmi_indel_totals { int32_t pos, ins_total, del_total, reserved /* 0 */; } tcmi_indel_totals;   /* 16 bytes */
#define TCMI_INDEL_LDS 512
#define TCMI_INDELS_HEADER "REGION\tPOS\tTYPE\tLEN\tSEQ\tCOUNT\tTOTAL_DP\tFREQ\n"
int  tcmi_readset_indel_events(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t n, const int64_t *cols /* host */, const int32_t *cov /* host, n */,
                               int64_t num, int64_t den, int32_t min_alt_depth, int32_t min_depth, tcmi_indel_event *events /* host, cap */,
                               int64_t cap, int64_t *n_found, char *text /* host, text_cap */, int64_t text_cap, int64_t *text_len,
                               tcmi_indel_totals *totals /* host, n */);
uint64_t tcmi_indel_hash(uint32_t seed, int32_t len, const uint8_t *nibbles /* one code per byte */, int32_t bits);
int  tcmi_indel_passes(int32_t count, int32_t cov, int64_t num, int64_t den, int32_t min_alt_depth, int32_t min_depth);
int  tcmi_indels_text(const tcmi_indel_event *events, int64_t n, const char *text, int64_t text_len, const tcmi_indel_totals *totals,
                      int64_t n_cols, const tcmi_variant *records, int64_t n_records, const char *region, int64_t pos_offset,
                      const uint8_t *ref, int64_t n_ref, char *out, int64_t cap, int64_t *len);
/* ---- allele evidence (additive: `ivar variants`' REF_QUAL / ALT_QUAL, and the mapping-quality and read-position annotations that
 *      lofreq and GATK filter on; the reference has nothing like it) ------------------------------------------------------------------
 * Per queried column and plane of the count matrix: how many tokens, and the sums of their base quality, of their records' MAPQ and of
 * their distance to the nearer end of the read's aligned part — counted by one HIP kernel over the inflated record stream a
 * device-decoded read set left resident on its context.  The count matrix and the packed read set keep neither QUAL per token, nor MAPQ,
 * nor the query index: the evidence lives in the records only.  All arithmetic is integer; the sums are the same in every run.
 *   columns        c_0 < c_1 < ... < c_{n-1} on the count matrix's axis (under a contig layout: shifted by the contig's slot), each in
 *                  [0, 2^29), n in 1..2^20.
 *   token          the count matrix's, as for tcmi_readset_strand_counts: a token counts here exactly when it counts in the matrix,
 *                  under the read filter, the base-quality floor, the primer table and the contig layout the read set REMEMBERS.  For
 *                  every plane k (TCMI_COV..TCMI_I) the token adds to, four counters of (c_i, k) grow:
 *   n[k]           by 1: the count matrix at (k, c_i).
 *   qual[k]        by the token's quality byte as the file stores it: the byte the floor tests, at query index qi — of a matched base
 *                  its own, of a D / N token the index at which its op starts; an index at or beyond l_seq gives 0, a record without
 *                  QUAL its stored 0xFF.  The byte is read whatever the floor.
 *   mapq[k]        by the record's MAPQ as stored (255 included).
 *   dist[k]        by min(255, max(0, min(qi - a0, a1 - 1 - qi))): [a0, a1) is the aligned part of the query — a0 the total length of the
 *                  S ops in front of the first op that is neither S nor H, a1 the sum of all query-consuming ops minus the S ops behind
 *                  the last op that is neither S nor H.  Both come from the CIGAR alone: l_seq plays no part, and neither does the
 *                  primer table (the distance is to the read's end, not to the mask's).  A D op that starts at a1 gives 0; the cap
 *                  keeps every token's value in a byte (255 bases from either end is as far as any filter asks).
 *   invariant      n[k] equals the count matrix a step tallies from the read set, at (k, c_i), on all seven planes.
 *   tcmi_readset_evidence_counts   records: host, room for n; pos = c_i.  Residency, sub-ranges, an empty read set (zeros, TCMI_OK),
 *                  the wait and the scratch as for tcmi_readset_strand_counts.
 *   tcmi_evidence_verdict   HOST, GPU-free, exact integers (128-bit products).  A bit set: 1 LOWQ iff qual < min_qual * n, 2 LOWMQ iff
 *                  mapq < min_mapq * n, 4 END iff dist < min_dist * n — the mean lies below the threshold.  A threshold of 0 switches
 *                  its bit off; n = 0 gives 0.  TCMI_E_ARG for a negative count or sum and the range errors below.
 *   tcmi_variants_evidence_text   HOST, re-entrant, no GPU: the writer of --variant-evidence's rows.  The first seven fields of a row are
 *                  byte for byte tcmi_variants_text's for the record; behind them REF_QUAL ALT_QUAL REF_MAPQ ALT_MAPQ REF_ENDDIST
 *                  ALT_ENDDIST — REF the plane of the upper-cased reference base (zeros when it is none of A, T, C, G), ALT the
 *                  record's allele plane (X for '*' rows, I for '+' rows); each a mean sum / n cut to one decimal in integers,
 *                  (10 * sum) / n printed as %lld.%lld, 0.0 when n = 0 — and EVIDENCE = PASS, or the failing names of the ALT allele
 *                  in the order LOWQ, LOWMQ, END, joined by commas.  ev[0..n_cols): the counts at the records' distinct positions,
 *                  ascending.  TCMI_E_ARG, and NOTHING written (*len = 0), when ev[j].pos is not the records' j-th distinct position
 *                  (or n_cols is not their number), when n[allele] differs from a record's count or n[TCMI_COV] from its cov (the
 *                  stream kernel and the matrix's disagree: no table), and when a sum is negative or above 255 * n.  Sizing call and
 *                  *len as for tcmi_variants_text; a short buffer gets *len, TCMI_E_ARG and nothing written.  The header line (TCMI_VARIANTS_EVIDENCE_HEADER) is the caller's.
 * TCMI_EVIDENCE_LDS: the columns whose list and [28] counters a workgroup stages in LDS as uint32 (14.5 KiB: eight workgroups per
 * compute unit, as the launch shape asks); a longer list is searched, and counted, in memory — as is any query on a stream so long
 * that 255 times the records one workgroup visits could pass 2^32 - 1.  The tests query on both sides of the edge.
 * Range errors are TCMI_E_ARG: a threshold outside 0..255. */
typedef struct tcmi_evidence_counts { int64_t qual[7], mapq[7], dist[7]; int32_t n[7]; int32_t pos; } tcmi_evidence_counts;   /* 200 bytes */
#define TCMI_EVIDENCE_LDS 128
#define TCMI_VARIANTS_EVIDENCE_HEADER "REGION\tPOS\tREF\tALT\tALT_DP\tTOTAL_DP\tALT_FREQ\tREF_QUAL\tALT_QUAL\tREF_MAPQ\tALT_MAPQ\tREF_ENDDIST\tALT_ENDDIST\tEVIDENCE\n"
int  tcmi_readset_evidence_counts(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t n, const int64_t *cols /* host */,
                                  tcmi_evidence_counts *records /* host, n */);
int  tcmi_evidence_verdict(int64_t n, int64_t qual, int64_t mapq, int64_t dist, int32_t min_qual, int32_t min_mapq, int32_t min_dist);
int  tcmi_variants_evidence_text(const tcmi_variant *records, int64_t n, const tcmi_evidence_counts *ev, int64_t n_cols, /* the records' distinct positions, ascending */
                                 int32_t min_qual, int32_t min_mapq, int32_t min_dist, const char *region, int64_t pos_offset,
                                 const uint8_t *ref, int64_t n_ref, char *text, int64_t cap, int64_t *len);
/* ---- codon counts (additive: what do the variant table's rows mean for the protein?  the reference has nothing like it) -------------
 * For queried codons — three adjacent columns of the count matrix's axis — the number of kept records by the class of their token at the
 * first column AND the second AND the third, counted by one HIP kernel over the inflated record stream a device-decoded read set left
 * resident on its context.  Translating every row of the variant table on its own is wrong whenever two rows fall into one codon
 * (SARS-CoV-2's N:R203K/G204R, GGG -> AAC): the count matrix forgets which read a token came from, only the records know the triplet a
 * molecule carries.  All arithmetic is integer; the sums are the same in every run.  RECORDS are counted, not templates.
 *   codons         c0_0 < c0_1 < ... < c0_{n-1}: the first columns on the count matrix's axis (under a contig layout: shifted by the
 *                  contig's slot), each in [0, 2^29 - 2), n in 1..16 384.  Codon e is the columns c0_e, c0_e + 1, c0_e + 2.
 *                  Consecutive c0 may differ by 1 or 2: overlapping reading frames are ordinary in viruses.
 *   class          tcmi_readset_link_counts' seven, under the read filter, the floor, the primer table, the mate rule, the duplicate
 *                  rule and the layout the read set REMEMBERS.
 *   j[t0][t1][t2]  the kept records with those classes at the three columns.  j[0][0][0] is always 0.
 *   ins_inside     the records counted in j whose token at the first or the second column carries the I mark: inserted bases lie inside
 *                  the codon, the record is frame-shifted there.  They stay in j.  An I mark on the third column is not inside.
 *   pos, reserved  c0_e and 0.
 *   invariant      for every codon, slot k in 0..2 and class x in 1..6: the sum of j with class x at slot k is the count matrix at
 *                  (plane x, c0 + k) for x in 1..5, and cov minus the planes 1..5 there for x = 6.
 *   tcmi_readset_codon_counts   residency, sub-ranges, an empty read set (zeros, TCMI_OK), the wait and the scratch as for
 *                  tcmi_readset_link_counts.  Its launch is timed under TCMI_K_LINK_COUNTS.
 *   tcmi_cds       one reading frame: a GFF row of type CDS on the axis' columns [start, end), strand +1 or -1, phase 0..2.  On +1 the
 *                  codons are the consecutive triplets from start + phase upward, on -1 from end - 1 - phase downward; an incomplete
 *                  last triplet is dropped.  A CDS written as several rows is several frames, each trusted for its own phase; the
 *                  codon that straddles two rows is not reported.  On the axis a codon is three adjacent columns, the lowest its c0.
 *   tcmi_codon_aa  HOST: three planes TCMI_A..TCMI_G in coding order -> the amino acid's letter in the standard genetic code, '*' for a
 *                  stop; anything else: 'X'.
 *   tcmi_codon_select   HOST: the distinct c0, ascending, of the frames' codons that hold at least one of `records` (ascending by pos)
 *                  with an allele in planes A..X ('+' rows do not select, as they do not link).  *n_found always says how many there
 *                  are; more than cap: nothing written and TCMI_E_ARG, except for the sizing call (c0 = NULL, cap = 0).
 *   tcmi_codons_text   HOST, re-entrant, no GPU: the writer of --codon-table's rows, one per (frame, counted codon inside it, reported
 *                  triplet).  counts[0..n): ascending by pos; names[f]: frame f's FEATURE; matrix: the count matrix ([TCMI_NCOL][ld],
 *                  L columns), which the invariant is checked against — a codon's neighbour columns need not have a variant record; a
 *                  column >= L has depth 0.  Row:
 *                  REGION FEATURE STRAND CODON POS REF_CODON REF_AA ALT_CODON ALT_AA EFFECT SUBS COUNT SPAN FREQ PARTIAL OTHER INS_INSIDE.
 *                  CODON: the 1-based number of the codon in its frame, in coding direction; POS = c0 - pos_offset + 1; the codons in
 *                  coding orientation (on -: the complement of the columns in descending order; a reference base outside A, C, G, T,
 *                  or beyond n_ref: N).  SPAN = the records with a class >= 1 at all three columns.  A complete triplet has all three
 *                  classes in 1..4, or all three 5: spelled ---, ALT_AA -, EFFECT DEL.  COUNT: its records; FREQ = COUNT / SPAN with
 *                  %.6f; OTHER = SPAN minus all complete triplets' counts (mixed deletions, N, bases past SEQ); PARTIAL = the records
 *                  with class 0 at one or two of the columns.  A complete triplet other than the reference codon is reported iff
 *                  COUNT >= min_alt_depth, COUNT * den >= num * SPAN and SPAN >= min_depth: the variant table's thresholds and exact
 *                  integer rule.  SUBS: the differing bases, 1..3; 0 for ---.  EFFECT: SYN, MIS, STOP_GAINED, STOP_LOST, DEL, or
 *                  UNKNOWN (a reference codon with a base outside A, C, G, T: REF_AA X).  Rows: POS ascending, then the frames in the
 *                  order given, then COUNT descending, then the triplet's class code ((t0 * 7 + t1) * 7 + t2 on the axis) ascending.
 *                  TCMI_E_ARG, and NOTHING written (*len = 0), when the invariant fails (the two kernels disagree: no table), a
 *                  counter is negative, or counts are not ascending.  Sizing call, short buffer and *len as for tcmi_variants_text.
 *                  The header line (TCMI_CODONS_HEADER) is the caller's.
 * TCMI_CODONS_LDS: the codons whose first columns and [344] counters a workgroup stages in LDS (11 x 344 counters + 11 columns = 15 180
 * bytes); more codons are counted with atomics in memory; for tests.
 * Range errors are TCMI_E_ARG: n outside 1..16 384, a c0 outside [0, 2^29 - 2) or not above the one before; den outside 1..10^6, num
 * outside 0..den, min_alt_depth < 1, min_depth < 0; a frame with start < 0, end < start, a strand other than +1 / -1 or a phase outside
 * 0..2. */
typedef struct tcmi_codon_counts { int32_t j[7][7][7]; int32_t ins_inside, pos, reserved /* 0 */; } tcmi_codon_counts;   /* 346 int32 */
typedef struct tcmi_cds { int32_t start, end /* axis columns, half open */, strand /* +1 / -1 */, phase /* 0..2 */; } tcmi_cds;
#define TCMI_CODONS_LDS 11
#define TCMI_CODONS_HEADER "REGION\tFEATURE\tSTRAND\tCODON\tPOS\tREF_CODON\tREF_AA\tALT_CODON\tALT_AA\tEFFECT\tSUBS\tCOUNT\tSPAN\tFREQ\tPARTIAL\tOTHER\tINS_INSIDE\n"
int  tcmi_readset_codon_counts(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t n, const int64_t *c0 /* host */,
                               tcmi_codon_counts *records /* host, n */);
int  tcmi_codon_aa(int b0, int b1, int b2);
int  tcmi_codon_select(const tcmi_variant *records, int64_t n, const tcmi_cds *cds, int64_t n_cds, int64_t *c0, int64_t cap, int64_t *n_found);
int  tcmi_codons_text(const tcmi_codon_counts *counts, int64_t n, const tcmi_cds *cds, int64_t n_cds, const char *const *names,
                      const int32_t *matrix, int64_t L, int64_t ld, int64_t num, int64_t den, int32_t min_alt_depth, int32_t min_depth,
                      const char *region, int64_t pos_offset, const uint8_t *ref, int64_t n_ref, char *text, int64_t cap, int64_t *len);
/* counters of a context: "one_sync_taken" / "one_sync_declined" — files (or block ranges) the one-sync path delivered / handed to the
 * several-kernel path; "one_sync_retried" — files the one-sync path took a second time, its arrays sized for the worst case, because
 * the records outnumbered what the hint of their mean size allowed for; "one_sync_last_decline_flags" — why the last one was handed over (packer flags; 0: it was not a packer flag);
 * "decode_batched" — files (or ranges) whose blocks the device decoder took in batches ("decode_token_mb");
 * "split_sub_taken" — tcmi_split_step calls whose range went through sub-ranges ("split_sub"); "h2d_piped" — decodes whose
 * compressed bytes crossed PCIe in pieces on a copy stream ("h2d_pieces"); "compute_units" — the device's CUs, which times the
 * option "wg_per_cu" is the grid the packer and the tally kernel count on */
int  tcmi_ctx_stat(tcmi_ctx *ctx, const char *key, int64_t *value);

/* per-kernel device timing (hipEvents on the context's stream); kernel ids below */
enum { TCMI_K_TALLY = 0 /* bit-plane tally kernel */, TCMI_K_CALL = 1, TCMI_K_ZERO = 2,
       TCMI_K_TALLY_GENERAL = 3 /* CIGAR-walk tally kernel */,
       TCMI_K_PACK_CLASSIFY = 4 /* device packer: classify + scan */, TCMI_K_PACK = 5 /* device packer: scatter + pack */,
       TCMI_K_INFLATE = 6 /* device BGZF inflate */, TCMI_K_RECORDS = 7 /* device BAM record walk */,
       TCMI_K_CRC = 8 /* retired (always 0 since ABI 5): the blocks' CRC-32 is taken in bgzf_copy's flush, filed under TCMI_K_INFLATE_COPY */,
       TCMI_K_INFLATE_COPY = 9 /* device BGZF inflate, second kernel: tokens -> bytes (TCMI_K_INFLATE is the first: symbols -> tokens) */,
       TCMI_K_VARIANTS = 10 /* the variant table's three launches (count, scan, emit) as one bracket */,
       TCMI_K_INTERVALS = 11 /* the amplicon table's one launch */,
       TCMI_K_AMPLICON_READS = 12 /* tcmi_readset_amplicon_reads' one launch */,
       TCMI_K_STRAND_COUNTS = 13 /* tcmi_readset_strand_counts' one launch */,
       TCMI_K_LINK_COUNTS = 14 /* tcmi_readset_link_counts' one launch; tcmi_readset_codon_counts' one launch is filed in the same bracket
                                    (a slot of its own would move TCMI_K_NKERNELS, which is part of the ABI) */,
       TCMI_K_INDEL_EVENTS = 15 /* tcmi_readset_indel_events' launches (count, verify, gather) of one attempt as one bracket */,
       TCMI_K_EVIDENCE_COUNTS = 16 /* tcmi_readset_evidence_counts' one launch */,
       TCMI_K_MATE_JOIN = 17 /* the mate join's table reset and two launches (build, probe) as one bracket; under the duplicate rule
                                "join + dedup": its table reset and three launches (ends, build, mark) behind them, in the same bracket */,
       TCMI_K_NKERNELS = 18 };
int  tcmi_profile_enable(tcmi_ctx *ctx, int on);
int  tcmi_profile_reset(tcmi_ctx *ctx);
int  tcmi_profile_get(tcmi_ctx *ctx, int kernel, double *total_ms, int64_t *launches);

/* ---- stage A: pileup tally  (replaces indexing.BuildIndex, indexing.py:75-154;
 *      inner loop parse_query_sequences, indexing.py:102-132; semantics SURVEY §8-P) */

/* Reference length the tally matrix needs: max(ref_len, max end position of any
 * piled-up read) — the reference keeps columns beyond the FASTA length (indexing.py:137-151). */
int tcmi_reads_extent(const tcmi_reads *reads, int64_t ref_len, int64_t *out_L);

/* Reads -> HBM in the tally kernel's layout.  By default the BAM-native arrays are copied to the device as they are
 * and packed there by HIP kernels (CIGAR projection, token classification, coverage runs, 4-bit -> bit planes);
 * inputs the device packer does not take (see option "device_pack") are packed on the host.
 * A read that would be kept (FLAG 0x4 clear, pos >= 0, on a reference that piles up, a reference span > 0) and whose CIGAR consumes
 * 2^29 or more query bases (Yq: the lengths of its M, I, S, = and X ops) is no alignment: TCMI_E_FORMAT, with the read's index and
 * its Yq — on either packer, as the file routes refuse such a record.  Below that Yq may differ from l_qseq: a query index at or
 * beyond l_qseq reads as N, bases behind Yq are ignored.                                                                         */
int tcmi_readset_upload(tcmi_ctx *ctx, const tcmi_reads *reads, tcmi_readset **out);
/* Several BAMs in ONE read set (BASELINE configs[3], many independent BAMs): BAM b's positions are
 * shifted by b * stride (a multiple of 256, >= the extent of every BAM), so one tally launch and one
 * call launch process the whole batch over n * stride positions; BAM b's counts / records are the
 * slice [b * stride, b * stride + L) of every plane.                                             */
int tcmi_readset_upload_batch(tcmi_ctx *ctx, const tcmi_reads *const *reads, int32_t n, int64_t stride,
                              tcmi_readset **out);
int tcmi_readset_free(tcmi_ctx *ctx, tcmi_readset *rs);
int tcmi_readset_info(const tcmi_readset *rs, int64_t *n_reads, int64_t *n_piled,
                      int64_t *algorithmic_bytes, int64_t *device_bytes, int64_t *max_end);
/* how the reads were split: aligned set (bit-plane kernel; entries, chunks) vs general set (CIGAR-walk kernel) */
int tcmi_readset_sets(const tcmi_readset *rs, int64_t *aligned_reads, int64_t *aligned_chunks,
                      int64_t *general_reads);

/* *packed_on_device = 1 when the HIP packer (pack_device.hip) built the read set, 0 when the host packer did */
int tcmi_readset_origin(const tcmi_readset *rs, int32_t *packed_on_device);

/* Device-resident tally.  d_counts: device int32 [7][ld] (plane order TCMI_COV..TCMI_I,
 * plane p at d_counts + p*ld, ld >= L).  Zeroes the planes first when `zero` != 0,
 * otherwise accumulates (used when one BAM is split over several read sets / GPUs).
 * The matrix is the caller's: any device pointer aligned to 4 bytes (else TCMI_E_ARG) and any ld >= L, odd ones and ld == L
 * included — a torch tensor shaped (7, L) will do.  Exactly 7 * ld words are touched: `zero` clears all of them, padding
 * [L, ld) of every plane included; without `zero` the padding is left as it is; nothing in front of d_counts or behind
 * d_counts + 7 * ld is read or written.  Every (ld, alignment) gives the same counts; the bit-plane kernel adds two adjacent
 * positions with one 64-bit atomic when ld is even AND d_counts is aligned to 8 bytes, and position by position otherwise
 * (ld rounded up to 256 on a pointer from hipMalloc, as the library's own workspaces have it, takes the faster form).
 * The launch is queued on the context's stream: memory another stream wrote (torch's) must be complete before the call. */
int tcmi_tally_dev(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t L, int64_t ld,
                   void *d_counts, int zero);

/* Host-buffer convenience: upload, tally, download.  counts: host int32 [L][7] in the
 * reference's row layout (position p-1 at counts + 7*(p-1)).                      */
int tcmi_tally(tcmi_ctx *ctx, const tcmi_reads *reads, int64_t L, int32_t *counts);

/* planes [7][ld] on device  <->  rows [L][7] on host; d_counts and ld as for tcmi_tally_dev.  The upload writes all 7 * ld
 * words (padding [L, ld) as zero); both wait for the context's stream.                                                */
int tcmi_counts_download(tcmi_ctx *ctx, const void *d_counts, int64_t L, int64_t ld, int32_t *counts);
int tcmi_counts_upload(tcmi_ctx *ctx, const int32_t *counts, int64_t L, int64_t ld, void *d_counts);

/* ---- stage B (position-local part): base calling
 *      replaces Sequences.GetNucleotide/GetDistribution (Sequences.py:119-165),
 *      Ambig.IsAmbiguous (Ambig.py:179-228), Events.MinorityDel (Events.py:85-106),
 *      the candidate test of Events.ListInserts (Events.py:29-36) and the case rule
 *      (Sequences.py:229-235 and copies).  Outputs, one byte per position:
 *        plain[p]  character emitted when the primary nucleotide is not X
 *                  ('N' when cov < mincov)
 *        alt[p]    character of the secondary nucleotide (primary == X, Sequences.py:283-290)
 *        flags[p]  TCMI_F_* bits                                                      */
/* tcmi_call_dev: d_counts as for tcmi_tally_dev (4-byte aligned, any ld >= L); it is only read.  d_plain, d_alt, d_flags:
 * L bytes each at any byte address; bytes [L, ...) are not written.  d_events / d_event_counts (4-byte aligned; both or
 * neither, else TCMI_E_ARG): the kernel calls 256 positions per block, b = 0 .. ceil(L/256) - 1; d_event_counts[b] = the positions of
 * block b with flags & TCMI_EVENT_MASK and d_events[256 * b .. 256 * b + d_event_counts[b]) = those positions, ascending — so
 * d_events needs ceil(L/256) * 256 words (the rest of a block's 256 is left as it was) and d_event_counts ceil(L/256) words,
 * and the blocks' lists one after the other are all event positions in ascending order. */
int tcmi_call_dev(tcmi_ctx *ctx, const void *d_counts, int64_t L, int64_t ld,
                  int32_t mincov, int include_ambig,
                  void *d_plain, void *d_alt, void *d_flags,
                  void *d_events /* int32[ceil(L/256)*256], may be NULL */,
                  void *d_event_counts /* int32[ceil(L/256)], may be NULL */);

/* Host-buffer convenience (counts rows [L][7] in, bytes out). event_idx (capacity L)
 * receives the ascending 0-based indices of positions with flags & TCMI_EVENT_MASK. */
int tcmi_call(tcmi_ctx *ctx, const int32_t *counts, int64_t L, int32_t mincov, int include_ambig,
              uint8_t *plain, uint8_t *alt, uint8_t *flags,
              int32_t *event_idx, int64_t *n_events);

/* Whole resident step: zero + tally + call + copy records to pinned host memory.
 * Returns host pointers valid until the next step on this context.              */
int tcmi_step(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t L, int32_t mincov, int include_ambig,
              const uint8_t **plain, const uint8_t **alt, const uint8_t **flags,
              const int32_t **counts_planes /* host [7][ld] */, int64_t *ld);
/* The same in two halves, so that the host walk of one BAM can overlap the GPU work of the next
 * (two contexts, two streams): _begin only enqueues, _end waits for the context's stream.     */
int tcmi_step_begin(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t L, int32_t mincov,
                    int include_ambig, int want_counts);
int tcmi_step_end(tcmi_ctx *ctx, const uint8_t **plain, const uint8_t **alt, const uint8_t **flags,
                  const int32_t **counts_planes, int64_t *ld);

/* ---- stage B (sequential part, HOST): the consensus walk
 *      replaces the loop of Sequences.BuildConsensus (Sequences.py:179-322) with
 *      ORFs.in_orf / SolveTripletLength / CorrectStartPositions / CorrectGFF
 *      (ORFs.py:1-192) restated in O(L) over the call records.  No GPU needed.
 *
 *  orf_*      : one entry per GFF row (all rows take part in in_orf, ORFs.py:16-26;
 *               only strand '+' rows get their end corrected, ORFs.py:154)
 *  ins_pos    : 1-based positions of accepted inserts (ascending), ins_shift =
 *               int(size_str) of Events.py:75-80 (last digit only), ins_seq/ins_off =
 *               concatenated insert strings.
 *  out_cons   : capacity cons_cap bytes (L + total insert length is enough)
 *  new_start/new_end : corrected GFF coordinates per row
 *  err_pos    : for TCMI_E_KEYERROR the missing key (L+1)                          */
int tcmi_consensus_walk(const uint8_t *plain, const uint8_t *alt, const uint8_t *flags, int64_t L,
                        int32_t n_orf, const int64_t *orf_start, const int64_t *orf_end,
                        const uint8_t *orf_is_plus,
                        int32_t n_ins, const int64_t *ins_pos, const int32_t *ins_shift,
                        const char *ins_seq, const int64_t *ins_off,
                        int include_ins,
                        char *out_cons, int64_t cons_cap, int64_t *out_len,
                        int64_t *new_start, int64_t *new_end, int64_t *err_pos);

/* ---- insert tokens (Events.ExtractInserts, Events.py:47-82), HOST.
 * For each 1-based candidate position (ascending) scans the reads overlapping it under the
 * filters of pysam's default-argument region pileup (Events.py:66) and returns the modal
 * upper-cased token (Counter.most_common, first-seen tie-break, Events.py:71-74).
 *   tokens / token_off : concatenated modal tokens, token k = tokens[token_off[k] .. token_off[k+1])
 *                        (empty when the column has no token)
 *   n_tokens[k]        : tokens in column k after filtering (0: empty pileup -> position dropped)
 *   max_depth          : htslib's maxcnt (pysam's max_depth, default 8000): reads that share their start with the read
 *                        before them are dropped once the column holds this many; 0 = no cap
 *   ignore_overlaps    : pysam's default 1: of two overlapping mates only one keeps its base on the column (needs the
 *                        mate fields and names of tcmi_reads; reads without names are taken as unpaired).  A mate whose
 *                        token on the column is a deletion / ref-skip is tested on its next query base, as htslib does,
 *                        with the tweak evaluated on that base's reference position
 *   status_flags       : bit 0 = max_depth dropped reads (modelled, informational); bit 1 = a pair of overlapping mates
 *                        whose quality tweak could not be evaluated (not raised by the entry points of this library any
 *                        more; kept for callers that test it): the tokens would NOT be what pysam gives — refuse         */
#define TCMI_TOKENS_DEPTH_CAPPED     1
#define TCMI_TOKENS_OVERLAP_UNKNOWN  2
int tcmi_modal_tokens(const tcmi_reads *reads, int32_t n_pos, const int64_t *positions,
                      int32_t min_base_quality, uint32_t flag_filter, int ignore_orphans,
                      int64_t max_depth, int ignore_overlaps, char *tokens, int64_t tokens_cap, int64_t *token_off,
                      int64_t *n_tokens, int32_t *status_flags);
/* The same under a contig layout (tcmi_ctx_set_layout's arguments): positions are on the layout's axis, reference t's reads sit
 * at pos + shift[t]; mates on different references never count as overlapping. */
int tcmi_modal_tokens_layout(const tcmi_reads *reads, int32_t n_ref, const int64_t *shift, const int64_t *slot_len, int32_t n_pos,
                             const int64_t *positions, int32_t min_base_quality, uint32_t flag_filter, int ignore_orphans,
                             int64_t max_depth, int ignore_overlaps, char *tokens, int64_t tokens_cap, int64_t *token_off,
                             int64_t *n_tokens, int32_t *status_flags);

/* ---- many BAMs: native batch runner (BASELINE.json configs[3]: independent BAMs, no collective).
 * The calling thread queues step i+1 behind step i on one stream over `n_slots` workspaces while
 * `n_walkers` host threads turn finished call records into consensus sequences
 * (Events.ListInserts + Sequences.BuildConsensus(..., includeINS=True), the FASTA content).
 *   readsets[i]   reads of BAM i resident in HBM (same device)
 *   host_reads[i] the same reads on the host, needed only to resolve insert tokens
 *                 (Events.py:47-82); the array or an entry may be NULL: an item that then has
 *                 insert candidates fails with TCMI_E_UNSUPPORTED
 *   out_cons      n_items * stride bytes, consensus i at out_cons + i*stride, length out_len[i];
 *                 stride >= L + 1 + total inserted bases
 *   status[i]     TCMI_OK or the error of item i (e.g. TCMI_E_KEYERROR where the reference raises) */
typedef struct tcmi_pipeline tcmi_pipeline;
int tcmi_pipeline_create(int device, int n_slots, int n_walkers, tcmi_pipeline **out);
int tcmi_pipeline_destroy(tcmi_pipeline *p);
int tcmi_pipeline_set_orfs(tcmi_pipeline *p, int32_t n_orf, const int64_t *start, const int64_t *end,
                           const uint8_t *is_plus);
tcmi_ctx *tcmi_pipeline_ctx(tcmi_pipeline *p, int slot);   /* slot contexts (upload reads with slot 0's) */
int tcmi_pipeline_run(tcmi_pipeline *p, int64_t n_items, const tcmi_readset *const *readsets,
                      const tcmi_reads *const *host_reads, int64_t L, int32_t mincov, int include_ambig,
                      char *out_cons, int64_t stride, int64_t *out_len, int32_t *status);
/* The same over BATCHED read sets (tcmi_readset_upload_batch with `batch` BAMs at `pos_stride`):
 * item i yields consensus i*batch .. i*batch + batch - 1 (host_reads, out_len, status likewise).   */
int tcmi_pipeline_run_batched(tcmi_pipeline *p, int64_t n_items, const tcmi_readset *const *readsets,
                              int32_t batch, int64_t pos_stride, const tcmi_reads *const *host_reads,
                              int64_t L, int32_t mincov, int include_ambig, char *out_cons,
                              int64_t stride, int64_t *out_len, int32_t *status);

/* ---- BAM reader (pysam's role; SAM spec §4.2), HOST, zlib inflate -------- */
typedef struct tcmi_bam tcmi_bam;
int  tcmi_bam_load(const char *path, int n_threads, tcmi_bam **out);
int  tcmi_bam_free(tcmi_bam *bam);
/* fills `reads` with pointers owned by `bam`; n_ref / first reference name and length */
int  tcmi_bam_reads(const tcmi_bam *bam, tcmi_reads *reads);
int  tcmi_bam_header(const tcmi_bam *bam, int32_t *n_ref, const char **ref0_name, int64_t *ref0_len);
/* any out pointer may be NULL; sorted = 1 when mapped reads ascend by (tid, pos)               */
int  tcmi_bam_info(const tcmi_bam *bam, int64_t *n_reads, int32_t *sorted, int64_t *file_bytes,
                   int64_t *inflated_bytes, int64_t *n_blocks, int64_t *n_cigar, int64_t *n_qual);
const char *tcmi_bam_text(const tcmi_bam *bam);    /* SAM header text, owned by bam                */
/* name and length of reference i (0 <= i < n_ref) of the header; the name is owned by bam */
int  tcmi_bam_ref(const tcmi_bam *bam, int32_t i, const char **name, int64_t *len);
/* MAPQ of every record ([n_reads], owned by bam): struct tcmi_reads carries none */
int  tcmi_bam_mapq(const tcmi_bam *bam, const uint8_t **mapq);
/* The read filter of tcmi_ctx_set_read_filter for the host reader's output: removes the failing records from a loaded file in
 * place — every per-read array, the offsets, names, mate fields and qualities are compacted, `sorted` and the span behind
 * sorted_max_span are taken again over what is left — so that tcmi_bam_reads, tcmi_bam_info and everything behind them see the
 * passing records only.  *n_removed (may be NULL): records removed by this call. */
int  tcmi_bam_filter(tcmi_bam *bam, int32_t min_mapq, uint32_t require_flags, uint32_t exclude_flags, int64_t *n_removed);

/* ---- BAM decoded ON THE DEVICE (the default file path; the host reader above stays for files it does not take) ----
 * tcmi_bamfile_read: HOST — file bytes into pinned memory, BGZF block table, BAM header (only the leading blocks the
 * header occupies are inflated on the host).  tcmi_readset_from_bamfile: the compressed bytes cross PCIe, HIP kernels
 * inflate every BGZF block, follow the record chain (records may straddle blocks), and pack the reads for the tally (reads
 * spanning more than 512 positions are tallied where they lie in the stream) — the host never sees a decoded read.
 * Returns TCMI_E_UNSUPPORTED for files that need the host reader (a record chain that does not close, a mapped read on a
 * second reference, a CIGAR kept in a CG:B tag, positions beyond 2^29): fall back to tcmi_bam_load + tcmi_readset_upload. */
typedef struct tcmi_bamfile tcmi_bamfile;
int  tcmi_bamfile_read(const char *path, tcmi_bamfile **out);
int  tcmi_bamfile_free(tcmi_bamfile *f);
int  tcmi_bamfile_info(const tcmi_bamfile *f, int64_t *file_bytes, int64_t *inflated_bytes, int64_t *n_blocks, int32_t *n_ref,
                       const char **ref0_name, int64_t *ref0_len);
const char *tcmi_bamfile_text(const tcmi_bamfile *f);
int  tcmi_bamfile_ref(const tcmi_bamfile *f, int32_t i, const char **name, int64_t *len);   /* as tcmi_bam_ref */
const char *tcmi_bamfile_path(const tcmi_bamfile *f);
/* The file's compressed bytes into HBM, to stay until tcmi_bamfile_free: tcmi_readset_from_bamfile[_blocks] on that device then
 * start from device memory, no PCIe copy per call (a file a peer GPU, a NIC or a storage engine delivered into HBM looks like
 * this; bench.py's headline times this form: "inputs resident in HBM when the timed region starts"). */
int  tcmi_bamfile_to_device(tcmi_ctx *ctx, tcmi_bamfile *f);
int  tcmi_readset_from_bamfile(tcmi_ctx *ctx, const tcmi_bamfile *f, tcmi_readset **out, int64_t *n_reads);
/* ... of the alignment records that START in BGZF blocks [first_block, first_block + n_blocks) only (n_blocks < 0: to the end of the
 * file).  Ranks that share ONE BAM file (BASELINE configs[4]) each decode a contiguous range of its blocks and nothing else; the
 * count matrices of the ranges add up to the file's (what indexing.py:96-100 piles up in one pass). */
int  tcmi_readset_from_bamfile_blocks(tcmi_ctx *ctx, const tcmi_bamfile *f, int64_t first_block, int64_t n_blocks, tcmi_readset **out,
                                      int64_t *n_reads);
/* A range that starts in the middle of the file starts at the first PLAUSIBLE record its first block finds — nothing in front of
 * it vouches for that offset.  *first: where that record starts, *next: where the first record behind the range starts, both as
 * offsets into the whole file's inflated stream (-1: the range starts with the file or holds no record start / its chain was never
 * fixed).  Ranges that tile a file are all true record chains iff every range's *next equals the *first of the next range that has
 * one (by induction from the header: what any reader of a BAM file relies on, htslib's bam_read1 included); tcmi_split_step checks
 * exactly that along with its reduce, trueconsense_amd/distributed.py before its collective. */
int  tcmi_readset_range_anchors(const tcmi_readset *rs, int64_t *first, int64_t *next);
/* BAM file -> call records with ONE wait of the host: what indexing.BuildIndex (indexing.py:75-154) and the position-local part of
 * Sequences.BuildConsensus (Sequences.py:119-165 via Ambig.py / Events.py) come to for one file.  Decode, record index, record chain,
 * classification, packing, tally and call are queued back to back on the context's stream from capacities instead of counts read
 * back (the several calls above wait three + one times); one wait; then everything that was deferred is checked, and a file the
 * one-pass packer cannot vouch for (a damaged block, a record chain that does not close, reads it does not take, a file beyond the
 * capacities) is taken through tcmi_readset_from_bamfile + tcmi_step instead — same results, same errors.  The step covers
 * L = max(ref_len, the reads' extent, 1) positions (*L_out).  Results as tcmi_step's (valid until the context's next step);
 * *rs_out is the caller's (tcmi_readset_free), with the inflated stream resident for tcmi_readset_modal_tokens. */
int  tcmi_bamfile_step(tcmi_ctx *ctx, const tcmi_bamfile *f, int64_t ref_len, int32_t mincov, int include_ambig, tcmi_readset **rs_out,
                       int64_t *L_out, const uint8_t **plain, const uint8_t **alt, const uint8_t **flags,
                       const int32_t **counts_planes /* host [7][ld]; NULL: not wanted */, int64_t *ld);
/* Events.ExtractInserts for a read set the DEVICE decoded (tcmi_readset_from_bamfile): same arguments and results as
 * tcmi_modal_tokens, but the reads of every candidate column are examined by a HIP kernel where they lie (the inflated
 * stream stays resident on the context until its next upload) and only a few thousand 48-byte entries per column reach
 * the host (+ the bases of insertions too long for an entry's 64-bit token key, from a 4 MB text buffer).  TCMI_E_UNSUPPORTED when the
 * stream is gone (another upload happened on the context), the read set was not decoded on the device, or that text buffer
 * overflows: use tcmi_bam_load + tcmi_modal_tokens. */
int  tcmi_readset_modal_tokens(tcmi_ctx *ctx, const tcmi_readset *rs, int32_t n_pos, const int64_t *positions,
                               int32_t min_base_quality, uint32_t flag_filter, int ignore_orphans, int64_t max_depth,
                               int ignore_overlaps, char *tokens, int64_t tokens_cap, int64_t *token_off, int64_t *n_tokens,
                               int32_t *status_flags);
/* ---- ONE BAM file over several GPUs (BASELINE configs[4]; what the ranks jointly replace is the single-pass pile-up of
 * indexing.py:96-100 and, for the insert candidates, the region pile-ups of Events.py:47-82).
 * The library links no collective library: the one exchange of the path — a sum of the int32 count matrix to the rank that calls —
 * is a hook of the caller's (RCCL's ncclReduce on the given stream from C: include/tcmi_rccl.h, libtcmi_rccl.so; torch.distributed from Python:
 * trueconsense_amd/distributed.py).
 *   tcmi_split_step   this rank's part of one step, in C (rank 0 is the root): decode + pack + tally the alignment records that
 *                     start in BGZF blocks [first_block, first_block + n_blocks) into d_counts — device int32 [7][ld] +
 *                     TCMI_SPLIT_TAIL_WORDS(world) more int32 behind it: six words per rank, written by that rank into its own
 *                     slot and zero in everybody else's, so that the sum hands the root the table {first_block, n_blocks, first,
 *                     next (two words each)} of all ranges — a range in the middle of the file starts at the first offset its
 *                     first block finds plausible for a record, and only the range in front can vouch for it: the root checks
 *                     PAIRWISE that every range starts where the one in front ends and that the last one ends with the stream
 *                     (tcmi_readset_range_anchors; the same rule as distributed.check_range_anchors) —, and one word that counts
 *                     the ranks that failed: a rank that cannot do its share (a range that is refused, a workspace that cannot
 *                     be allocated) still takes part in the exchange, with zeros, so nobody waits for it forever;
 *                     reduce(user, d_counts, 7 * ld + TCMI_SPLIT_TAIL_WORDS(world), stream) — the hook must sum over the ranks,
 *                     at least to rank 0 —, and on rank 0 the call kernel: results as tcmi_step's.  *rs_out (any rank; NULL on
 *                     failure) keeps the rank's decoded stream resident for tcmi_readset_ins_entries.  Returns the rank's own
 *                     error, or on rank 0 TCMI_E_UNSUPPORTED when another rank failed or the ranges' record chains do not join.
 *   tcmi_readset_ins_entries   the entries of the candidate columns (TCMI_INS_ENTRY_BYTES each, opaque; per column in file order)
 *                     from this rank's records: what the ranks send to the root.  ent_off[n_pos + 1]; insertions of more than 12
 *                     bases leave their bases in long_text (long_used bytes).  TCMI_E_ARG with ent_off / long_used filled in when
 *                     a buffer is too small.
 *   tcmi_ins_entries_rebase    before concatenating the pieces of several ranks: piece k's long-insertion texts lie `long_base`
 *                     bytes into the concatenated text buffer
 *   tcmi_modal_from_entries    HOST: the vote of tcmi_readset_modal_tokens over per-column concatenations (rank order = file
 *                     order) of such pieces.  status_flags bit 1 (TCMI_TOKENS_OVERLAP_UNKNOWN): a pair of overlapping mates whose
 *                     other mate had to be looked at on another position — not possible across pieces: use the host sweep
 *                     (tcmi_bam_load + tcmi_modal_tokens) for that file. */
#define TCMI_INS_ENTRY_BYTES 48
typedef int (*tcmi_reduce_fn)(void *user, void *d_counts, int64_t n_int32, void *stream);
#define TCMI_SPLIT_TAIL_WORDS(world) (6 * (world) + 1)
int  tcmi_split_step(tcmi_ctx *ctx, const tcmi_bamfile *f, int64_t first_block, int64_t n_blocks, int64_t L, int64_t ld, void *d_counts,
                     int32_t mincov, int include_ambig, tcmi_reduce_fn reduce, void *user, int rank, int world, tcmi_readset **rs_out,
                     const uint8_t **plain, const uint8_t **alt, const uint8_t **flags);
int  tcmi_readset_ins_entries(tcmi_ctx *ctx, const tcmi_readset *rs, int32_t n_pos, const int64_t *positions, uint32_t flag_filter,
                              int ignore_orphans, void *entries, int64_t entries_cap, int64_t *ent_off, uint8_t *long_text,
                              int64_t long_cap, int64_t *long_used);
int  tcmi_ins_entries_rebase(void *entries, int64_t n_entries, int64_t long_base);
int  tcmi_modal_from_entries(int32_t n_pos, void *entries, const int64_t *ent_off, int32_t min_base_quality, int64_t max_depth,
                             int ignore_overlaps, const uint8_t *long_text, int64_t long_bytes, char *tokens, int64_t tokens_cap,
                             int64_t *token_off, int64_t *n_tokens, int32_t *status_flags);
/* for tests and tools: the device-inflated stream and the record offsets copied back to the host */
int  tcmi_bamfile_decode_to_host(tcmi_ctx *ctx, const tcmi_bamfile *f, uint8_t *stream, int64_t stream_cap,
                                 uint64_t *rec_off, int64_t rec_cap, int64_t *n_rec);

/* ---- BAM files -> FASTA text: native runner of the whole path for many inputs (TrueConsense.py:212-264 per file;
 * BASELINE configs[1] / [3]).  Three stages on their own threads, consecutive BAMs overlapping: read (host: file bytes,
 * block table, header), gpu (one thread per context: device decode + pack + tally + call; the host reader for files
 * the device decoder declines), walk (host: insert tokens if a candidate exists, consensus walk, FASTA text).
 *   out_text        n * stride bytes; text i (">name mincov=N\n<consensus>\n", Outputs.py:182-183) at out_text + i*stride
 *   stage_seconds   [4] busy seconds summed over the items: read, decode + pack, step, walk (may be NULL)
 *   decoded_on      [2] items decoded on the device / by the host reader (may be NULL)                                */
typedef struct tcmi_filerunner tcmi_filerunner;
int tcmi_filerunner_create(int device, int n_readers, int n_gpu, int n_walkers, int host_decode_threads, tcmi_filerunner **out);
int tcmi_filerunner_destroy(tcmi_filerunner *r);
int tcmi_filerunner_set_orfs(tcmi_filerunner *r, int32_t n_orf, const int64_t *start, const int64_t *end, const uint8_t *is_plus);
tcmi_ctx *tcmi_filerunner_ctx(tcmi_filerunner *r, int k);
int tcmi_filerunner_run(tcmi_filerunner *r, int64_t n, const char *const *paths, const char *const *names, int64_t ref_len,
                        int32_t mincov, int include_ambig, int device_decode, char *out_text, int64_t stride, int64_t *out_len,
                        int32_t *status, double *stage_seconds, int64_t *decoded_on);
/* ... of files read before (tcmi_bamfile_read; they stay the caller's): the read stage has nothing to do, and with
 * tcmi_bamfile_to_device the GPU stage starts from HBM.  Everything else as tcmi_filerunner_run. */
int tcmi_filerunner_run_resident(tcmi_filerunner *r, int64_t n, tcmi_bamfile *const *files, const char *const *names, int64_t ref_len,
                                 int32_t mincov, int include_ambig, char *out_text, int64_t stride, int64_t *out_len, int32_t *status,
                                 double *stage_seconds, int64_t *decoded_on);
/* The command line's other three outputs for many samples (Outputs.py:13-71, 104-180; Coverage.py:1-16), written by the runner's
 * walker threads.  tcmi_filerunner_set_outputs: the reference (id and sequence of its first FASTA record), the complete VCF header
 * text (Outputs.py:115-127), the GFF header text and per GFF row (the rows of tcmi_filerunner_set_orfs, same order) six strings:
 * source, type, score, strand, phase, attributes.  tcmi_filerunner_run_files: per sample the paths of its FASTA and (optionally;
 * an array or an entry may be NULL) VCF, corrected GFF and coverage TSV. */
int tcmi_filerunner_set_outputs(tcmi_filerunner *r, const char *ref_id, const char *ref_seq, const char *vcf_head, const char *gff_head,
                                int32_t n_rows, const char *const *row_cols);
int tcmi_filerunner_run_files(tcmi_filerunner *r, int64_t n, const char *const *paths, const char *const *names, const char *const *fasta,
                              const char *const *vcf, const char *const *gff, const char *const *doc, int64_t ref_len, int32_t mincov,
                              int include_ambig, int device_decode, int32_t *status, double *stage_seconds, int64_t *decoded_on);
/* ... and per sample (an array or an entry may be NULL) its variant table.  tcmi_ctx_set_variants on every context of the runner first
 * (tcmi_filerunner_ctx; the same setting on all, its reference the one of tcmi_filerunner_set_outputs, which also gives the rows
 * their REGION): the GPU stage copies the step's records next to the call records, the walker writes header + tcmi_variants_text.  A
 * sample the host reader took gets its table too.  n_variants (may be NULL): per sample the records written. */
int tcmi_filerunner_run_files_table(tcmi_filerunner *r, int64_t n, const char *const *paths, const char *const *names, const char *const *fasta,
                                    const char *const *vcf, const char *const *gff, const char *const *doc, const char *const *table, int64_t ref_len,
                                    int32_t mincov, int include_ambig, int device_decode, int32_t *status, double *stage_seconds, int64_t *decoded_on,
                                    int64_t *n_variants);
/* ... and the amplicon table's records.  tcmi_ctx_set_intervals on every context of the runner first (the same n_intervals intervals
 * on all): the GPU stage copies the step's records next to the call records, and they land in stats[i * n_intervals ...) for sample
 * i (zeroes for a sample that failed).  A sample the host reader took gets its records through the same kernel.  The caller writes
 * the table (tcmi_amplicons_text).  n_intervals = 0 with stats = NULL: tcmi_filerunner_run_files_table. */
int tcmi_filerunner_run_files_stats(tcmi_filerunner *r, int64_t n, const char *const *paths, const char *const *names, const char *const *fasta,
                                    const char *const *vcf, const char *const *gff, const char *const *doc, const char *const *table, int64_t ref_len,
                                    int32_t mincov, int include_ambig, int device_decode, int32_t *status, double *stage_seconds, int64_t *decoded_on,
                                    int64_t *n_variants, int64_t n_intervals, tcmi_interval_stat *stats);

#ifdef __cplusplus
}
#endif
#endif /* TCMI_H */
