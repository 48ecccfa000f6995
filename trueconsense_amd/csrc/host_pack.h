// host_pack.h — HOST: the packer behind tcmi_readset_upload for everything the device packer declines (long reads, positions beyond
// 2^29, unsorted input, batches, project_reads = 0).  It selects the reads that pile up, splits them into the ALIGNED and
// the GENERAL set and packs both as the tally kernels take them (layout: readset_layout.h) — into host memory.  Stages that take plain
// inputs and leave plain memory: no HIP header, no context, so a program of its own runs them under a sanitizer
// (tests/host_pack_main.cpp, tests/test_host_pack.py).  readset.cpp calls them and copies the result into HBM.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/tcmi.h"
#include "readset_layout.h"

struct tcmi_host_pack_opts {
    int host_threads = 8;       // threads that classify and pack
    bool use_fast = true;       // tally_variant != 1; false: every read into the general set
    bool project_reads = true;  // reads with indels / skips go to the aligned set, projected onto the reference
    int chunk_stages = 0;       // stages per chunk, 0 = up to TCMI_F_MAXSTAGE
    int stage_cap = 0;          // upper bound on the reads per stage (0 = fill the LDS buffer)
    bool balance = true;        // size the chunks so that their number is a multiple of `slots` (chunk_stages = 0 only)
    int64_t slots = 1024;       // resident workgroups of the tally kernel: n_cu * wg_per_cu
};

// one entry of the aligned set: read i of BAM r (positions shifted by off); for a projected read the piece
// [seg, seg + len) of its reference span (long reads are cut into pieces of <= TCMI_F_SEG positions)
struct tcmi_host_sel { const tcmi_reads *r; int64_t i, off, y0, len, seg; bool projected; };
struct tcmi_host_gsel { const tcmi_reads *r; int64_t i, off; };
struct tcmi_host_slice {            // what one classification thread found in its slice of a BAM
    std::vector<tcmi_host_sel> fsel; std::vector<tcmi_host_gsel> gsel;
    std::vector<int64_t> ref_ext;   // under a contig layout: the kept reads' max end per reference, in its own coordinates
    int64_t n_dropped = 0;          // ... and the mapped reads on references without a slot
    int64_t g_cig = 0, g_seqw = 0, alg = 0, max_end = 0; bool any_cut = false;
    int err = TCMI_OK; char msg[160] = {0};
};

// The packed read set in host memory, and the lists it was made from.  A context keeps one between uploads: an upload of 1 M reads walks
// through ~200 MB of these buffers, and a third of its time used to go into page faults of fresh allocations and their release.
struct tcmi_host_packed {
    // select
    std::vector<tcmi_host_sel> fsel;        // aligned set (len > 0), in the order it is packed
    std::vector<tcmi_host_gsel> gsel;       // general set
    std::vector<tcmi_host_slice> slices;
    int64_t n_reads_in = 0, alg = 0, max_end = 0, n_dropped = 0;
    std::vector<int64_t> ref_ext;
    // aligned set: plan_chunks (chunks, f_words, room for f_seq), pack_aligned (the rest)
    std::vector<tcmi_fast_chunk> chunks;
    std::vector<uint32_t> f_lenoff;         // [fsel.size()] the packed header words
    std::vector<uint32_t> f_event;          // position | TCMI_F_EV_* : tokens that are not plain A/C/G/T bases
    std::vector<uint32_t> f_covrun;         // coverage runs (tcmi_fast_chunk::run0 / n_runs)
    uint32_t *f_seq = nullptr;              // [f_words] not zero-filled: every packing thread clears its own chunks
    size_t f_seq_cap = 0, f_words = 0;
    // general set: pack_general
    int64_t g_cig = 0, g_seqw = 0, n_rounds = 0;
    std::vector<int32_t> g_pos, g_lseq;     // [gsel.size()]
    std::vector<uint32_t> g_meta;           // [gsel.size()] flag << 16 | n_cigar
    std::vector<uint32_t> g_cigar, g_seq;   // [g_cig], [g_seqw] 8 bases per word, raw BAM codes in linear nibble order (+ 1 word of room)
    std::vector<int64_t> g_round_cig, g_round_seq;   // [n_rounds + 1]
    char msg[200] = {0};                    // the text of a refusal

    int64_t n_piled() const { return (int64_t)(fsel.size() + gsel.size()); }
    size_t bytes() const;                   // what the buffers hold on to
    tcmi_host_packed() = default;
    tcmi_host_packed(const tcmi_host_packed &) = delete;
    tcmi_host_packed &operator=(const tcmi_host_packed &) = delete;
    ~tcmi_host_packed() { delete[] f_seq; }
};

// The argument check of one tcmi_reads: TCMI_OK, or TCMI_E_ARG and its text.
int tcmi_host_check_reads(const tcmi_reads *r, const char **msg);
// Does read i pile up (mapped, on a reference with a slot, pos >= 0, reference span > 0)?  *span: that span.
bool tcmi_host_piles_up(const tcmi_reads *r, int64_t i, int64_t *span, const tcmi_layout &lay);

// The stages, in this order.  One or several BAMs become one read set; BAM b's positions are shifted by b * stride, so that the kernels
// see one long coordinate axis and a single launch tallies the whole batch.  _select and _pack_aligned return TCMI_OK or a refusal's
// code with its text in out->msg; nothing of `out` may be used after one.
int tcmi_host_select(const tcmi_reads *const *batch, int32_t n_batch, int64_t stride, const tcmi_layout &lay, const tcmi_host_pack_opts &opt,
                     tcmi_host_packed *out);
void tcmi_host_plan_chunks(const tcmi_host_pack_opts &opt, tcmi_host_packed *out);
int tcmi_host_pack_aligned(const tcmi_host_pack_opts &opt, tcmi_host_packed *out);
void tcmi_host_pack_general(tcmi_host_packed *out);
