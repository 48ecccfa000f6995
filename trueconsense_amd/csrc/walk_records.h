// walk_records.h — HOST: call records of one BAM -> consensus, and the pieces both native runners (array_pipeline.cpp: read sets
// resident in HBM; pipeline.cpp: BAM files) put around it: the ORF rows, the insert-candidate scan, the token buffer that grows, the
// host reader's reads of a file under a read filter.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "outputs_text.h"
#include "tcmi_internal.h"

// the ORF rows the walk corrects (tcmi_pipeline_set_orfs, tcmi_filerunner_set_orfs)
struct tcmi_orfs {
    std::vector<int64_t> start, end;
    std::vector<uint8_t> plus;
    size_t size() const { return start.size(); }
};
// -> TCMI_OK, or TCMI_E_ARG (o: the runner's rows, null when the runner is)
int tcmi_orfs_assign(tcmi_orfs *o, int32_t n_orf, const int64_t *start, const int64_t *end, const uint8_t *is_plus);

// the 1-based positions whose call record carries the insert-candidate bit (Events.py:29-36 evaluated by the call kernel)
void tcmi_insert_candidates(const uint8_t *flags, int64_t L, std::vector<int64_t> &cand);

// modal tokens of the candidate columns: candidate k's token at toks[off[k] .. off[k + 1]), cnt[k] reads voted.  valid: resolved (the
// file runner: on the device, by tcmi_readset_modal_tokens, while the decoded stream was still resident)
struct tcmi_tokens {
    std::vector<int64_t> off, cnt;
    std::vector<char> toks;
    bool valid = false;
};

// A token call into buffers sized for n_cand columns: `call(text, capacity)` is tried with 64 KiB, and while it finds that too small
// ("token buffer too small" in tcmi_last_error(ctx)) with 16 times as much, up to 1 GiB.  -> the last call's code
template <class Call>
int tcmi_tokens_grow(tcmi_ctx *ctx, size_t n_cand, tcmi_tokens &t, Call call)
{
    t.off.assign(n_cand + 1, 0);
    t.cnt.assign(n_cand, 0);
    t.toks.assign(1 << 16, 0);
    for (;;) {
        const int rc = call(t.toks.data(), (int64_t)t.toks.size());
        if (rc != TCMI_E_ARG || t.toks.size() >= ((size_t)1 << 30) || !std::strstr(tcmi_last_error(ctx), "token buffer too small")) return rc;
        t.toks.resize(t.toks.size() * 16);
    }
}

// The reads of a BAM file as the host reader decodes them, those that pass a read filter: flat arrays that live as long as this does.
struct tcmi_host_reads {
    tcmi_bam *bam = nullptr;
    tcmi_reads reads;
    tcmi_host_reads() = default;
    tcmi_host_reads(const tcmi_host_reads &) = delete;
    tcmi_host_reads &operator=(const tcmi_host_reads &) = delete;
    ~tcmi_host_reads() { if (bam) tcmi_bam_free(bam); }
    int load(const char *path, int threads, const tcmi_read_filter &flt);       // a failure's words: tcmi_last_error(nullptr)
};

// what the other writers (VCF, corrected GFF) take from the walk besides the consensus
struct tcmi_walk_extra {
    std::vector<int64_t> new_start, new_end;        // corrected GFF coordinates per row (of the walk WITH inserts: Outputs.py:95-98)
    tcmi_inserts ins;                               // the accepted inserts
    std::string cons_noinsert;                      // the second walk (includeINS = False)
};

// Call records -> consensus: the candidates' modal tokens (`pre` when it is valid, else one host sweep over `reads`) -> accepted
// inserts (Events.py:5-82), then the sequential walk (consensus_walk.cpp).  out: `cap` bytes, *out_len of them written.
int tcmi_walk_records(const uint8_t *plain, const uint8_t *alt, const uint8_t *flags, int64_t L, const std::vector<int64_t> &cand,
                      const tcmi_reads *reads, const tcmi_tokens *pre, const tcmi_orfs &orfs, char *out, int64_t cap, int64_t *out_len,
                      long long item, tcmi_walk_extra *extra = nullptr);
