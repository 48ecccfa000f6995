// ins_entries.hip — DEVICE: the reads on the insert-candidate columns of a device-decoded read set, for the token vote of
// Events.ExtractInserts (insert_tokens.cpp), read from the inflated BAM stream the packer left in the context's arena:
//   ins_sorted_kernel / ins_ranges_kernel   do the kept reads ascend by position; per column those that can reach it (binary searches)
//   ins_entries_kernel                      one lane per (column, read): the read's token on the column as a 48-byte tcmi_dev_entry
//   ins_probe_kernel                        the other mate of an overlapping pair on one reference position (rare)
#include <algorithm>
#include <cstring>
#include <vector>

#include "stream_count.h"

namespace {

constexpr int PB = 256;                          // lanes per workgroup of ins_entries_kernel

// ---- insert-candidate columns: every read of a column as an entry for the host's token vote (Events.py:47-82) -----------------
// One lane per (candidate column, read that starts within TCMI_D_MAXLEN positions before it).  The lane applies the samtools
// stepper's filters, finds the CIGAR op that covers the column and builds what pysam's get_query_sequences(add_indels=True)
// would print for it as a packed 64-bit key (insert_tokens.cpp), with the quality pysam tests, the base, the mate fields and a
// hash of the read name; the few thousand entries per column go to the host, which applies the rules that depend on the other
// reads of the column (max_depth admission, overlapping mates, the vote).  The decoded reads themselves never leave the device.
struct InsArgs {
    PackSrc src;
    const uint32_t *c_idx;
    const int32_t *cols;            // [n_cand] 0-based columns
    const int64_t *lo;              // [n_cand] first compacted read index to look at
    const int64_t *off;             // [n_cand + 1] pair offsets: candidate k owns pairs [off[k], off[k+1])
    tcmi_dev_entry *out;            // [off[n_cand]]: pair p's entry at out[p] — in file order; key 0: the read gives none on that column
    int32_t n_cand;
    uint32_t flag_filter;
    int32_t ignore_orphans;
    // insertions of more than 12 bases do not fit the entry's key: their bases (one 4-bit code per byte) go here, the key says where
    uint8_t *long_text;
    uint32_t *long_cursor;          // bytes taken
    uint32_t long_cap;
};


__global__ __launch_bounds__(PB) void ins_entries_kernel(InsArgs a)
{
    const int64_t p = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (p >= a.off[a.n_cand]) return;
    a.out[p].key = 0;                                           // (overwritten below if the read has a token on the column)
    int k = 0;
    while (k + 1 < a.n_cand && p >= a.off[k + 1]) ++k;          // (a handful of candidates)
    const int64_t j = a.lo[k] + (p - a.off[k]);
    const int32_t col = a.cols[k];
    const uint32_t i = a.c_idx[j];
    const ReadView v = view(a.src, i);
    if ((v.flag & a.flag_filter) || !passes(a.src.flt, v)) return;   // (the read set's own filter: no failing record is among the kept reads; tested all the same)
    if (a.ignore_orphans && (v.flag & 0x1u) && !(v.flag & 0x2u)) return;
    // the op that covers the column
    int64_t x = v.pos, y = 0;
    int64_t span = 0;
    for (uint32_t c = 0; c < v.n_cigar; ++c) {
        const uint32_t w = ld_u32(v.cigar + 4 * (size_t)c);
        if (consumes_ref(w & 0xFu)) span += w >> 4;
    }
    if (col < v.pos || col >= v.pos + span) return;
    for (uint32_t c = 0; c < v.n_cigar; ++c) {
        const uint32_t w = ld_u32(v.cigar + 4 * (size_t)c), op = w & 0xFu;
        const int64_t len = w >> 4;
        if (consumes_ref(op)) {
            if (col < x + len) {
                const bool rev = v.flag & 0x10u;
                const int32_t lq = v.l_seq;
                const int64_t qpos = is_match(op) ? y + (col - x) : y;
                const uint8_t *qual = v.seq + ((size_t)lq + 1) / 2;
                tcmi_dev_entry e;
                e.qual = (uint8_t)(qpos < lq ? byte_at(qual + qpos) : 0u);
                const uint32_t nib = qpos < lq ? nib_at(v.seq, (int32_t)qpos) : 15u;
                e.bits = (uint8_t)(nib | (is_match(op) && qpos < lq ? 0x10u : 0u));   // 0x10: a base on the column (within SEQ)
                // first character: "=ACMGRSVTWYHKDBN", '=' prints as '.' / ',' by strand; '*' for a deleted base, '>' '<' for a skip
                const char *NT = "=ACMGRSVTWYHKDBN";
                char first = is_match(op) ? NT[nib] : (op == 3 ? (rev ? '<' : '>') : '*');
                if (first == '=') first = rev ? ',' : '.';
                // p->indel of htslib's resolve_cigar2 on the last reference base of the op
                int64_t indel = 0;
                if (col == x + len - 1 && c + 1 < v.n_cigar) {
                    const uint32_t w2 = ld_u32(v.cigar + 4 * (size_t)(c + 1)), op2 = w2 & 0xFu;
                    if (op2 == 2 && op != 2) {
                        indel = -(int64_t)(w2 >> 4);
                        for (uint32_t t = c + 2; t < v.n_cigar; ++t) { const uint32_t wt = ld_u32(v.cigar + 4 * (size_t)t); if ((wt & 0xFu) != 2) break; indel -= wt >> 4; }
                    } else if (op2 == 1) {
                        indel = w2 >> 4;
                        for (uint32_t t = c + 2; t < v.n_cigar; ++t) {
                            const uint32_t wt = ld_u32(v.cigar + 4 * (size_t)t), o = wt & 0xFu;
                            if (o == 1) indel += wt >> 4; else if (o != 6) break;
                        }
                    } else if (op2 == 6 && c + 2 < v.n_cigar) {
                        for (uint32_t t = c + 2; t < v.n_cigar; ++t) {
                            const uint32_t wt = ld_u32(v.cigar + 4 * (size_t)t), o = wt & 0xFu;
                            if (o == 1) indel += wt >> 4; else if (consumes_ref(o)) break;
                        }
                    }
                }
                uint64_t key = (1ull << 63) | (uint8_t)first;
                if (indel > 12) {
                    // does not fit the key: bits 8-39 where its bases start in the text buffer, bits 40-62 how many (bits |= 0x40;
                    // 0x80: the buffer is full or the insertion absurdly long — the host sweep takes the BAM)
                    e.bits |= 0x40;
                    const uint32_t slot = indel < (1 << 23) ? atomicAdd(a.long_cursor, (uint32_t)indel) : a.long_cap;
                    if (indel < (1 << 23) && (uint64_t)slot + (uint64_t)indel <= a.long_cap) {
                        for (int64_t t = 1; t <= indel; ++t) {
                            const int64_t q2 = qpos + t;
                            a.long_text[slot + (uint32_t)(t - 1)] = (uint8_t)(q2 >= lq ? 15u : nib_at(v.seq, (int32_t)q2));
                        }
                        key |= ((uint64_t)slot << 8) | ((uint64_t)indel << 40);
                    } else e.bits |= 0x80;
                } else if (indel > 0) {
                    key |= (1ull << 8) | ((uint64_t)indel << 10);
                    bool any_eq = false;
                    for (int64_t t = 1; t <= indel; ++t) {
                        const int64_t q2 = qpos + t;
                        const uint32_t nb = q2 >= lq ? 15u : nib_at(v.seq, (int32_t)q2);
                        any_eq |= nb == 0;
                        key |= (uint64_t)nb << (15 + 4 * (t - 1));
                    }
                    if (any_eq && rev) key |= 1ull << 14;
                } else if (indel < 0) {
                    key |= (2ull << 8) | ((uint64_t)(-indel) << 10);
                }
                e.key = key;
                // mate fields and the name (behind block_size: refID 0, pos 4, l_read_name 8, ..., next_refID 20, next_pos 24, tlen 28, name 32)
                const uint8_t *r = a.src.stream + a.src.rec_off[i] + 4;
                const int32_t mtid = (int32_t)ld_u32(r + 20);
                e.mpos = (int32_t)ld_u32(r + 24);
                e.isize = (int32_t)ld_u32(r + 28);
                if (mtid >= 0 && mtid != v.tid) e.bits |= 0x20;
                const uint32_t l_name = ld_u32(r + 8) & 0xFFu;
                uint64_t h = 1469598103934665603ull;
                for (uint32_t t = 0; t + 1 < l_name; ++t) { h ^= byte_at(r + 32 + t); h *= 1099511628211ull; }
                e.name_hash = h ? h : 1;
                e.j = (uint32_t)j; e.pos = v.pos; e.end = (int32_t)(v.pos + span); e.l_qseq = lq; e.flag = (uint16_t)v.flag;
                // a deletion / ref-skip token is tested on the quality of the next query base: a matched one? on which reference position
                // (where the overlap tweak of a pair of mates can reach it: insert_tokens.cpp)
                e.qref = -1;
                if (!is_match(op) && qpos < lq) {
                    int64_t xr = x + len;
                    for (uint32_t t = c + 1; t < v.n_cigar; ++t) {
                        const uint32_t wt = ld_u32(v.cigar + 4 * (size_t)t), o = wt & 0xFu;
                        if (is_match(o)) { if ((wt >> 4) > 0 && xr <= INT32_MAX) e.qref = (int32_t)xr; break; }
                        if ((o == 1 || o == 4) && (wt >> 4) > 0) break;
                        if (consumes_ref(o)) xr += wt >> 4;
                    }
                }
                a.out[p] = e;
                return;
            }
            x += len;
        }
        if (consumes_query(op)) y += len;
    }
}

// do the kept reads ascend by position?  (the packer also takes input with a few reads out of place; the range search below does not)
__global__ __launch_bounds__(256) void ins_sorted_kernel(const int32_t *c_pos, int64_t nf, uint32_t *unsorted)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
    if (i < nf && c_pos[i] < c_pos[i - 1]) atomicOr(unsorted, 1u);
}

// which of the kept reads (ascending positions) can cover column cols[k]: those that start in (col - max_len, col]
__global__ __launch_bounds__(64) void ins_ranges_kernel(const int32_t *c_pos, int64_t nf, const int32_t *cols, int32_t n_cand, int32_t max_len,
                                                        int64_t *lo, int64_t *hi)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n_cand) return;
    const int64_t first = (int64_t)cols[k] - max_len + 1, last = cols[k];
    int64_t a = 0, b = nf;
    while (a < b) { const int64_t m = (a + b) >> 1; if ((int64_t)c_pos[m] < first) a = m + 1; else b = m; }
    lo[k] = a;
    b = nf;
    while (a < b) { const int64_t m = (a + b) >> 1; if ((int64_t)c_pos[m] <= last) a = m + 1; else b = m; }
    hi[k] = a;
}

// does read j (compacted index) have a matched base on reference position `ref`?  -> matched | base << 8 | quality << 16
struct ProbeArgs {
    PackSrc src;
    const uint32_t *c_idx;
    const int64_t *idx;
    const int32_t *ref;
    uint32_t *out;
    int32_t n;
};

__global__ __launch_bounds__(64) void ins_probe_kernel(ProbeArgs a)
{
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= a.n) return;
    uint32_t res = 15u << 8;
    const ReadView v = view(a.src, a.c_idx[a.idx[t]]);
    const int64_t ref = a.ref[t];
    int64_t x = v.pos, y = 0;
    for (uint32_t c = 0; c < v.n_cigar; ++c) {
        const uint32_t w = ld_u32(v.cigar + 4 * (size_t)c), op = w & 0xFu;
        const int64_t len = w >> 4;
        if (consumes_ref(op)) {
            if (ref < x + len) {
                if (is_match(op) && ref >= x) {
                    const int64_t q = y + (ref - x);
                    if (q < v.l_seq) {
                        const uint8_t *qual = v.seq + ((size_t)v.l_seq + 1) / 2;
                        res = 1u | (nib_at(v.seq, (int32_t)q) << 8) | (byte_at(qual + q) << 16);
                    }
                }
                break;
            }
            x += len;
        }
        if (consumes_query(op)) y += len;
    }
    a.out[t] = res;
}

} // namespace

// the device half of Events.ExtractInserts for a device-decoded read set: every read that can reach a candidate column as a 48-byte
// entry (ins_entries_kernel), in file order per column, in the context's pinned scratch (valid until the context's next call)
static int collect_ins_entries(tcmi_ctx *ctx, const tcmi_readset *rs, int32_t n_pos, const int64_t *positions, uint32_t flag_filter, int ignore_orphans,
                               std::vector<int64_t> &off, std::vector<int32_t> &cnt, const tcmi_dev_entry **ents_out, std::vector<uint8_t> &long_text)
{
    if (!ctx || !rs || n_pos < 0 || (n_pos > 0 && !positions)) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");

    if (rs->s_reads > 0)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "long reads lie outside the packed set: their tokens are not looked at here (host sweep)");
    if (rs->n_lay > 0)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "the read set was uploaded under a contig layout: host sweep (tcmi_modal_tokens_layout)");
    if (tcmi_stream_gone(ctx, rs))
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "the read set's decoded stream is no longer (or never was) resident on this context: host sweep");
    for (int32_t k = 1; k < n_pos; ++k)
        if (positions[k] <= positions[k - 1]) return tcmi_fail(ctx, TCMI_E_ARG, "positions must ascend");
    off.assign((size_t)n_pos + 1, 0); cnt.assign((size_t)n_pos, 0); *ents_out = nullptr; long_text.clear();
    if (n_pos == 0) return TCMI_OK;
    TCMI_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t nf = rs->f_reads;
    // The kept reads ascend by position (the device packer takes nothing else): which of them can reach each column is a
    // binary search on the device; what comes back is two numbers per column.  Scratch (device + pinned host) belongs to the
    // context and only grows: hipMalloc / hipFree per file cost more than the kernels (hipFree waits for the whole device).
    auto scratch = [&](size_t dev_bytes, size_t host_bytes) -> int {
        const size_t dev_slack = dev_bytes / 4 + (1 << 20), host_slack = host_bytes / 4 + (1 << 20);
        if (!tcmi_grow_dev(ctx, ctx->tok_dev, ctx->tok_dev_cap, dev_bytes, dev_slack))
            return tcmi_fail(ctx, TCMI_E_NOMEM, "insert-token scratch (%zu bytes)", dev_bytes + dev_slack);
        if (!tcmi_grow_pinned(ctx, ctx->tok_host, ctx->tok_host_cap, host_bytes, host_slack))
            return tcmi_fail(ctx, TCMI_E_NOMEM, "insert-token host scratch (%zu bytes)", host_bytes + host_slack);
        return TCMI_OK;
    };
    std::vector<int32_t> cols((size_t)n_pos);
    for (int32_t k = 0; k < n_pos; ++k) cols[(size_t)k] = (int32_t)(positions[k] - 1);
    const size_t b_cols = tcmi_align256((size_t)n_pos * 4), b_lo = tcmi_align256((size_t)n_pos * 8), b_off = tcmi_align256(((size_t)n_pos + 1) * 8);
    {
        const int rc = scratch(b_cols + 2 * b_lo + b_off, 2 * b_lo);
        if (rc) return rc;
    }
    int32_t *d_cols = (int32_t *)ctx->tok_dev;
    int64_t *d_lo = (int64_t *)(ctx->tok_dev + b_cols), *d_hi = (int64_t *)(ctx->tok_dev + b_cols + b_lo), *d_off = (int64_t *)(ctx->tok_dev + b_cols + 2 * b_lo);
    int64_t *h_lo = (int64_t *)ctx->tok_host, *h_hi = (int64_t *)(ctx->tok_host + b_lo);
    const int32_t max_len = (int32_t)std::min<int64_t>(std::max<int64_t>(rs->max_len, 1), TCMI_D_MAXLEN);
    TCMI_HIP(ctx, hipMemcpyAsync(d_cols, cols.data(), (size_t)n_pos * 4, hipMemcpyHostToDevice, ctx->stream));
    (void)hipGetLastError();
    uint32_t *d_unsorted = (uint32_t *)d_off;                   // (the offsets go there later)
    TCMI_HIP(ctx, hipMemsetAsync(d_unsorted, 0, 4, ctx->stream));
    if (nf > 1) hipLaunchKernelGGL(ins_sorted_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, ctx->stream, rs->d_cpos, nf, d_unsorted);
    hipLaunchKernelGGL(ins_ranges_kernel, dim3((unsigned)((n_pos + 63) / 64)), dim3(64), 0, ctx->stream, rs->d_cpos, nf, d_cols, n_pos, max_len, d_lo, d_hi);
    TCMI_HIP(ctx, hipGetLastError());
    TCMI_HIP(ctx, hipMemcpyAsync(h_lo, d_lo, (size_t)n_pos * 8, hipMemcpyDeviceToHost, ctx->stream));
    TCMI_HIP(ctx, hipMemcpyAsync(h_hi, d_hi, (size_t)n_pos * 8, hipMemcpyDeviceToHost, ctx->stream));
    uint32_t unsorted = 0;
    TCMI_HIP(ctx, hipMemcpyAsync(&unsorted, d_unsorted, 4, hipMemcpyDeviceToHost, ctx->stream));
    TCMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (unsorted) return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "reads are not sorted by position: host sweep");
    const std::vector<int64_t> lo_v(h_lo, h_lo + n_pos), hi_v(h_hi, h_hi + n_pos);   // (the scratch below may move)
    for (int32_t k = 0; k < n_pos; ++k) off[(size_t)k + 1] = off[(size_t)k] + std::max<int64_t>(0, hi_v[(size_t)k] - lo_v[(size_t)k]);
    const int64_t total = off[(size_t)n_pos];
    for (int32_t k = 0; k < n_pos; ++k) cnt[(size_t)k] = (int32_t)(off[(size_t)k + 1] - off[(size_t)k]);
    const tcmi_dev_entry *ents = nullptr;
    constexpr size_t LONG_TEXT_CAP = 4u << 20;                  // bases of insertions longer than 12 on the candidate columns of one call
    if (total > 0) {
        const size_t b_head = b_cols + 2 * b_lo + b_off, b_ent = tcmi_align256((size_t)total * sizeof(tcmi_dev_entry));
        const int rc = scratch(b_head + b_ent + 256 + LONG_TEXT_CAP, std::max(2 * b_lo, b_ent));
        if (rc) return rc;
        // (a regrown device buffer lost the columns and ranges: they are sent again — all tiny)
        d_cols = (int32_t *)ctx->tok_dev;
        d_lo = (int64_t *)(ctx->tok_dev + b_cols); d_off = (int64_t *)(ctx->tok_dev + b_cols + 2 * b_lo);
        InsArgs a;
        a.src = stream_src(rs);
        a.c_idx = rs->d_cidx;
        a.out = (tcmi_dev_entry *)(ctx->tok_dev + b_head);
        a.cols = d_cols; a.lo = d_lo; a.off = d_off;
        a.n_cand = n_pos; a.flag_filter = flag_filter; a.ignore_orphans = ignore_orphans;
        a.long_cursor = (uint32_t *)(ctx->tok_dev + b_head + b_ent); a.long_text = (uint8_t *)(ctx->tok_dev + b_head + b_ent + 256); a.long_cap = (uint32_t)LONG_TEXT_CAP;
        TCMI_HIP(ctx, hipMemsetAsync(a.long_cursor, 0, 4, ctx->stream));
        TCMI_HIP(ctx, hipMemcpyAsync(d_cols, cols.data(), (size_t)n_pos * 4, hipMemcpyHostToDevice, ctx->stream));
        TCMI_HIP(ctx, hipMemcpyAsync(d_lo, lo_v.data(), (size_t)n_pos * 8, hipMemcpyHostToDevice, ctx->stream));
        TCMI_HIP(ctx, hipMemcpyAsync(d_off, off.data(), ((size_t)n_pos + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        (void)hipGetLastError();
        hipLaunchKernelGGL(ins_entries_kernel, dim3((unsigned)((total + PB - 1) / PB)), dim3(PB), 0, ctx->stream, a);
        TCMI_HIP(ctx, hipGetLastError());
        TCMI_HIP(ctx, hipMemcpyAsync(ctx->tok_host, a.out, (size_t)total * sizeof(tcmi_dev_entry), hipMemcpyDeviceToHost, ctx->stream));
        uint32_t long_used = 0;
        TCMI_HIP(ctx, hipMemcpyAsync(&long_used, a.long_cursor, 4, hipMemcpyDeviceToHost, ctx->stream));
        TCMI_HIP(ctx, hipStreamSynchronize(ctx->stream));       // (lo_v / off / cols were pageable: their copies are done)
        ents = (const tcmi_dev_entry *)ctx->tok_host;
        if (long_used) {                                        // (rare: a long insertion on a candidate column) its bases
            long_text.resize(std::min<size_t>(long_used, LONG_TEXT_CAP));
            TCMI_HIP(ctx, hipMemcpy(long_text.data(), a.long_text, long_text.size(), hipMemcpyDeviceToHost));
        }
    }
    *ents_out = ents;
    return TCMI_OK;
}

extern "C" int tcmi_readset_modal_tokens(tcmi_ctx *ctx, const tcmi_readset *rs, int32_t n_pos, const int64_t *positions,
                                         int32_t min_base_quality, uint32_t flag_filter, int ignore_orphans, int64_t max_depth,
                                         int ignore_overlaps, char *tokens, int64_t tokens_cap, int64_t *token_off, int64_t *n_tokens,
                                         int32_t *status_flags)
{
    if (!ctx || !rs || n_pos < 0 || (n_pos > 0 && (!positions || !tokens || !token_off || !n_tokens)))
        return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    if (!rs->parts.empty())
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "a read set of sub-ranges (tcmi_split_step): collect its entries (tcmi_readset_ins_entries) and vote on them (tcmi_modal_from_entries)");
    if (n_pos == 0) { if (status_flags) *status_flags = 0; return TCMI_OK; }
    std::vector<int64_t> off;
    std::vector<int32_t> cnt;
    std::vector<uint8_t> long_text;
    const tcmi_dev_entry *ents = nullptr;
    {
        const int rc = collect_ins_entries(ctx, rs, n_pos, positions, flag_filter, ignore_orphans, off, cnt, &ents, long_text);
        if (rc) return rc;
    }
    const int64_t nf = rs->f_reads;
    // the other mate of an overlapping pair, looked at on one reference position (rare: a pair with a deletion on a candidate column)
    const tcmi_prober prober = [&](const std::vector<tcmi_probe_req> &req, std::vector<tcmi_probe_res> &res) -> int {
        const size_t n = req.size();
        std::vector<int64_t> idx(n);
        std::vector<int32_t> ref(n);
        std::vector<uint32_t> out(n);
        for (size_t t = 0; t < n; ++t) {
            if (req[t].idx < 0 || req[t].idx >= nf) return tcmi_fail(ctx, TCMI_E_ARG, "internal: probe of read %lld", (long long)req[t].idx);
            idx[t] = req[t].idx; ref[t] = req[t].ref;
        }
        char *buf = nullptr;
        hipError_t e = hipMalloc((void **)&buf, n * 16);
        if (e != hipSuccess) return tcmi_fail(ctx, TCMI_E_NOMEM, "probe buffers: %s", hipGetErrorString(e));
        ProbeArgs a;
        a.src = stream_src(rs);
        a.c_idx = rs->d_cidx;
        a.idx = (const int64_t *)buf; a.ref = (const int32_t *)(buf + n * 8); a.out = (uint32_t *)(buf + n * 12); a.n = (int32_t)n;
        e = hipMemcpyAsync((void *)a.idx, idx.data(), n * 8, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync((void *)a.ref, ref.data(), n * 4, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) {
            (void)hipGetLastError();
            hipLaunchKernelGGL(ins_probe_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, a);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(out.data(), a.out, n * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        (void)hipFree(buf);
        if (e != hipSuccess) return tcmi_fail(ctx, TCMI_E_HIP, "probe kernel failed: %s", hipGetErrorString(e));
        for (size_t t = 0; t < n; ++t) res[t] = tcmi_probe_res{(uint8_t)(out[t] & 1u), (uint8_t)((out[t] >> 8) & 15u), (uint8_t)(out[t] >> 16)};
        return TCMI_OK;
    };
    return tcmi_modal_from_dev_entries(n_pos, ents, off.data(), cnt.data(), min_base_quality, max_depth, ignore_overlaps, &prober, tokens,
                                       tokens_cap, token_off, n_tokens, status_flags, long_text.data(), long_text.size());
}

// The entries themselves (48 bytes each, opaque to the caller) instead of the vote: ranks that share ONE file (BASELINE configs[4])
// each collect the entries of the candidate columns from the records of their own block range and send them to the rank that
// calls; concatenated in rank order (= file order) they are what tcmi_readset_modal_tokens votes on (tcmi_modal_from_entries).
extern "C" int tcmi_readset_ins_entries(tcmi_ctx *ctx, const tcmi_readset *rs, int32_t n_pos, const int64_t *positions, uint32_t flag_filter,
                                        int ignore_orphans, void *entries, int64_t entries_cap, int64_t *ent_off, uint8_t *long_text,
                                        int64_t long_cap, int64_t *long_used)
{
    if (!ctx || !rs || n_pos < 0 || !ent_off || (n_pos > 0 && !positions)) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    static_assert(sizeof(tcmi_dev_entry) == TCMI_INS_ENTRY_BYTES, "include/tcmi.h promises 48-byte entries");
    std::vector<int64_t> off;
    std::vector<int32_t> cnt;
    std::vector<uint8_t> text;
    const tcmi_dev_entry *ents = nullptr;
    if (!rs->parts.empty()) {
        // a read set of sub-ranges: the parts' entries per column one behind the other — file order —, the text offsets of a part's
        // long insertions moved behind the texts of the parts in front of it (what rank 0 does with the ranks' pieces)
        const size_t P = rs->parts.size();
        std::vector<std::vector<int64_t>> p_off(P);
        std::vector<std::vector<tcmi_dev_entry>> p_ent(P);
        std::vector<int64_t> p_base(P, 0);
        for (size_t p = 0; p < P; ++p) {
            const tcmi_readset::Part &pt = rs->parts[p];
            p_off[p].assign((size_t)n_pos + 1, 0);
            p_base[p] = (int64_t)text.size();
            if (pt.rs->n_piled == 0 || pt.rs->f_reads == 0) continue;
            std::vector<uint8_t> t1;
            const tcmi_dev_entry *e1 = nullptr;
            const int rc = collect_ins_entries(pt.cx, pt.rs, n_pos, positions, flag_filter, ignore_orphans, p_off[p], cnt, &e1, t1);
            if (rc) return tcmi_fail(ctx, rc, "%s", pt.cx->err.c_str());
            const int64_t n1 = p_off[p][(size_t)n_pos];
            if (n1) p_ent[p].assign(e1, e1 + n1);                // (the part's pinned scratch is its context's: copied out before the next call there)
            if (n1 && p_base[p]) {
                const int rc2 = tcmi_ins_entries_rebase(p_ent[p].data(), n1, p_base[p]);
                if (rc2) return rc2;
            }
            text.insert(text.end(), t1.begin(), t1.end());
        }
        ent_off[0] = 0;
        for (int32_t k = 0; k < n_pos; ++k) {
            int64_t n = 0;
            for (size_t p = 0; p < P; ++p) n += p_off[p][(size_t)k + 1] - p_off[p][(size_t)k];
            ent_off[k + 1] = ent_off[k] + n;
        }
        if (long_used) *long_used = (int64_t)text.size();
        if (ent_off[n_pos] > entries_cap || (int64_t)text.size() > long_cap)
            return tcmi_fail(ctx, TCMI_E_ARG, "entry buffer too small: %lld entries, %zu bytes of long insertions (ent_off / long_used say what is needed)",
                             (long long)ent_off[n_pos], text.size());
        tcmi_dev_entry *dst = static_cast<tcmi_dev_entry *>(entries);
        for (int32_t k = 0; k < n_pos; ++k)
            for (size_t p = 0; p < P; ++p) {
                const int64_t a = p_off[p][(size_t)k], b = p_off[p][(size_t)k + 1];
                if (b > a) { std::memcpy(dst, p_ent[p].data() + a, (size_t)(b - a) * sizeof(tcmi_dev_entry)); dst += b - a; }
            }
        if (!text.empty()) std::memcpy(long_text, text.data(), text.size());
        return TCMI_OK;
    }
    if (rs->n_piled == 0 || rs->f_reads == 0) {                 // (no kept reads in this range: no entries)
        for (int32_t k = 0; k <= n_pos; ++k) ent_off[k] = 0;
        if (long_used) *long_used = 0;
        return TCMI_OK;
    }
    const int rc = collect_ins_entries(ctx, rs, n_pos, positions, flag_filter, ignore_orphans, off, cnt, &ents, text);
    if (rc) return rc;
    for (int32_t k = 0; k <= n_pos; ++k) ent_off[k] = off[(size_t)k];
    if (long_used) *long_used = (int64_t)text.size();
    if (off[(size_t)n_pos] > entries_cap || (int64_t)text.size() > long_cap)
        return tcmi_fail(ctx, TCMI_E_ARG, "entry buffer too small: %lld entries, %zu bytes of long insertions (ent_off / long_used say what is needed)",
                         (long long)off[(size_t)n_pos], text.size());
    if (off[(size_t)n_pos]) std::memcpy(entries, ents, (size_t)off[(size_t)n_pos] * sizeof(tcmi_dev_entry));
    if (!text.empty()) std::memcpy(long_text, text.data(), text.size());
    return TCMI_OK;
}
