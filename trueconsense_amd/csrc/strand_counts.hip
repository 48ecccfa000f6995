// strand_counts.hip — --variant-strand on gfx950: the count matrix's seven planes at given columns, split by the strand of the record
// (FLAG 0x10), counted in the inflated BAM stream a device-decoded read set left in the context's arena (include/tcmi.h:
// tcmi_readset_strand_counts).  The matrix sums the strands and the packed set does not keep the flag: only the records have it.
//
// One launch, one lane per record, 256-lane workgroups that stride over the records: the grid is min(ceil(records / 256), compute
// units x 8), as amplicon_reads.hip's.  LDS: the columns and [n][14] counters of up to TCMI_STRAND_LDS columns, 15 KiB.
//   per record   the fixed fields (view_rec), the read filter the set was built under (passes), the contig's shift (shift_of), one walk
//                over the CIGAR for the reference span [p, q], the primer table's head_end / tail_start when the set has one, then a
//                binary search for the first queried column >= p.  A record without a queried column in [p, q] — nearly every record
//                of a sparse query — is done here.
//   the walk     the others visit their queried columns in ascending order with ONE incremental walk of the CIGAR (the op index, the
//                op's first column and query index are kept between columns).  Per column the token rule of tally_stream_kernel
//                (tally.hip), restated for one column: a matched base counts coverage and its letter; a D column coverage and X,
//                unless it is the deletion's last column with an insertion behind it; an N column coverage; the I mark goes to the
//                last column of an op in front of an insertion; a token below the floor (a matched base by its own QUAL byte, a D / N
//                token by that of the query index at which its op starts, a query index at or beyond l_seq quality 0) or on a column
//                outside [head_end, tail_start) adds nothing at all, the I mark included.
//   counters     a sorted BAM puts a wavefront's 64 records on the same few columns: per round (each lane's next column) the lanes
//                that hit the same (column, strand) are joined by a ballot loop over the distinct keys, and per plane one lane adds
//                the popcount — to the workgroup's counters in LDS while the columns are staged, else to memory.  At its end a
//                workgroup hands every non-zero LDS counter to memory with one atomic add.
// The sums are integers: their order does not matter and every run gives the same numbers.  The stream is only read.
#include <algorithm>
#include <cstring>
#include <vector>

#include "pack_device.h"

namespace {

constexpr int BLOCK = 256;
constexpr int LDS_N = TCMI_STRAND_LDS;
constexpr int WG_PER_CU = 8;
constexpr int NK = 14;                  // counters per column: fwd[7] | rev[7] in plane order
constexpr int64_t MAX_N = 1 << 20;
constexpr int64_t MAX_COL = 1 << 29;

struct ScArgs {
    PackSrc src;                        // the resident stream, the read set's filter, floor and layout
    tcmi_primer_tab pt;                 // the primer table the read set was built under (none: zeros)
    const int32_t *cols;                // [n] ascending
    int32_t *counts;                    // [n][14]
    int32_t n;
};

// (the twin of tally.hip's stream_seg_find)
__device__ inline int32_t seg_value(const int32_t *t, int32_t n, int32_t x, int32_t none)
{
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (t[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo > 0 && x < t[n + lo - 1] ? t[2 * n + lo - 1] : none;
}

// a kept record between its queried columns
struct Walk {
    ReadView v;
    int32_t x, y;                       // the first column and the query index of op k
    uint32_t k;
    int32_t q;                          // the last column
    int32_t keep0, keep1;               // tokens on columns outside [keep0, keep1) are masked
};

// record i: kept exactly when the device packer keeps it (amplicon_reads.hip: slot_of) -> its walk at the head of the CIGAR
__device__ inline bool open_walk(const ScArgs &a, int64_t i, Walk &w)
{
    w.v = view_rec(a.src.stream + a.src.rec_off[i]);
    const ReadView &v = w.v;
    if ((v.flag & 0x4u) || !passes(a.src.flt, v) || v.bad || v.pos < 0) return false;
    const int32_t shift = shift_of(a.src, v.tid);
    if (shift < 0) return false;
    int64_t span = 0;
    for (uint32_t k = 0; k < v.n_cigar; ++k) {
        const uint32_t c = ld_u32(v.cigar + 4 * (size_t)k);
        if (consumes_ref(c & 0xFu)) span += c >> 4;
    }
    if (span <= 0) return false;
    const int64_t p = (int64_t)v.pos + shift, q = p + span - 1;
    if (p >= MAX_COL) return false;                         // (beyond every column that can be asked for)
    w.x = (int32_t)p; w.y = 0; w.k = 0;
    w.q = (int32_t)(q < MAX_COL ? q : MAX_COL);
    w.keep0 = INT32_MIN; w.keep1 = INT32_MAX;
    if (a.pt.n_head + a.pt.n_tail != 0) {
        w.keep0 = seg_value(a.pt.seg, a.pt.n_head, w.x, w.x);
        w.keep1 = seg_value(a.pt.seg + 3 * a.pt.n_head, a.pt.n_tail, w.q, w.q + 1);
    }
    return true;
}

// the planes the record's token on column c adds to (bit TCMI_COV..TCMI_I), c in [w.x, w.q] and not below an earlier call's
__device__ inline uint32_t token_at(Walk &w, int32_t c, uint32_t Q)
{
    const ReadView &v = w.v;
    uint32_t op = 0;
    int32_t len = 0;
    for (;; ++w.k) {                                        // on to the op that holds column c
        if (w.k >= v.n_cigar) return 0u;
        const uint32_t cw = ld_u32(v.cigar + 4 * (size_t)w.k);
        op = cw & 0xFu;
        len = (int32_t)(cw >> 4);
        if (consumes_ref(op)) {
            if (c - w.x < len) break;
            w.x += len;
        }
        if (consumes_query(op)) w.y += len;
    }
    if (c < w.keep0 || c >= w.keep1) return 0u;             // masked: nothing, the I mark included
    const int32_t j = c - w.x;
    const uint8_t *qual = v.seq + ((size_t)v.l_seq + 1) / 2;
    const int32_t qi = is_match(op) ? w.y + j : w.y;       // a D / N token is tested with the query index at which its op starts
    if (Q != 0u && (qi < v.l_seq ? byte_at(qual + qi) : 0u) < Q) return 0u;      // below the floor (Q = 0: nothing is, and QUAL is not read)
    const bool ins = j == len - 1 && ins_after(v.cigar, v.n_cigar, w.k);
    uint32_t bits = 1u << TCMI_COV;                         // M, =, X, D and N all count coverage
    if (is_match(op)) {
        const uint32_t nib = qi < v.l_seq ? nib_at(v.seq, qi) : 15u;           // past SEQ -> 'N'
        if (__popc(nib) == 1) { const int b = __ffs(nib) - 1; bits |= 1u << (b == 0 ? TCMI_A : b == 1 ? TCMI_C : b == 2 ? TCMI_G : TCMI_T); }
    } else if (op == 2 && !ins) bits |= 1u << TCMI_X;       // "*+.." does not count X
    if (ins) bits |= 1u << TCMI_I;
    return bits;
}

__device__ inline int32_t first_at_or_above(const int32_t *cols, int32_t n, int32_t p)
{
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (cols[mid] < p) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(BLOCK) void strand_counts_kernel(ScArgs a)
{
    __shared__ int32_t s_cols[LDS_N];
    __shared__ uint32_t s_cnt[NK * LDS_N];
    const int tid = threadIdx.x, lane = tid & 63;
    const bool staged = a.n <= LDS_N;                       // (uniform)
    const int n_cnt = NK * a.n;
    if (staged) {
        for (int k = tid; k < a.n; k += BLOCK) s_cols[k] = a.cols[k];
        for (int k = tid; k < n_cnt; k += BLOCK) s_cnt[k] = 0u;
        __syncthreads();
    }
    const int32_t *cols = staged ? s_cols : a.cols;
    const uint32_t Q = a.src.min_bq;
    // (the bound is uniform over the workgroup: every lane of a wavefront takes part in every ballot)
    for (int64_t base = (int64_t)blockIdx.x * BLOCK; base < a.src.n; base += (int64_t)gridDim.x * BLOCK) {
        const int64_t i = base + tid;
        Walk w;
        int32_t ci = 0;
        bool have = i < a.src.n && open_walk(a, i, w);
        if (have) {
            ci = first_at_or_above(cols, a.n, w.x);
            have = ci < a.n && cols[ci] <= w.q;
        }
        const uint32_t strand = have && (w.v.flag & 0x10u) ? 1u : 0u;
        while (__ballot(have)) {                            // one round per queried column of the wavefront's busiest record
            const uint32_t bits = have ? token_at(w, cols[ci], Q) : 0u;
            const uint32_t key = 2u * (uint32_t)ci + strand;
            bool todo = bits != 0u;
            for (;;) {                                      // one pass per distinct (column, strand) the round's tokens hit
                const unsigned long long m = __ballot(todo);
                if (!m) break;
                const int lead = (int)__builtin_ctzll(m);
                const uint32_t lk = __shfl(key, lead, 64);
                const bool same = todo && key == lk;
#pragma unroll
                for (int pl = 0; pl < TCMI_NCOL; ++pl) {
                    const unsigned long long mp = __ballot(same && ((bits >> pl) & 1u));
                    if (lane == lead && mp) {
                        if (staged) atomicAdd(&s_cnt[(NK / 2) * lk + pl], (uint32_t)__popcll(mp));
                        else atomicAdd(&a.counts[(int64_t)(NK / 2) * lk + pl], (int32_t)__popcll(mp));
                    }
                }
                if (same) todo = false;
            }
            if (have) {
                ++ci;
                have = ci < a.n && cols[ci] <= w.q;
            }
        }
    }
    if (staged) {
        __syncthreads();
        for (int k = tid; k < n_cnt; k += BLOCK) {
            const uint32_t c = s_cnt[k];
            if (c) atomicAdd(&a.counts[k], (int32_t)c);
        }
    }
}

// one read set on its own context: the columns (host, int32) -> sums[14 * n] ADDED to
int count_one(tcmi_ctx *ctx, const tcmi_readset *rs, int32_t n, const int32_t *cols, int64_t *sums)
{
    if (rs->packed_on_device != 2)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "strand counts: the read set was not decoded on the device (flat arrays or the host reader): there is no record stream to count in");
    if (rs->n_piled == 0) return TCMI_OK;                   // (no kept record: nothing to add; such a set may hold no stream at all)
    if (rs->device != ctx->device)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "strand counts: the read set lives on device %d, this context on device %d", rs->device, ctx->device);
    if (!rs->d_stream || !rs->d_rec_off || rs->arena_epoch != ctx->arena_epoch)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "strand counts: the read set's decoded stream is no longer resident on this context (another upload happened on it)");
    if (rs->n_lay && rs->lay_gen != ctx->lay_gen)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "strand counts: the context's contig layout changed since the read set was uploaded");
    TCMI_HIP(ctx, hipSetDevice(ctx->device));
    const size_t b_col = tcmi_align256((size_t)n * 4), b_cnt = tcmi_align256((size_t)NK * n * 4);
    // scratch of the context, grow-only and shared with tcmi_readset_amplicon_reads (both wait for the stream before they return)
    if (ctx->ar_dev_cap < b_col + b_cnt) {
        if (ctx->ar_dev) { TCMI_HIP(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(ctx->ar_dev); ctx->ar_dev = nullptr; ctx->ar_dev_cap = 0; }
        const size_t want = b_col + b_cnt + (64u << 10);
        if (hipMalloc((void **)&ctx->ar_dev, want) != hipSuccess) return tcmi_fail(ctx, TCMI_E_NOMEM, "strand counts: device scratch (%zu bytes)", want);
        ctx->ar_dev_cap = want;
    }
    char *pin = static_cast<char *>(tcmi_ctx_pinned(ctx, b_col + b_cnt));
    if (!pin) return tcmi_fail(ctx, TCMI_E_NOMEM, "strand counts: pinned scratch");
    std::memcpy(pin, cols, (size_t)n * 4);
    ScArgs a;
    a.src = stream_src(rs);
    a.src.lay = rs->d_lay; a.src.n_lay = rs->n_lay;
    a.pt = tcmi_primer_args(rs->primers);
    a.cols = reinterpret_cast<const int32_t *>(ctx->ar_dev);
    a.counts = reinterpret_cast<int32_t *>(ctx->ar_dev + b_col);
    a.n = n;
    TCMI_HIP(ctx, hipMemcpyAsync(ctx->ar_dev, pin, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    TCMI_HIP(ctx, hipMemsetAsync(a.counts, 0, (size_t)NK * n * 4, ctx->stream));
    if (rs->n_reads > 0) {
        const int64_t blocks = (rs->n_reads + BLOCK - 1) / BLOCK;
        const int64_t grid = std::min<int64_t>(blocks, (int64_t)std::max(ctx->n_cu, 1) * WG_PER_CU);
        (void)hipGetLastError();                            // drop any stale error of this thread
        tcmi_prof_begin(ctx, TCMI_K_STRAND_COUNTS);
        hipLaunchKernelGGL(strand_counts_kernel, dim3((unsigned)grid), dim3(BLOCK), 0, ctx->stream, a);
        tcmi_prof_end(ctx, TCMI_K_STRAND_COUNTS);
        TCMI_HIP(ctx, hipGetLastError());
    }
    TCMI_HIP(ctx, hipMemcpyAsync(pin + b_col, a.counts, (size_t)NK * n * 4, hipMemcpyDeviceToHost, ctx->stream));
    TCMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int32_t *got = reinterpret_cast<const int32_t *>(pin + b_col);
    for (int64_t k = 0; k < (int64_t)NK * n; ++k) sums[k] += got[k];
    return TCMI_OK;
}

} // namespace

extern "C" int tcmi_readset_strand_counts(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t n, const int64_t *cols, tcmi_strand_counts *records)
{
    if (!ctx || !rs) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    if (n < 1 || n > MAX_N) return tcmi_fail(ctx, TCMI_E_ARG, "strand counts: %lld columns: 1..1048576 are allowed", (long long)n);
    if (!cols || !records) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    for (int64_t i = 0; i < n; ++i) {
        if (cols[i] < 0 || cols[i] >= MAX_COL)
            return tcmi_fail(ctx, TCMI_E_ARG, "strand counts: column %lld (%lld) lies outside [0, 2^29)", (long long)i, (long long)cols[i]);
        if (i && cols[i] <= cols[i - 1])
            return tcmi_fail(ctx, TCMI_E_ARG, "strand counts: the columns are not strictly ascending at index %lld (%lld after %lld)", (long long)i,
                             (long long)cols[i], (long long)cols[i - 1]);
    }
    std::vector<int32_t> c32;
    std::vector<int64_t> sums;
    try {
        c32.assign(cols, cols + n);
        sums.assign((size_t)NK * (size_t)n, 0);
    } catch (...) {                                         // (no exception may cross the C ABI)
        return tcmi_fail(ctx, TCMI_E_NOMEM, "strand counts: no host memory for %lld columns", (long long)n);
    }
    if (!rs->parts.empty()) {
        // a read set of sub-ranges (tcmi_split_step, "split_sub"): every record starts in exactly one part — the sum over the parts,
        // each counted on its own context, where its stream lives
        for (const tcmi_readset::Part &pt : rs->parts) {
            const int rc = count_one(pt.cx, pt.rs, (int32_t)n, c32.data(), sums.data());
            if (rc) return tcmi_fail(ctx, rc, "%s", pt.cx->err.c_str());
        }
    } else {
        const int rc = count_one(ctx, rs, (int32_t)n, c32.data(), sums.data());
        if (rc) return rc;
    }
    for (int64_t i = 0; i < n; ++i) {
        for (int k = 0; k < TCMI_NCOL; ++k) {
            records[i].fwd[k] = (int32_t)sums[(size_t)(NK * i + k)];
            records[i].rev[k] = (int32_t)sums[(size_t)(NK * i + TCMI_NCOL + k)];
        }
        records[i].pos = (int32_t)cols[i];
        records[i].reserved = 0;
    }
    return TCMI_OK;
}
