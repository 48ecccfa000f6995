// tally.hip — stage A on gfx950: reads (CIGAR + 4-bit SEQ) -> per-position counters.
//
// Replaces indexing.BuildIndex (TrueConsense/indexing.py:75-154): htslib's pileup plus the
// per-token Python loop parse_query_sequences (indexing.py:102-132).  Semantics: SURVEY §8-P.
//
// One kernel per device read set (tcmi_internal.h), and one for what the device packer leaves in the stream:
//   tally_fast_kernel    ALIGNED reads (one match op): bit-sliced register accumulation,
//                        no atomics in the inner loop — see the comment above it.
//   tally_atomic_kernel  GENERAL reads (any CIGAR): token-by-token walk, LDS atomics.
//   tally_stream_kernel  reads of a device-decoded stream that span more than a chunk's window: one wavefront per read.
//
// tally_atomic_kernel decomposition (read-major; the count matrix is a commutative integer sum):
//   workgroup  = `rounds_per_wg` consecutive ROUNDS of 256 coordinate-sorted reads
//   LDS window = counters for WIN positions starting at the first read's position:
//                planes A,C,G,T,X,I (u32) + a coverage difference array
//   flush      = prefix-sum of the difference array, then one global atomic per touched
//                (plane, position), 64 consecutive positions per wave instruction.
// Tokens that fall outside the window (sparse input, long reads, unsorted input) go straight
// to global atomics: always correct, only slower.
//
// Integer work, HBM-streaming: no MFMA anywhere (BASELINE.json north_star).
#include "stream_count.h"

namespace {

constexpr int WIN = 512;        // positions per LDS window
constexpr int NPLANE = 6;       // A C G T X I
constexpr int BLOCK = 256;      // == TCMI_ROUND: one thread per read of a round

enum { PL_A = 0, PL_C = 1, PL_G = 2, PL_T = 3, PL_X = 4, PL_I = 5 };
__device__ constexpr int plane_col(int pl)
{
    return pl == PL_A ? TCMI_A : pl == PL_C ? TCMI_C : pl == PL_G ? TCMI_G : pl == PL_T ? TCMI_T : pl == PL_X ? TCMI_X : TCMI_I;
}

struct TallyArgs {
    const int32_t *pos;
    const uint32_t *meta;
    const int32_t *lseq;
    const uint32_t *cigar;
    const uint32_t *seq;
    const int64_t *round_cig;
    const int64_t *round_seq;
    int64_t n_piled;
    int64_t n_rounds;
    int64_t ld;
    int32_t *counts;
    int32_t L;
    int32_t rounds_per_wg;
};

// htslib resolve_cigar2's peek at the last reference base of op k, over aligned CIGAR words (its twin: pack_device.h's ins_after)
__device__ inline bool ins_after_words(const uint32_t *cg, int n, int k)
{
    if (k + 1 >= n) return false;
    const uint32_t op2 = cg[k + 1] & 0xF;
    int64_t tot = 0;
    if (op2 == 1) {
        tot = cg[k + 1] >> 4;
        for (int j = k + 2; j < n; ++j) {
            const uint32_t o = cg[j] & 0xF;
            if (o == 1) tot += cg[j] >> 4;
            else if (o != 6) break;
        }
    } else if (op2 == 6 && k + 2 < n) {
        for (int j = k + 2; j < n; ++j) {
            const uint32_t o = cg[j] & 0xF;
            if (o == 1) tot += cg[j] >> 4;
            else if (consumes_ref(o)) break;
        }
    }
    return tot > 0;
}

// inclusive block scan of a 64-bit value over 256 threads (4 waves of 64)
__device__ inline uint64_t block_scan_incl(uint64_t v, uint64_t *wave_tot /* LDS [4] */)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    __syncthreads();                       // wave_tot may still be read from a previous scan
    if (lane == 63) wave_tot[wave] = v;
    __syncthreads();
    uint64_t base = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w)
        if (w < wave) base += wave_tot[w];
    return v + base;
}

__device__ inline void add_token(uint32_t *win, const TallyArgs &a, int plane, int32_t p, int32_t P0)
{
    const uint32_t w = (uint32_t)(p - P0);
    if (w < (uint32_t)WIN) atomicAdd(&win[plane * WIN + w], 1u);
    else if ((uint32_t)p < (uint32_t)a.L) atomicAdd(&a.counts[(int64_t)plane_col(plane) * a.ld + p], 1);
}

// coverage of [x0, x1): in-window part through the difference array, the rest per position
__device__ inline void add_coverage(int32_t *covd, const TallyArgs &a, int32_t x0, int32_t x1, int32_t P0)
{
    const int32_t lo = max(x0, P0), hi = min(x1, P0 + WIN);
    if (lo < hi) {
        atomicAdd(&covd[lo - P0], 1);
        atomicAdd(&covd[hi - P0], -1);
        for (int32_t p = x0; p < min(x1, P0); ++p)
            if ((uint32_t)p < (uint32_t)a.L) atomicAdd(&a.counts[(int64_t)TCMI_COV * a.ld + p], 1);
        for (int32_t p = max(x0, P0 + WIN); p < x1; ++p)
            if ((uint32_t)p < (uint32_t)a.L) atomicAdd(&a.counts[(int64_t)TCMI_COV * a.ld + p], 1);
    } else {
        for (int32_t p = x0; p < x1; ++p)
            if ((uint32_t)p < (uint32_t)a.L) atomicAdd(&a.counts[(int64_t)TCMI_COV * a.ld + p], 1);
    }
}

// one read, token by token (general CIGAR)
__device__ inline void tally_read_general(uint32_t *win, int32_t *covd, const TallyArgs &a, int32_t pos, int nc,
                                          int32_t lq, const uint32_t *cg, const uint32_t *sq, int32_t P0)
{
    int32_t x = pos, y = 0;
    for (int k = 0; k < nc; ++k) {
        const uint32_t c = cg[k], op = c & 0xF;
        const int32_t len = (int32_t)(c >> 4);
        if (consumes_ref(op)) {
            const bool ins = len > 0 && ins_after_words(cg, nc, k);
            if (is_match(op)) {
                uint32_t word = 0;
                for (int32_t j = 0; j < len; ++j) {
                    const int32_t q = y + j;
                    uint32_t nib = 15u;                              // past SEQ -> 'N'
                    if (q < lq) {
                        if (j == 0 || (q & 7) == 0) word = sq[q >> 3];
                        nib = (word >> ((q & 7) * 4)) & 15u;
                    }
                    if (__popc(nib) == 1) add_token(win, a, __ffs(nib) - 1, x + j, P0);   // A=1 C=2 G=4 T=8
                }
            } else if (op == 2) {                                     // D: token "*" counts X ...
                const int32_t nx = ins ? len - 1 : len;              // ... but "*+.." does not
                for (int32_t j = 0; j < nx; ++j) add_token(win, a, PL_X, x + j, P0);
            }
            if (ins) add_token(win, a, PL_I, x + len - 1, P0);        // '+' in the token
            x += len;
        }
        if (consumes_query(op)) y += len;
    }
    add_coverage(covd, a, pos, x, P0);                                // M/=/X, D and N all add coverage
}

__global__ __launch_bounds__(BLOCK) void tally_atomic_kernel(TallyArgs a)
{
    __shared__ uint32_t win[NPLANE * WIN];
    __shared__ int32_t covd[WIN + 1];
    __shared__ uint64_t scan_tmp[4];

    const int t = threadIdx.x;
    const int64_t round0 = (int64_t)blockIdx.x * a.rounds_per_wg;
    if (round0 >= a.n_rounds) return;
    const int64_t round1 = min(round0 + a.rounds_per_wg, a.n_rounds);
    const int32_t P0 = a.pos[round0 * BLOCK];

    for (int i = t; i < NPLANE * WIN; i += BLOCK) win[i] = 0;
    for (int i = t; i <= WIN; i += BLOCK) covd[i] = 0;
    __syncthreads();

    for (int64_t rd = round0; rd < round1; ++rd) {
        const int64_t r = rd * BLOCK + t;
        const bool valid = r < a.n_piled;
        int32_t pos = 0, lq = 0;
        uint32_t meta = 0;
        if (valid) { pos = a.pos[r]; meta = a.meta[r]; lq = a.lseq[r]; }
        const uint32_t nc = meta & 0xFFFFu;
        const uint32_t nw = (uint32_t)(lq + 7) >> 3;
        const uint64_t mine = ((uint64_t)nw << 32) | nc;
        const uint64_t excl = block_scan_incl(mine, scan_tmp) - mine;
        if (valid) {
            const uint32_t *cg = a.cigar + a.round_cig[rd] + (uint32_t)excl;
            const uint32_t *sq = a.seq + a.round_seq[rd] + (excl >> 32);
            tally_read_general(win, covd, a, pos, (int)nc, lq, cg, sq, P0);
        }
    }
    __syncthreads();

    // coverage: inclusive prefix sum of the difference array (2 entries per thread)
    {
        const int32_t d0 = covd[2 * t], d1 = covd[2 * t + 1];
        const uint64_t incl = block_scan_incl((uint64_t)(int64_t)(d0 + d1), scan_tmp);
        const int32_t before = (int32_t)(int64_t)incl - (d0 + d1);
        __syncthreads();
        covd[2 * t] = before + d0;
        covd[2 * t + 1] = before + d0 + d1;
    }
    __syncthreads();
    for (int w = t; w < WIN; w += BLOCK) {
        const int32_t p = P0 + w;
        if ((uint32_t)p >= (uint32_t)a.L) continue;
        const int32_t cv = covd[w];
        if (cv) atomicAdd(&a.counts[(int64_t)TCMI_COV * a.ld + p], cv);
#pragma unroll
        for (int pl = 0; pl < NPLANE; ++pl) {
            const uint32_t v = win[pl * WIN + w];
            if (v) atomicAdd(&a.counts[(int64_t)plane_col(pl) * a.ld + p], (int32_t)v);
        }
    }
}

// ---- tally_stream_kernel: the reads the packer left out (spans above TCMI_D_MAXLEN), straight from the inflated BAM stream -------
// One wavefront per read.  The CIGAR is walked op by op (wave-uniform), the lanes take the positions of an op 64 at a time and add
// each token to the count matrix with a global atomic — the token rules of tally_read_general above: a
// matched base counts by its letter, a deleted position counts X unless an insertion follows the deletion's last base ("*+.."),
// the last reference base in front of an insertion counts I, every position from pos to the end counts coverage (M, =, X, D, N).
// Under a base-quality floor (s.min_bq > 0) a token whose quality is below it is skipped — no coverage, no letter, no X, no I —:
// a matched base has its own QUAL byte, a D / N token that of the next query base (the query index at which the op starts), a query
// index at or beyond l_seq quality 0; coverage is then added token by token.
// Under a primer table (pt; tcmi_ctx_set_primers) the read's head_end and tail_start are looked up once — its CIGAR's reference length
// first, for the last column — and a token on a column outside [head_end, tail_start) is skipped likewise, column by column: a D / N
// op that crosses the mask's edge loses only its masked columns, the I mark goes with the op's last column.  Coverage token by token
// then too; without a floor a query index at or beyond l_seq is not skipped outside the mask.  Under the mate-overlap rule (pt.clip;
// tcmi_ctx_set_mate_overlap) head_end is at least the read's first column + its clip: the same mask, token by token likewise.
__global__ __launch_bounds__(256) void tally_stream_kernel(PackSrc s, const uint32_t *gen_idx, uint32_t n_gen, int32_t *counts, int64_t ld, int32_t L,
                                                           tcmi_primer_tab pt)
{
    const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= n_gen) return;
    const ReadView v = view(s, (int64_t)gen_idx[w]);
    auto add = [&](int col, int32_t p) { if ((uint32_t)p < (uint32_t)L) atomicAdd(&counts[(int64_t)col * ld + p], 1); };
    const uint32_t Q = s.min_bq;
    const uint8_t *qual = v.seq + ((size_t)v.l_seq + 1) / 2;
    auto skipped = [&](int32_t q) { return qual_at(qual, v.l_seq, q) < Q; };                  // (Q = 0: nothing is)
    int32_t x = v.pos + shift_of(s, v.tid), y = 0;
    const int32_t x0 = x;
    const bool table = pt.n_head + pt.n_tail != 0;
    const bool by_token = Q != 0u || table || pt.clip != nullptr;      // coverage token by token
    int32_t keep0 = INT32_MIN, keep1 = INT32_MAX;               // tokens on columns outside [keep0, keep1) are masked
    if (table) {
        const int32_t span = (int32_t)ref_span(v);
        keep0 = seg_find(pt.seg, pt.n_head, x0, x0);
        keep1 = seg_find(pt.seg + 3 * pt.n_head, pt.n_tail, x0 + span - 1, x0 + span);
    }
    if (pt.clip) keep0 = max(keep0, x0 + (int32_t)pt.clip[gen_idx[w]]);        // (the mate join: the read's first clip columns are its mate's)
    auto masked = [&](int32_t col) { return col < keep0 || col >= keep1; };
    for (uint32_t k = 0; k < v.n_cigar; ++k) {
        const uint32_t c = ld_u32(v.cigar + 4 * (size_t)k), op = c & 0xFu;
        const int32_t len = (int32_t)(c >> 4);
        if (consumes_ref(op)) {
            const bool ins = len > 0 && ins_after(v.cigar, v.n_cigar, k);
            bool skip_last = false;
            if (by_token && len > 0) skip_last = skipped(is_match(op) ? y + len - 1 : y) || masked(x + len - 1);
            if (is_match(op)) {
                for (int32_t j = lane; j < len; j += 64) {
                    const int32_t q = y + j;
                    if (by_token) { if (skipped(q) || masked(x + j)) continue; add(TCMI_COV, x + j); }
                    const uint32_t nib = q < v.l_seq ? nib_at(v.seq, q) : 15u;          // past SEQ -> 'N'
                    if (__popc(nib) == 1) add(base_plane(nib), x + j);
                }
            } else if (!skipped(y)) {                                                 // (the floor skips a D / N op whole; Q = 0: never)
                const int32_t nx = ins ? len - 1 : len;                              // "*+.." does not count X
                for (int32_t j = lane; j < len; j += 64) {
                    if (masked(x + j)) continue;
                    if (by_token) add(TCMI_COV, x + j);
                    if (op == 2 && j < nx) add(TCMI_X, x + j);
                }
            }
            if (ins && !skip_last && lane == 0) add(TCMI_I, x + len - 1);
            x += len;
        }
        if (consumes_query(op)) y += len;
    }
    if (!by_token) for (int32_t p = x0 + lane; p < x; p += 64) add(TCMI_COV, p);
}

} // namespace

// the long reads of a device-decoded read set into the count matrix (behind the packed set's kernel)
static int launch_tally_stream(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t L, int64_t ld, int32_t *d_counts)
{
    if (rs->s_reads <= 0) return TCMI_OK;
    if (tcmi_stream_gone(ctx, rs))
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "the read set's long reads lie in a decoded stream that is gone (another upload on this context): upload it again");
    PackSrc s = stream_src(rs);
    if (rs->n_lay && rs->lay_gen != ctx->lay_gen)
        return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "the context's contig layout changed since the read set was uploaded: upload it again");
    s.lay = rs->d_lay; s.n_lay = rs->n_lay;
    (void)hipGetLastError();
    tcmi_prof_begin(ctx, TCMI_K_TALLY_GENERAL);
    hipLaunchKernelGGL(tally_stream_kernel, dim3((unsigned)((rs->s_reads + 3) / 4)), dim3(256), 0, ctx->stream, s, rs->d_gen_idx, (uint32_t)rs->s_reads,
                       d_counts, ld, (int32_t)L, tcmi_mask_args(rs));
    tcmi_prof_end(ctx, TCMI_K_TALLY_GENERAL);
    TCMI_HIP(ctx, hipGetLastError());
    return TCMI_OK;
}

int tcmi_launch_tally(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t L, int64_t ld, int32_t *d_counts)
{
    if (rs->f_chunks > 0 || (ctx->ride && rs->g_reads == 0)) {   // (an empty fast launch still carries a ride-along call)
        const int rc = tcmi_launch_tally_fast(ctx, rs, L, ld, d_counts);
        if (rc) return rc;
    }
    if (rs->s_reads > 0) {                                    // long reads of a device-decoded stream
        const int rc = launch_tally_stream(ctx, rs, L, ld, d_counts);
        if (rc) return rc;
    }
    if (rs->g_reads == 0) return TCMI_OK;
    TallyArgs a;
    a.pos = rs->d_pos; a.meta = rs->d_meta; a.lseq = rs->d_lseq; a.cigar = rs->d_cigar; a.seq = rs->d_seq;
    a.round_cig = rs->d_round_cig; a.round_seq = rs->d_round_seq;
    a.n_piled = rs->g_reads; a.n_rounds = rs->n_rounds; a.ld = ld; a.counts = d_counts; a.L = (int32_t)L;
    int rpw = ctx->rounds_per_wg;
    if (rpw <= 0) rpw = rs->n_rounds >= 4096 ? 4 : rs->n_rounds >= 1024 ? 2 : 1;
    a.rounds_per_wg = rpw;
    const int64_t grid = (rs->n_rounds + rpw - 1) / rpw;
    if (grid <= 0 || grid > INT32_MAX) return tcmi_fail(ctx, TCMI_E_ARG, "bad grid %lld", (long long)grid);
    tcmi_prof_begin(ctx, TCMI_K_TALLY_GENERAL);
    (void)hipGetLastError();                               // drop any stale error of this thread
    hipLaunchKernelGGL(tally_atomic_kernel, dim3((unsigned)grid), dim3(BLOCK), 0, ctx->stream, a);
    tcmi_prof_end(ctx, TCMI_K_TALLY_GENERAL);
    TCMI_HIP(ctx, hipGetLastError());
    return TCMI_OK;
}
