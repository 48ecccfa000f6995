// tally_planes.hip — stage A for ALIGNED reads on gfx950, bases as 2-bit codes in two bit planes.
// Counterpart of the per-token loop of indexing.py:102-132 for the tokens that are plain bases
// (SURVEY §8-P2).
//
// Data (readset_layout.h): per read ONE packed header word and its aligned bases as codes
// A=0 C=1 G=2 T=3 (anything else 0, listed as an OTHER event), 32 bases per pair of 32-bit words
// {lo plane, hi plane}, with one zero pair between reads: 52 bytes for a 150-bp read.  The layout is
// produced on the device by pack_device.hip (default) or on the host by host_pack.cpp.
//
// One workgroup per chunk (<= 8 stages of <= 510 reads), lane (g, s) owns 32 positions g of the
// window and depth slice s of the reads.  Per read of the slice: one 64-bit LDS header, ONE
// ds_read2_b64 (two pairs), two v_alignbit funnel shifts bring the read's planes onto the lane's
// 32 positions (a lane that straddles an end of the read sees the zero pair there; a lane wholly
// outside the read is told so by its clamped pair index and takes zeros); lo, hi and lo&hi
// (= C|T, G|T, T) are then COUNTED BIT-SLICED: carry-save adders (sum and carry: one v_bitop3_b32
// each) fold eight reads into the ones / twos / fours planes and an eights carry that ripples through
// the upper planes (8 planes: <= 255 reads per lane and chunk).  ~19 VALU instructions per read and
// 32 positions.  At the end of the chunk the planes are spread into byte counters once, the slices
// are summed through LDS, and per position
//     C = n(lo) - n(lo&hi),  G = n(hi) - n(lo&hi),  T = n(lo&hi),  A = coverage - C - G - T
// (covered positions without an A/C/G/T base land in A and are taken out by the tail blocks).
// Coverage comes from the packer's per-chunk list of runs of reads with equal (position, length):
// a (+n, -n) pair per run in an LDS difference array, prefix-summed at the end.
//
// HBM-streaming integer work: no MFMA (BASELINE.json north_star).
#include <algorithm>

#include "tally_common.h"

namespace {

#ifndef TCMI_P_BODY8
#define TCMI_P_BODY8 1   // 0: four-read bodies only (fewer live registers, more carry ripples)
#endif
constexpr int NPL = TCMI_P_NPL;                 // counter planes per vector
constexpr int CPL = (MAXPOS + FB - 1) / FB;     // coverage entries per lane in the final prefix sum
static_assert(NLD * FB * 4 <= TCMI_F_SEQCAP, "the unconditional stage stores must fit the stage buffer");

// carry-save adder on bit vectors: sum and carry of three inputs (one v_bitop3_b32 each on gfx950;
// truth table: bit i of the immediate = f(a = i >> 2 & 1, b = i >> 1 & 1, c = i & 1))
#define TCMI_XOR3(a_, b_, c_) __builtin_amdgcn_bitop3_b32((a_), (b_), (c_), 0x96)
#define TCMI_MAJ(a_, b_, c_) __builtin_amdgcn_bitop3_b32((a_), (b_), (c_), 0xE8)

struct Planes {                                 // one bit-sliced counter per bit position: value = sum p[k] << k
    uint32_t p[NPL];
};

// fold eight bit vectors into the counter: seven carry-save adders, then the eights carry ripples upward
__device__ inline void add8(Planes &c, const uint32_t (&x)[8])
{
    const uint32_t s1 = TCMI_XOR3(c.p[0], x[0], x[1]), c1 = TCMI_MAJ(c.p[0], x[0], x[1]);
    const uint32_t s2 = TCMI_XOR3(s1, x[2], x[3]), c2 = TCMI_MAJ(s1, x[2], x[3]);
    const uint32_t s3 = TCMI_XOR3(s2, x[4], x[5]), c3 = TCMI_MAJ(s2, x[4], x[5]);
    c.p[0] = TCMI_XOR3(s3, x[6], x[7]);
    const uint32_t c4 = TCMI_MAJ(s3, x[6], x[7]);
    const uint32_t t1 = TCMI_XOR3(c.p[1], c1, c2), d1 = TCMI_MAJ(c.p[1], c1, c2);
    c.p[1] = TCMI_XOR3(t1, c3, c4);
    const uint32_t d2 = TCMI_MAJ(t1, c3, c4);
    uint32_t e = TCMI_MAJ(c.p[2], d1, d2);
    c.p[2] = TCMI_XOR3(c.p[2], d1, d2);
#pragma unroll
    for (int k = 3; k < NPL - 1; ++k) {
        const uint32_t t = c.p[k] & e;
        c.p[k] ^= e;
        e = t;
    }
    c.p[NPL - 1] ^= e;
}

// fold four bit vectors into the counter (the remainder of a stage)
__device__ inline void add4(Planes &c, const uint32_t (&x)[4])
{
    const uint32_t s1 = TCMI_XOR3(c.p[0], x[0], x[1]), c1 = TCMI_MAJ(c.p[0], x[0], x[1]);
    c.p[0] = TCMI_XOR3(s1, x[2], x[3]);
    const uint32_t c2 = TCMI_MAJ(s1, x[2], x[3]);
    uint32_t e = TCMI_MAJ(c.p[1], c1, c2);
    c.p[1] = TCMI_XOR3(c.p[1], c1, c2);
#pragma unroll
    for (int k = 2; k < NPL - 1; ++k) {
        const uint32_t t = c.p[k] & e;
        c.p[k] ^= e;
        e = t;
    }
    c.p[NPL - 1] ^= e;
}

// byte i of the result = count at bit position J + 8 i, from the planes [0, NP) (the others are known to be zero):
// one shift and one v_and_or_b32 per plane
template <int J, int NP>
__device__ inline uint32_t spread(const Planes &c)
{
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const uint32_t m = 0x01010101u << k;
        const uint32_t v = J >= k ? (c.p[k] >> (J - k)) : (c.p[k] << (k - J));
        r = __builtin_amdgcn_bitop3_b32(v, m, r, 0xEA);     // (v & m) | r
    }
    return r;
}

// the bit-sliced counters of a lane -> eight registers of four byte counters each, stored [register][lane]
template <int NP, int NV>
__device__ inline void spread_all(const Planes (&cnt)[NV], uint32_t *s_part, int tid)
{
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        s_part[(v * 8 + 0) * FB + tid] = spread<0, NP>(cnt[v]);
        s_part[(v * 8 + 1) * FB + tid] = spread<1, NP>(cnt[v]);
        s_part[(v * 8 + 2) * FB + tid] = spread<2, NP>(cnt[v]);
        s_part[(v * 8 + 3) * FB + tid] = spread<3, NP>(cnt[v]);
        s_part[(v * 8 + 4) * FB + tid] = spread<4, NP>(cnt[v]);
        s_part[(v * 8 + 5) * FB + tid] = spread<5, NP>(cnt[v]);
        s_part[(v * 8 + 6) * FB + tid] = spread<6, NP>(cnt[v]);
        s_part[(v * 8 + 7) * FB + tid] = spread<7, NP>(cnt[v]);
    }
}

// DROP (tally_planes_drop_kernel): a read set packed under a base-quality floor carries a third plane, one word per pair (a.drop;
// the packer has taken the skipped tokens out of lo / hi and pushed no event for them).  Its words are staged behind the pairs, funnel-
// shifted like lo and hi and counted in a FOURTH bit-sliced counter; per position coverage = runs - n(drop), and A = coverage - C - G - T
// needs no change.  LDS: 12 KiB more for the staged drop words and 1.5 KiB more for the fourth window counter.
constexpr int DROP_WAVES = 3;                   // workgroups per CU the drop variant's registers and LDS (46 KiB) are set for
#define TCMI_TALLY_DROP 0
__global__ __launch_bounds__(FB, TCMI_P_WAVES) void tally_planes_kernel(FastArgs a)
#include "tally_planes_body.h"
#undef TCMI_TALLY_DROP
#define TCMI_TALLY_DROP 1
__global__ __launch_bounds__(FB, DROP_WAVES) void tally_planes_drop_kernel(FastArgs a)
#include "tally_planes_body.h"
#undef TCMI_TALLY_DROP
#undef TCMI_XOR3
#undef TCMI_MAJ

} // namespace



// Launch over the aligned set of a read set: [ride-along call blocks][tail blocks: event words][chunk blocks].
int tcmi_launch_tally_fast(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t L, int64_t ld, int32_t *d_counts)
{
    FastArgs a = {};
    a.lenoff = rs->d_flenoff; a.seq = rs->d_fseq; a.chunks = rs->d_fchunk; a.events = rs->d_fevent; a.covrun = rs->d_fcovrun;
    a.counts = d_counts; a.ld = ld; a.n_events = rs->f_events; a.L = (int32_t)L;
    a.drop = rs->d_fdrop;                                       // (a read set packed under a base-quality floor: the drop variant)
    const int wg_per_cu = a.drop ? std::min(ctx->wg_per_cu, DROP_WAVES) : ctx->wg_per_cu;
    a.pair_ok = (ld % 2 == 0) && (reinterpret_cast<uintptr_t>(d_counts) % 8 == 0);
    a.n_tail = (int32_t)((rs->f_events + FB - 1) / FB);
    int64_t n_chunk_blocks = rs->f_chunks;
    if (rs->d_dev_counts) {                                     // totals still on the device: f_chunks / f_events are the capacities
        a.dev_counts = rs->d_dev_counts;
        a.n_tail = (int32_t)std::min<int64_t>(a.n_tail, 128);
        // (one round of the chip's slots and a half: pk_pack cuts a file into about one chunk per slot; a file with more takes turns)
        n_chunk_blocks = std::min<int64_t>(n_chunk_blocks, (int64_t)ctx->n_cu * wg_per_cu * 3 / 2);
    }
    a.n_chunk_blocks = (int32_t)std::max<int64_t>(1, n_chunk_blocks);
    int64_t grid = (rs->f_chunks ? n_chunk_blocks : 0) + a.n_tail;
    if (ctx->ride && !ctx->ride->taken) {                     // carry another workspace's call in this launch
        tcmi_ride *r = ctx->ride;
        a.counts2 = r->counts; a.ld2 = r->ld; a.L2 = (int32_t)r->L; a.n_call2 = (int32_t)((r->L + TILE - 1) / TILE);
        a.mincov = r->mincov; a.include_ambig = r->amb; a.plain = r->plain; a.alt = r->alt; a.flags = r->flags;
        grid += a.n_call2;
        r->taken = true;
    }
    if (grid > INT32_MAX) return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "too many chunks");
    if (grid == 0) return TCMI_OK;
    a.n_chunks = (int32_t)rs->f_chunks;
    tcmi_prof_begin(ctx, TCMI_K_TALLY);
    (void)hipGetLastError();                                   // drop any stale error of this thread
    if (a.drop) hipLaunchKernelGGL(tally_planes_drop_kernel, dim3((unsigned)grid), dim3(FB), 0, ctx->stream, a);
    else hipLaunchKernelGGL(tally_planes_kernel, dim3((unsigned)grid), dim3(FB), 0, ctx->stream, a);
    tcmi_prof_end(ctx, TCMI_K_TALLY);
    TCMI_HIP(ctx, hipGetLastError());
    return TCMI_OK;
}
