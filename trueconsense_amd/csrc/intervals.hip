// intervals.hip — the amplicon table on gfx950: order statistics of the coverage plane of the count matrix int32 [7][ld] over
// n intervals [start, end) of its axis -> one 32-byte tcmi_interval_stat per interval, in the order given (include/tcmi.h:
// tcmi_interval_stats_dev).  Intervals overlap, nest and repeat, so this is neither a partition nor a prefix scan: a segmented
// reduction plus an exact selection.
//
// One launch, one 256-lane workgroup per interval, no workgroup waits for another, no global atomics.
//   The columns at or beyond L have depth 0 and are never read: the interval is cut at L and the `zeros` columns behind the cut
//   enter every statistic by arithmetic (a key of their own for the minimum, one bucket of the selection's histogram), so an
//   interval that ends at 2^29 costs what its part below L costs.
//   pass 1   coalesced strided loads of the plane: sum, depths below the bound, and the smallest (depth, position) as one 64-bit
//            key — through the wavefront by shuffles, then through LDS, as var_count_kernel joins its four wavefronts.  The same
//            pass stages the flipped depths in LDS while the cut interval fits STAGE words.
//   median   the ((n - 1) / 2)-th smallest, by radix selection over the words with the sign bit flipped: up to four rounds of an
//            8-bit digit, most significant first (a digit that is the same in every word of the interval — pass 1 ORs the
//            differences — needs no round); each round histograms (LDS atomics) the words that carry the digits chosen so far,
//            one lane per bucket takes the exclusive prefix, and the one bucket that holds rank k names the next digit.  The words
//            come from LDS, or — a cut interval longer than STAGE — from the plane once more (L2).
//   record   lane 0, as two 16-byte stores where the destination allows it; the destination may be pinned host memory.
// The matrix is only read, and only plane TCMI_COV of it, and only below L.
#include "tcmi_internal.h"
#include "intervals_rule.h"

namespace {

constexpr int BLOCK = 256;
constexpr int STAGE = TCMI_IV_STAGE;                        // words of LDS that stage an interval (16 KiB)
typedef int vec4 __attribute__((ext_vector_type(4)));

struct IvArgs {
    const int32_t *cov;             // plane TCMI_COV of the matrix
    int64_t L;
    const int64_t *start, *end;
    int32_t min_depth;
    int wide;                       // the records start on 16 bytes
};

__global__ __launch_bounds__(BLOCK) void interval_stats_kernel(IvArgs a, tcmi_interval_stat *__restrict__ out)
{
    __shared__ uint32_t s_stage[STAGE];
    __shared__ int s_hist[256];
    __shared__ long long s_sum[BLOCK / 64], s_key[BLOCK / 64];
    __shared__ int s_below[BLOCK / 64], s_wave[BLOCK / 64];
    __shared__ uint32_t s_diff[BLOCK / 64];
    __shared__ int s_digit, s_k;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t s = a.start[blockIdx.x], e = a.end[blockIdx.x];
    // (the entry points have checked the intervals; the cuts below keep a damaged one inside the plane all the same)
    if (s < 0) s = 0;
    if (e > TCMI_IV_MAX_END) e = TCMI_IV_MAX_END;
    tcmi_interval_stat *const rec = out + blockIdx.x;
    if (e <= s) {                                           // (uniform over the workgroup)
        if (tid == 0) {
            if (a.wide) { vec4 *o = reinterpret_cast<vec4 *>(rec); o[0] = vec4{0, 0, 0, 0}; o[1] = vec4{-1, 0, 0, 0}; }
            else { int *o = reinterpret_cast<int *>(rec); o[0] = o[1] = o[2] = o[3] = 0; o[4] = -1; o[5] = o[6] = o[7] = 0; }
        }
        return;
    }
    const int n = (int)(e - s);                             // <= 2^29
    const int64_t s_cut = s < a.L ? s : a.L, e_cut = e < a.L ? e : a.L;
    const int m = (int)(e_cut - s_cut);                     // columns below L: the ones that are read
    const int zeros = n - m;                                // columns at or beyond L: depth 0, the first of them at max(s, L)
    const bool staged = m <= STAGE;
    const int32_t *const src = a.cov + s_cut;

    // ---- pass 1 ----
    long long sum = 0, key = INT64_MAX;
    int below = 0;
    // w0: one word of the interval (its first column, or a column behind L); diff: the bits in which any word differs from it
    const uint32_t w0 = m > 0 ? tcmi_iv_flip(src[0]) : 0x80000000u;
    uint32_t diff = zeros > 0 ? w0 ^ 0x80000000u : 0u;
    for (int k = tid; k < m; k += BLOCK) {
        const int32_t d = src[k];
        sum += d;
        below += d < a.min_depth;
        diff |= tcmi_iv_flip(d) ^ w0;
        const long long kk = tcmi_iv_key(d, s_cut + k);
        key = kk < key ? kk : key;
        if (staged) s_stage[k] = tcmi_iv_flip(d);
    }
    if (tid == 0 && zeros > 0) {
        const long long kk = tcmi_iv_key(0, s > a.L ? s : a.L);
        key = kk < key ? kk : key;
        below += 0 < a.min_depth ? zeros : 0;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        sum += __shfl_xor(sum, d, 64);
        below += __shfl_xor(below, d, 64);
        const long long other = __shfl_xor(key, d, 64);
        key = other < key ? other : key;
        diff |= (uint32_t)__shfl_xor((int)diff, d, 64);
    }
    if (lane == 0) { s_sum[wave] = sum; s_key[wave] = key; s_below[wave] = below; s_diff[wave] = diff; }
    if (tid == 0) s_k = (n - 1) / 2;
    __syncthreads();                                        // (also: the staged words are in LDS)

    // ---- the median: up to four rounds of radix selection ----
    // a digit in which no two words differ is w0's: its round is skipped (coverage seldom fills more than two bytes, so a real
    // matrix takes two rounds, not four, and never the rounds in which every word would add to one LDS counter)
    diff = s_diff[0] | s_diff[1] | s_diff[2] | s_diff[3];
    uint32_t prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (((diff >> shift) & 255u) == 0) {               // (uniform over the workgroup; rank k stays: every word is in this bucket)
            prefix |= w0 & (255u << shift);
            mask |= 255u << shift;
            continue;
        }
        s_hist[tid] = 0;
        __syncthreads();
        if (staged) {
            for (int k = tid; k < m; k += BLOCK) {
                const uint32_t w = s_stage[k];
                if ((w & mask) == prefix) atomicAdd(&s_hist[(w >> shift) & 255u], 1);
            }
        } else {
            for (int k = tid; k < m; k += BLOCK) {
                const uint32_t w = tcmi_iv_flip(src[k]);
                if ((w & mask) == prefix) atomicAdd(&s_hist[(w >> shift) & 255u], 1);
            }
        }
        if (tid == 0 && zeros > 0 && (0x80000000u & mask) == prefix) atomicAdd(&s_hist[(0x80000000u >> shift) & 255u], zeros);
        __syncthreads();
        // bucket tid's exclusive prefix (counts are at most 2^29: int holds them)
        const int h = s_hist[tid];
        int incl = h;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(incl, d, 64);
            if (lane >= d) incl += y;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int excl = incl - h;
        for (int w = 0; w < wave; ++w) excl += s_wave[w];
        const int k = s_k;
        __syncthreads();                                    // (everyone has read s_k and s_wave)
        if (k >= excl && k < excl + h) { s_digit = tid; s_k = k - excl; }       // exactly one bucket: the counts sum to more than k
        __syncthreads();
        prefix |= (uint32_t)s_digit << shift;
        mask |= 255u << shift;
    }

    if (tid == 0) {
        long long tsum = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        long long tkey = s_key[0];
        for (int w = 1; w < BLOCK / 64; ++w) tkey = s_key[w] < tkey ? s_key[w] : tkey;
        const int tbelow = s_below[0] + s_below[1] + s_below[2] + s_below[3];
        const int lo = (int)(uint32_t)(unsigned long long)tsum, hi = (int)(uint32_t)((unsigned long long)tsum >> 32);
        const int mn = (int)(tkey >> 32), mp = (int)(uint32_t)(unsigned long long)tkey;
        const int med = tcmi_iv_unflip(prefix);
        if (a.wide) { vec4 *o = reinterpret_cast<vec4 *>(rec); o[0] = vec4{lo, hi, n, mn}; o[1] = vec4{mp, med, tbelow, 0}; }
        else { int *o = reinterpret_cast<int *>(rec); o[0] = lo; o[1] = hi; o[2] = n; o[3] = mn; o[4] = mp; o[5] = med; o[6] = tbelow; o[7] = 0; }
    }
}

} // namespace

int tcmi_launch_intervals(tcmi_ctx *ctx, const tcmi_iv_job &j)
{
    if (j.n <= 0 || j.n > TCMI_IV_MAX_N) return tcmi_fail(ctx, TCMI_E_ARG, "intervals: nothing to launch over, or more than %d intervals", (int)TCMI_IV_MAX_N);
    IvArgs a = {j.counts + (int64_t)TCMI_COV * j.ld, j.L, j.start, j.end, j.min_depth, reinterpret_cast<uintptr_t>(j.records) % 16 == 0};
    tcmi_prof_begin(ctx, TCMI_K_INTERVALS);
    (void)hipGetLastError();                               // drop any stale error of this thread
    hipLaunchKernelGGL(interval_stats_kernel, dim3((unsigned)j.n), dim3(BLOCK), 0, ctx->stream, a, j.records);
    tcmi_prof_end(ctx, TCMI_K_INTERVALS);
    TCMI_HIP(ctx, hipGetLastError());
    return TCMI_OK;
}
