// variants.hip — the variant table on gfx950: count matrix int32 [7][ld] -> an ordered list of 16-byte records, one per
// (position, non-reference allele) that passes the rule of variants_rule.h (include/tcmi.h: tcmi_variants_dev).
//
// One lane per position, 256-lane workgroups, the planes read coalesced as call_kernel reads them.  Three launches on the
// context's stream, none of whose workgroups waits for another, and no atomics: the order of the records (position, then allele
// in plane order) is the order of the lanes, so it is the same in every run.
//   var_count_kernel   grid ceil(L / 256): popcount of each lane's allele mask, block sum -> blk_cnt[b]
//   var_scan_kernel    one workgroup: exclusive prefix of blk_cnt -> 64-bit blk_base, in chunks of 1024 with a carry (as pk_prefix
//                      of pack_device.hip); the total goes to a word the host can read (pinned memory)
//   var_emit_kernel    the count kernel's grid: the mask once more, the lane's exclusive offset inside the block (one wave64 ballot
//                      per allele, the four wavefronts joined through LDS as call_kernel joins its events), the lane's records at
//                      blk_base[b] + offset — one 16-byte store each, only below the capacity.  The destination may be pinned host
//                      memory: the step path's records cross PCIe as the kernel's own stores, and nothing else does.
// The matrix is only read.  Positions at or beyond n_ref give nothing, so the launches cover min(L, n_ref) positions.
#include "tcmi_internal.h"

namespace {

constexpr int BLOCK = 256;
constexpr int SCAN = 1024;
typedef int vec4 __attribute__((ext_vector_type(4)));       // a record as one 16-byte store

struct VarArgs {
    const int32_t *counts;
    int64_t L, ld;                  // L: positions the grid covers (already cut to n_ref)
    const uint8_t *ref;
    tcmi_var_rule rule;
};

// the allele mask of this lane's position (0 beyond L) and its counters
__device__ inline unsigned lane_mask(const VarArgs &a, int64_t p, int32_t c[TCMI_NCOL])
{
    if (p >= a.L) return 0u;
#pragma unroll
    for (int k = 0; k < TCMI_NCOL; ++k) c[k] = a.counts[(int64_t)k * a.ld + p];
    return tcmi_variant_mask(c, a.ref[p], a.rule);
}

__global__ __launch_bounds__(BLOCK) void var_count_kernel(VarArgs a, uint32_t *__restrict__ blk_cnt)
{
    __shared__ int wave_cnt[BLOCK / 64];
    int32_t c[TCMI_NCOL];
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    int n = __popc(lane_mask(a, p, c));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = (uint32_t)(wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3]);
}

// exclusive prefix sums of blk_cnt[0..n) -> blk_base[0..n), the total -> *total; one workgroup
__global__ __launch_bounds__(SCAN) void var_scan_kernel(const uint32_t *__restrict__ blk_cnt, int64_t n, unsigned long long *__restrict__ blk_base,
                                                        unsigned long long *total)
{
    __shared__ unsigned long long s_w[SCAN / 64];
    __shared__ unsigned long long s_run;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_run = 0;
    __syncthreads();
    for (int64_t i0 = 0; i0 < n; i0 += SCAN) {
        const int64_t i = i0 + tid;
        const unsigned long long x = i < n ? blk_cnt[i] : 0ull;
        unsigned long long incl = x;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long y = (unsigned long long)__shfl_up((long long)incl, d, 64);
            if (lane >= d) incl += y;
        }
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        unsigned long long before = s_run;
        for (int w = 0; w < wave; ++w) before += s_w[w];
        if (i < n) blk_base[i] = before + incl - x;
        __syncthreads();
        if (tid == SCAN - 1) s_run = before + incl;
        __syncthreads();
    }
    if (tid == 0) *total = s_run;
}

__global__ __launch_bounds__(BLOCK) void var_emit_kernel(VarArgs a, const unsigned long long *__restrict__ blk_base, tcmi_variant *__restrict__ out,
                                                         int64_t cap, int wide)
{
    __shared__ int wave_cnt[BLOCK / 64];
    int32_t c[TCMI_NCOL];
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const unsigned mask = lane_mask(a, p, c);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    int off = 0, in_wave = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {   // (every lane takes part in every ballot)
        const unsigned long long m = __ballot((mask >> k) & 1u);
        off += __popcll(m & below);
        in_wave += __popcll(m);
    }
    if (lane == 0) wave_cnt[wave] = in_wave;
    __syncthreads();
    for (int w = 0; w < wave; ++w) off += wave_cnt[w];
    if (!mask) return;
    int64_t at = (int64_t)blk_base[blockIdx.x] + off;
    vec4 *const out16 = reinterpret_cast<vec4 *>(out);      // (wide: the records start on 16 bytes)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (!((mask >> k) & 1u)) continue;
        if (at < cap) {
            if (wide) out16[at] = vec4{(int)p, k + 1, c[k + 1], c[0]};
            else { out[at].pos = (int32_t)p; out[at].allele = k + 1; out[at].count = c[k + 1]; out[at].cov = c[0]; }
        }
        ++at;
    }
}

} // namespace

int tcmi_launch_variants(tcmi_ctx *ctx, const tcmi_var_job &j)
{
    const int64_t Lv = j.L < j.n_ref ? j.L : j.n_ref;
    if (Lv <= 0) return tcmi_fail(ctx, TCMI_E_ARG, "variants: nothing to launch over");
    const int64_t grid = (Lv + BLOCK - 1) / BLOCK;
    VarArgs a = {j.counts, Lv, j.ld, j.ref, j.rule};
    const int wide = reinterpret_cast<uintptr_t>(j.records) % 16 == 0;
    tcmi_prof_begin(ctx, TCMI_K_VARIANTS);
    (void)hipGetLastError();                               // drop any stale error of this thread
    hipLaunchKernelGGL(var_count_kernel, dim3((unsigned)grid), dim3(BLOCK), 0, ctx->stream, a, j.blk_cnt);
    hipLaunchKernelGGL(var_scan_kernel, dim3(1), dim3(SCAN), 0, ctx->stream, j.blk_cnt, grid, j.blk_base, j.total);
    hipLaunchKernelGGL(var_emit_kernel, dim3((unsigned)grid), dim3(BLOCK), 0, ctx->stream, a, j.blk_base, j.records, j.cap, wide);
    tcmi_prof_end(ctx, TCMI_K_VARIANTS);
    TCMI_HIP(ctx, hipGetLastError());
    return TCMI_OK;
}
