// bgzf_copy.hip — DEVICE: a BGZF block's tokens -> its bytes in the inflated BAM stream, the record starts in it, its CRC-32 (the second
// of the device decoder's two kernels: bgzf_device.h says why there are two and what a token is; bgzf_symbols.hip writes the tokens).
//
// A match may copy what the previous match produced: the second serial chain of a deflate stream.  bgzf_copy takes 64 tokens at
// a time: an inclusive scan of the lengths gives every token its output position, the literals of a stretch go to the ring at once,
// the matches one after the other (TCMI_LM_ASM: a byte a lane up to 64 bytes, an aligned dword a lane beyond — the LDS takes
// unaligned words at about a cycle a LANE —; teams of eight lanes for up to eight independent short matches in files of short
// tokens; in files under 4 : 1 the far matches of up to 8 bytes are finished in the batch's set-up, straight from the flushed
// stream).  The ring is 8 KB of LDS that hold the recent output; while a segment of it is flushed to the stream the chain of BAM
// records is followed through it and the segment's part of the block's CRC-32 is taken.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>

#include "bgzf_device.h"

namespace {

#ifndef TCMI_COPY_RING
#define TCMI_COPY_RING 8192
#endif
#ifndef TCMI_COPY_SEG
#define TCMI_COPY_SEG 2048
#endif
constexpr int CWIN = TCMI_COPY_RING, CWMASK = CWIN - 1;       // bgzf_copy's ring of recent output
constexpr int CSEG = TCMI_COPY_SEG;
// a round of bgzf_copy writes the literals of up to CSEG + 258 bytes ahead of the match it copies: what a match may still read
// from the ring ends that much earlier; a source further back has been flushed (CWIN >= 2 CSEG + 522)
constexpr int CNEAR = CWIN - CSEG - 264;
static_assert(CWIN >= 2 * CSEG + 528 && (CWIN & (CWIN - 1)) == 0 && CWIN % CSEG == 0, "a far match must find its source flushed");
constexpr int FAR_WORDS = 128;                       // bgzf_copy: words of LDS in which the sources of a batch's far matches are parked
constexpr int TEAM_BATCH_BYTES = 1536;               // bgzf_copy: a batch of 64 tokens this short (<= 24 bytes a token) copies its matches in teams

struct CopyArgs {
    const uint8_t *file;        // compressed file (raw tokens copy from it)
    const BlockDesc *blocks;
    const uint32_t *tokens;
    const uint32_t *n_tok;
    uint8_t *out;
    uint32_t *rec_slot;
    uint32_t *n_rec;
    int32_t *overshoot;         // bytes by which the block's last record runs into the next blocks (0x7FFFFFFF: its size field does)
    uint32_t *first_rec;        // offset of the first record start found in the block (0xFFFFFFFF: none)
    uint32_t *status;           // in: bgzf_symbols' verdict; out: the block's
    int32_t n_blocks;           // (the launch's blocks end here)
    int32_t first_block;        // ... and start here
    uint32_t n_ref;             // reference sequences of the BAM header
    uint64_t *stamps;           // diagnostic, as SymArgs::stamps
    uint32_t team_bytes;        // a batch of 64 tokens with at most this many bytes of output copies its matches in teams
    // the CRC-32 of every block's output against the value in its trailer (SAM spec 4.1; htslib checks it on every block it reads), taken
    // while the bytes are flushed from the ring (crc != 0):
    uint32_t crc;
    uint32_t zeros_seg[32];     // zeros_seg[i]: the CRC register with only bit i set, CSEG zero bytes later
    const uint32_t *crc_ops;    // [CRC_NOPS][8][16]: the register after 2^k more zero bytes, by nibble (crc_later)
};

// The copy loop of the matches of a stretch, hand-scheduled.  mm: the matches still to be copied; pm: those of them the inner loop
// takes unasked — plain (source in the ring or parked next to it, source and destination apart by the match's length at least) and
// of eight bytes or more.  14 instructions a match: EIGHT bytes a lane at min(8 lane, len - 8) (the last piece overlaps the one
// before instead of running past the end; LDS takes any byte address); the operands come packed for it (vA2 = (len - 1) << 16 |
// (destination - 7) & 0xffff, vB2 = source - 7): one v_cmpx gives the lane mask (vA2 >= 8 lane << 16  <=>  len > 8 lane), one SDWA
// v_min the piece's place + 7, two adds the addresses (the destination's within 16 bits); the NEXT match's operands are fetched
// while the LDS read is under way.  (A CU of these wavefronts issues about one instruction a cycle, whatever its kind: what counts
// is the number of instructions.)  Then the first other match: a plain one of 3 - 7 bytes goes byte-wise (LMs); a far match
// (source flushed to HBM long ago) is copied here too, 64 bytes a load; anything else leaves with its lane in j (C++ copies it:
// periods shorter than the match, ranges across the ring's end) — or j = -1: all done.
#define TCMI_LM_ASM() \
                    asm volatile( \
                        "s_mov_b64 s[92:93], exec\n" \
                        "LO%=:\n" \
                        "s_andn2_b64 s[80:81], %[mm], %[pm]\n" \
                        "s_ff1_i32_b64 %[j], s[80:81]\n" \
                        "s_mov_b64 s[82:83], %[mm]\n" \
                        "s_cmp_lt_i32 %[j], 0\n" \
                        "s_cbranch_scc1 LR%=\n" \
                        "s_lshl_b64 s[82:83], 1, %[j]\n" \
                        "s_sub_u32 s82, s82, 1\n" \
                        "s_subb_u32 s83, s83, 0\n" \
                        "s_and_b64 s[82:83], s[82:83], %[mm]\n" \
                        "LR%=:\n" \
                        "s_andn2_b64 %[mm], %[mm], s[82:83]\n" \
                        "s_cmp_eq_u64 s[82:83], 0\n" \
                        "s_cbranch_scc1 LN%=\n" \
                        "LM%=:\n" \
                        "s_ff1_i32_b64 s84, s[82:83]\n" \
                        "v_readlane_b32 %[sa], %[vA2], s84\n" \
                        "v_readlane_b32 %[sb], %[vB2], s84\n" \
                        "s_bitset0_b64 s[82:83], s84\n" \
                        "s_cmp_lt_u32 %[sa], 0x400000\n" \
                        "s_cbranch_scc0 LML%=\n" \
                        "v_cmpx_ge_u32 vcc, %[sa], %[vX1]\n" \
                        "v_add_u32 %[t0], %[sb], %[vlane7]\n" \
                        "v_add_u32_sdwa %[t1], %[sa], %[vlane7] dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:DWORD\n" \
                        "ds_read_u8 %[t2], %[t0]\n" \
                        "s_waitcnt lgkmcnt(0)\n" \
                        "ds_write_b8 %[t1], %[t2]\n" \
                        "s_mov_b64 exec, s[92:93]\n" \
                        "LMe%=:\n" \
                        "s_cmp_lg_u64 s[82:83], 0\n" \
                        "s_cbranch_scc1 LM%=\n" \
                        "LN%=:\n" \
                        "s_cmp_lt_i32 %[j], 0\n" \
                        "s_cbranch_scc1 LMx%=\n" \
                        "v_readlane_b32 %[sb], %[vB], %[j]\n" \
                        "v_readlane_b32 %[sa], %[vA], %[j]\n" \
                        "s_cmp_lt_u32 %[sb], 0x20000\n" \
                        "s_cbranch_scc0 LMx%=\n" \
                        "s_bitset0_b64 %[mm], %[j]\n" \
                        "v_readlane_b32 %[sb], %[vC], %[j]\n" \
                        "s_lshr_b32 %[len], %[sa], 16\n" \
                        "s_and_b32 %[sa], %[sa], 0xffff\n" \
                        "v_add_u32 %[t1], %[sa], %[vlane]\n" \
                        "v_add_u32 %[t0], %[sb], %[vlane]\n" \
                        "LMg%=:\n" \
                        "v_cmp_gt_u32 vcc, %[len], %[vlane]\n" \
                        "s_mov_b64 exec, vcc\n" \
                        "global_load_ubyte %[t2], %[t0], %[outp]\n" \
                        "s_waitcnt vmcnt(0)\n" \
                        "ds_write_b8 %[t1], %[t2]\n" \
                        "s_mov_b64 exec, s[92:93]\n" \
                        "s_cmp_gt_u32 %[len], 64\n" \
                        "s_cbranch_scc0 LF1%=\n" \
                        "s_sub_u32 %[len], %[len], 64\n" \
                        "v_add_u32 %[t0], 64, %[t0]\n" \
                        "v_add_u32 %[t1], 64, %[t1]\n" \
                        "s_branch LMg%=\n" \
                        "LF1%=:\n" \
                        "s_mov_b32 %[j], -1\n" \
                        "s_cmp_lg_u64 %[mm], 0\n" \
                        "s_cbranch_scc1 LO%=\n" \
                        "s_branch LMx%=\n" \
                        "LML%=:\n" \
                        "v_readlane_b32 s85, %[vXl], s84\n" \
                        "v_readlane_b32 s86, %[vYl], s84\n" \
                        "v_readlane_b32 s87, %[vKl], s84\n" \
                        "LMq%=:\n" \
                        "s_lshr_b32 s88, s86, 16\n" \
                        "v_add_u32 v48, s87, %[vlane32]\n" \
                        "v_cmpx_gt_i32 vcc, 32, v48\n" \
                        "v_add_u32_sdwa v49, s86, %[vlane4] dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:DWORD\n" \
                        "v_add_u32_sdwa v50, s85, %[vlane4] dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:DWORD\n" \
                        "ds_read2_b32 v[52:53], v49 offset1:1\n" \
                        "ds_read_b32 v51, v50\n" \
                        "v_max_i32 v48, 0, v48\n" \
                        "v_lshrrev_b32_e64 v48, v48, -1\n" \
                        "v_and_b32_sdwa v54, s85, %[vlane0] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:DWORD\n" \
                        "v_lshlrev_b32_e64 v54, v54, -1\n" \
                        "v_and_b32 v48, v48, v54\n" \
                        "s_waitcnt lgkmcnt(0)\n" \
                        "v_alignbit_b32 v52, v53, v52, s88\n" \
                        "v_bfi_b32 v51, v48, v52, v51\n" \
                        "ds_write_b32 v50, v51\n" \
                        "s_mov_b64 exec, s[92:93]\n" \
                        "s_cmp_lt_i32 s87, -2016\n" \
                        "s_cbranch_scc0 LMe%=\n" \
                        "s_add_u32 s87, s87, 2048\n" \
                        "s_add_u32 s85, s85, 256\n" \
                        "s_and_b32 s85, s85, 0xffff\n" \
                        "s_add_u32 s86, s86, 256\n" \
                        "s_branch LMq%=\n" \
                        "LMx%=:\n" \
                        "s_mov_b64 exec, s[92:93]\n" \
                        : [mm] "+s"(mm), [j] "=&s"(j), [sa] "=&s"(sa), [sb] "=&s"(sb), [len] "=&s"(len), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2) \
                        : [vA] "v"(vA), [vB] "v"(vB), [vC] "v"(vC), [vlane] "v"(lane), [vX] "v"(lane_hi), [vA2] "v"(vA2), [vB2] "v"(vB2), [vXl] "v"(vXl), [vYl] "v"(vYl), [vKl] "v"(vKl), [vX1] "v"(lane_sh16), [vlane7] "v"(lane_p7), [vlane4] "v"(lane_x4), [vlane32] "v"(lane_x32), [vlane0] "v"(lane0_31), [outp] "s"(out), [pm] "s"(plain_mask) \
                        : "s80", "s81", "s82", "s83", "s84", "s85", "s86", "s87", "s88", "s92", "s93", "vcc", "scc", "memory", "v48", "v49", "v50", "v51", "v52", "v53", "v54");

// bgzf_copy: CW blocks per workgroup, a wavefront each (they share nothing but the CRC tables); every wavefront has its ring, the 512
// bytes next to it where far matches are parked, and the teams' slots.  LDS addresses stay below 64 K: the copy loops do their
// address arithmetic in 16 bits.
#ifndef TCMI_COPY_CW
#define TCMI_COPY_CW 4                              // bgzf_copy: blocks (wavefronts) per workgroup: they share the CRC tables (A/B: 2, 3; 4 x 64 lanes build the tables)
#endif
constexpr int CW = TCMI_COPY_CW;
constexpr int CRC_NOPS = 12;                        // crc_ops: 1, 2, 4, .. 2048 zero bytes
struct CopyLds { uint8_t win[CWIN]; uint32_t far[FAR_WORDS]; uint2 team[8]; };
struct CopyShared {
    CopyLds w[CW];
    uint32_t t[4][256];         // t[k][v]: the CRC register after byte v and k zero bytes ("slicing by 4")
    uint32_t seg[8][16];        // seg[j][n]: the register n << 4 j, CSEG zero bytes later
};
static_assert(sizeof(CopyLds) % 16 == 0 && CW * sizeof(CopyLds) + CWIN < 65536, "16-bit LDS addresses in the copy loops");
static_assert((160 * 1024 / sizeof(CopyShared)) * CW >= 14, "at least fourteen blocks per compute unit");

// the CRC register (linear form: starts at 0, no final inversion) after the 16 bytes of v, from state c
__device__ __forceinline__ uint32_t crc16(const uint32_t (*t)[256], uint32_t c, uint4 v)
{
    auto x3 = [](uint32_t x, uint32_t y, uint32_t z) { return (uint32_t)__builtin_amdgcn_bitop3_b32(x, y, z, 0x96); };
    auto step = [&](uint32_t x) { return x3(t[3][x & 0xFFu], t[2][(x >> 8) & 0xFFu], t[1][(x >> 16) & 0xFFu]) ^ t[0][x >> 24]; };
    c = step(c ^ v.x);
    c = step(c ^ v.y);
    c = step(c ^ v.z);
    return step(c ^ v.w);
}
// a linear operator on the register given by nibble tables (tab[j][n] = op(n << 4 j)): LDS or global memory
__device__ __forceinline__ uint32_t crc_apply(const uint32_t (*tab)[16], uint32_t c)
{
    auto x3 = [](uint32_t x, uint32_t y, uint32_t z) { return (uint32_t)__builtin_amdgcn_bitop3_b32(x, y, z, 0x96); };
    return x3(x3(tab[0][c & 15u], tab[1][(c >> 4) & 15u], tab[2][(c >> 8) & 15u]), x3(tab[3][(c >> 12) & 15u], tab[4][(c >> 16) & 15u], tab[5][(c >> 20) & 15u]),
              tab[6][(c >> 24) & 15u] ^ tab[7][c >> 28]);
}
// A lane's column of a segment: CCOL = CSEG / 64 bytes (32 of the 2 KiB segments, 16 of 1 KiB ones).
constexpr int CCOL = CSEG / 64, CCOL_LOG = CCOL == 32 ? 5 : 4;
static_assert(CCOL == 32 || CCOL == 16, "the CRC's columns: 64 lanes x 16 or 32 bytes a segment");
// XOR over the lanes of (x of lane l, CCOL (63 - l) zero bytes later): a lane that starts a span of 2 s columns takes its right
// neighbour's span (CCOL s bytes) behind its own; lane 0 ends up with all of it (ops[k]: 2^k zero bytes, nibble tables in global memory)
__device__ __forceinline__ uint32_t crc_fold(const uint32_t *ops, uint32_t c)
{
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint32_t right = (uint32_t)__shfl_down((int)c, 1 << k, 64);
        c = crc_apply(reinterpret_cast<const uint32_t (*)[16]>(ops + (size_t)(CCOL_LOG + k) * 128), c) ^ right;
    }
    return c;
}
// bytes of a 16-byte piece that starts at position `at`: those in front of `from` count as zeros, those in [inv, inv + 4) are inverted
// (the block's first four: the standard's all-ones start, in the linear form)
__device__ __forceinline__ uint4 crc_masked(uint4 v, int32_t at, int32_t from, int32_t inv)
{
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t keep = 0, flip = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int32_t p = at + 4 * k + b;
            if (p >= from) keep |= 0xFFu << (8 * b);
            if (p >= from && p >= inv && p < inv + 4) flip |= 0xFFu << (8 * b);
        }
        w[k] = (w[k] & keep) ^ flip;
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// TEAMS: with the rounds of teams for batches of short tokens (files that compress less than ~12 : 1: the host picks the variant;
// both are right for any input — the lean one is 4 % faster where no batch would use teams)
// DIRECT: with the short far matches of a teams' batch finished in the batch's set-up (files that compress less than ~4 : 1: most of
// their matches are 3 - 8 bytes long and come from anywhere in the 32 KB window; at 6 : 1 few do and the lean set-up is 3 % faster)
template <bool TEAMS, bool DIRECT>
__global__ __launch_bounds__(64 * CW) __attribute__((amdgpu_waves_per_eu(4, 4))) void bgzf_copy(CopyArgs a)
{
    __shared__ __attribute__((aligned(16))) CopyShared S;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));     // (uniform, and known to be: the block's fields go to scalar registers)
    if (a.crc) {                                    // the tables of the workgroup's four wavefronts (CW * 64 = 256 lanes: an entry each)
        for (uint32_t v = threadIdx.x; v < 256u; v += 64u * CW) {      // the reflected CRC-32 table (polynomial 0xEDB88320)
            uint32_t c = v;
#pragma unroll
            for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
            S.t[0][v] = c;
        }
        for (uint32_t v = threadIdx.x; v < 128u; v += 64u * CW) {
            const uint32_t j = v >> 4, n = v & 15u;
            uint32_t m = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) m ^= a.zeros_seg[4 * j + i] & (0u - ((n >> i) & 1u));
            S.seg[j][n] = m;
        }
        __syncthreads();
        for (int k = 1; k < 4; ++k) {               // one more zero byte behind it
            for (uint32_t v = threadIdx.x; v < 256u; v += 64u * CW) { const uint32_t c = S.t[k - 1][v]; S.t[k][v] = S.t[0][c & 0xFFu] ^ (c >> 8); }
            __syncthreads();
        }
    }
    CopyLds &s_lds = S.w[wave];
    uint8_t *const s_win = s_lds.win;
    const uint32_t B = (uint32_t)reinterpret_cast<uintptr_t>(s_win);    // the ring's LDS address (the copy loops take addresses, not ring indices)
    const int blk = a.first_block + (int)blockIdx.x * CW + wave;
    if (blk >= a.n_blocks) return;
    const BlockDesc d = a.blocks[blk];
    const uint32_t ulen = d.ulen;
    uint32_t err = uni(a.status[blk]);
    const uint32_t ntok = err == ST_OK ? uni(a.n_tok[blk]) : 0u;
    const uint32_t *toks = a.tokens + d.tok;
    // The blocks' outputs follow each other in the stream without gaps, so this block's starts at any byte.  Positions in this
    // kernel count from the 16-byte boundary in front of it (`a0` bytes of the previous block come first and are never touched):
    // ring index and stream address of a byte are then equal modulo 16 and the flush can use 16-byte rows.
    const uint32_t a0 = (uint32_t)(d.uout & 15u);
    uint8_t *const out = a.out + (d.uout - a0);
    const uint32_t vend = a0 + ulen;    // the block's end
    const uint8_t *const payload = a.file + d.cin;
    uint32_t *slots = a.rec_slot + (size_t)blk * MAX_REC_PER_BLOCK;
    const uint32_t *const win32 = reinterpret_cast<const uint32_t *>(s_win);
    const uint32_t lane_hi = ((uint32_t)lane << 16) | 0xFFFFu;  // (len << 16 | anything) > lane_hi  <=>  len > lane: the copy round's lane mask from the packed operand
    // per-lane constants of TCMI_LM_ASM's two copy rounds (bytes: lane + 7, lane << 16; dwords: 4 lane, 32 lane, lane 0's 31)
    const uint32_t lane_p7 = (uint32_t)lane + 7u, lane_sh16 = (uint32_t)lane << 16, lane_x4 = (uint32_t)lane * 4u, lane_x32 = (uint32_t)lane * 32u;
    const uint32_t lane0_31 = lane == 0 ? 31u : 0u;
    // (teams of eight lanes: lane l belongs to team l / 8 and takes that team's piece l % 8)
    const uint32_t team_of = (uint32_t)lane >> 3, team_sub = (uint32_t)lane & 7u, team_sub8 = team_sub * 8u;
    const uint32_t team_base = B + (uint32_t)(CWIN + FAR_WORDS * 4), team_slot = team_base + team_of * 8u;     // s_lds.team, as LDS addresses

    uint32_t op = a0, flushed = 0;
    uint32_t next_rec = d.entry >= 0 ? a0 + (uint32_t)d.entry : 0xFFFFFFF0u;
    bool searching = d.entry == -2;     // the block's first record start is still to be found, from `search_pos` on
    uint32_t search_pos = a0;
    uint32_t first_rec = d.entry >= 0 ? (uint32_t)d.entry : 0xFFFFFFFFu;
    uint32_t rec_size = 0;              // 4 + block_size of the last record listed (0: none yet)
    uint32_t n_rec = 0;
    uint32_t next_evt = 0;
    uint32_t bad = 0;
    bool tail_unknown = false;

    // four bytes of the ring at any position
    auto ring_u32 = [&](uint32_t x) __attribute__((always_inline)) {
        const uint32_t i = (x & CWMASK) >> 2;
        return __builtin_amdgcn_alignbit(win32[(i + 1) & (CWIN / 4 - 1)], win32[i], (x & 3u) * 8u);
    };
    // Could an alignment record start at c (its first 40 bytes are in the ring)?  block_size, refID, pos, l_read_name, the variable
    // lengths against block_size, next_refID — what BAM readers that must find a record in the middle of a file test.  A wrong yes
    // is caught by the host: the chain of records through all blocks must close.
    // (`avail`: bytes of the candidate that lie in this block — at the block's end fewer than the 36 of the fixed fields; what
    // is not there is not tested)
    auto plausible = [&](uint32_t c, uint32_t avail) __attribute__((always_inline)) {
        const uint32_t bs = ring_u32(c), refid = ring_u32(c + 4), pos = ring_u32(c + 8), w2 = ring_u32(c + 12), w3 = ring_u32(c + 16);
        const uint32_t l_seq = ring_u32(c + 20), nref = ring_u32(c + 24), npos = ring_u32(c + 28);
        const uint32_t l_name = w2 & 0xFFu, n_cig = w3 & 0xFFFFu;
        const uint64_t need = 32ull + l_name + 4ull * n_cig + ((uint64_t)l_seq + 1) / 2 + l_seq;
        bool ok = avail >= 4u && bs >= 33u && bs < (1u << 24);
        if (avail >= 8u) ok = ok && refid + 1u <= a.n_ref;
        if (avail >= 12u) ok = ok && (int32_t)pos >= -1;
        if (avail >= 13u) ok = ok && l_name >= 1u;
        if (avail >= 24u) ok = ok && l_seq < (1u << 28) && need <= bs;
        if (avail >= 28u) ok = ok && nref + 1u <= a.n_ref;
        if (avail >= 32u) ok = ok && (int32_t)npos >= -1;
        return ok;
    };

    const bool do_crc = a.crc != 0;
    uint32_t crc_acc = 0;               // this lane's column of the flushed segments (linear form)
    // List the record starts whose block_size field is complete, flush the segments that are complete.  The chain of records is
    // serial (a record's start is known when its predecessor's size is), but the records of a BAM block mostly have one size: 16
    // lanes look at where the next 16 records start if they all have the size of the last one, and the chain advances over all
    // that do (at least one per step: the first candidate is a record start for sure).
    auto housekeeping = [&]() __attribute__((always_inline)) {
        while (searching && search_pos + 40u <= op) {            // 64 candidates at a time
            const uint32_t c = search_pos + (uint32_t)lane;
            const unsigned long long hit = __ballot(c + 40u <= op && c < vend && plausible(c, 40u));
            if (hit) {
                next_rec = search_pos + (uint32_t)__builtin_ctzll(hit);
                first_rec = next_rec - a0;
                searching = false;
            } else {
                search_pos = min(search_pos + 64u, op - 39u);
                if (search_pos >= vend) searching = false;
            }
        }
        while (next_rec + 4 <= op) {
            const uint32_t cand = next_rec + (uint32_t)lane * rec_size;
            const bool look = lane < 16 && (lane == 0 || rec_size != 0) && cand + 4 <= op;
            uint32_t bs = 0;
            if (look) {
                const uint32_t i = (cand & CWMASK) >> 2;
                bs = __builtin_amdgcn_alignbit(win32[(i + 1) & (CWIN / 4 - 1)], win32[i], (cand & 3u) * 8u);
            }
            const uint32_t n_look = (uint32_t)__popcll(__ballot(look));                         // (a prefix of the lanes)
            const uint32_t same = (uint32_t)__builtin_ctzll(~__ballot(look && bs + 4u == rec_size));  // leading candidates of the same size
            uint32_t n_conf;
            if (same < n_look) {
                // candidate `same` starts a record of another size (or the first one at all)
                const uint32_t ubs = (uint32_t)__builtin_amdgcn_readlane((int)bs, (int)same);
                if (__builtin_expect(ubs - 32u > (1u << 28) - 32u, 0)) { err = ST_BAD_RECORD; next_rec = 0xFFFFFFF0u; break; }
                n_conf = same + 1u;
                next_rec += same * rec_size + 4u + ubs;
                rec_size = 4u + ubs;
            } else {
                n_conf = n_look;
                next_rec += n_look * rec_size;
            }
            if (n_rec + n_conf > (uint32_t)MAX_REC_PER_BLOCK) { err = ST_BAD_RECORD; next_rec = 0xFFFFFFF0u; break; }
            if ((uint32_t)lane < n_conf) slots[n_rec + (uint32_t)lane] = cand - a0;
            n_rec += n_conf;
        }
        while (op - flushed >= CSEG) {
            const uint4 *src = reinterpret_cast<const uint4 *>(s_win + (flushed & CWMASK));
            uint4 *dst = reinterpret_cast<uint4 *>(out + flushed);
            if (flushed == 0 && a0 != 0) {                       // the block's first row: its first bytes are the previous block's
                if (lane == 0) { for (uint32_t i = a0; i < 16u; ++i) out[i] = s_win[i]; }
                else dst[lane] = src[lane];
            } else dst[lane] = src[lane];
#pragma unroll
            for (int k = 1; k < CSEG / 16 / 64; ++k) dst[k * 64 + lane] = src[k * 64 + lane];
            if (do_crc) {
                // the segment's CRC while it is in the ring: lane l takes the CCOL bytes at CCOL l (its column: the register of the column's
                // bytes so far, CSEG zero bytes later, plus these)
                uint4 p0 = src[(CCOL / 16) * lane], p1 = CCOL == 32 ? src[2 * lane + 1] : make_uint4(0u, 0u, 0u, 0u);
                if (flushed == 0) { p0 = crc_masked(p0, CCOL * lane, (int32_t)a0, (int32_t)a0); if (CCOL == 32) p1 = crc_masked(p1, 32 * lane + 16, (int32_t)a0, (int32_t)a0); }
                uint32_t cs = crc16(S.t, 0u, p0);
                if (CCOL == 32) cs = crc16(S.t, cs, p1);
                crc_acc = crc_apply(S.seg, crc_acc) ^ cs;
            }
            flushed += CSEG;
        }
        next_evt = flushed + (uint32_t)CSEG;
    };
    // a match of any kind: all lanes; with dist < len the pattern of the last `dist` bytes repeats
    auto copy_any = [&](uint32_t at, uint32_t len, uint32_t dist) __attribute__((always_inline)) {
        if (dist + a0 > at) { bad = 1; return; }                 // before the block's first byte
        if (dist > (uint32_t)CNEAR) {
            const uint8_t *src = out + (at - dist);             // flushed by this wavefront (see CNEAR)
#pragma clang loop vectorize(disable) unroll(disable)
            for (uint32_t i = (uint32_t)lane; i < len; i += 64) s_win[(at + i) & CWMASK] = src[i];
        } else if (dist >= len) {
#pragma clang loop vectorize(disable) unroll(disable)
            for (uint32_t i = (uint32_t)lane; i < len; i += 64) s_win[(at + i) & CWMASK] = s_win[(at + i - dist) & CWMASK];
        } else {
            const float inv = 1.0f / (float)dist;
#pragma clang loop vectorize(disable) unroll(disable)
            for (int i = lane; i < (int)len; i += 64) {
                int qd = (int)((float)i * inv);
                int r = i - qd * (int)dist;
                if (r < 0) r += (int)dist;
                if (r >= (int)dist) r -= (int)dist;
                s_win[(at + i) & CWMASK] = s_win[(at - dist + r) & CWMASK];
            }
        }
    };
    if (a.stamps && lane < 16) a.stamps[(size_t)blk * 16 + lane] = 0;
    TCMI_STAMP(a.stamps, blk, 0);
#ifdef TCMI_COPY_PHASES                 // (diagnostic build: where a block's cycles go — batch set-up, match loop, other matches, housekeeping)
    uint64_t ph_t = __builtin_amdgcn_s_memtime(), ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t hist[6] = {0, 0, 0, 0, 0, 0};     // plain matches of < 8, 8 - 64, 65 - 128, 129 - 192, 193 - 256, 257+ bytes
#define PH(k_) do { const uint64_t now_ = __builtin_amdgcn_s_memtime(); ph[k_] += now_ - ph_t; ph_t = now_; } while (0)
#else
#define PH(k_) do { } while (0)
#endif
    uint32_t n_match = 0, n_slow = 0, n_round = 0;
    const uint32_t n_team = 0, n_teamed = 0;
    housekeeping();
    // the tokens of the batch that starts at `base`, a token a lane: consecutive words (bgzf_symbols left them in order).
    // ONE load, of every lane, outside any branch, masked where it is used: a load under a condition makes the compiler wait for it on
    // the spot, and the batch's copy loops would start a trip to memory later (2.5 : 1: 1 035 -> 977 us).
    bool t_has = false;
    auto fetch_tokens = [&](uint32_t base) __attribute__((always_inline)) {
        const uint32_t g = base + (uint32_t)lane;
        t_has = g < ntok;
        return toks[t_has ? g : 0u];                        // (a lane without a token reads word 0 and drops it)
    };
    uint32_t t_ahead = fetch_tokens(0);         // (a batch's tokens are asked for while the batch before is copied: HBM is a microsecond away)
    bool t_ahead_has = t_has;
    for (uint32_t base = 0; base < ntok && err == ST_OK && !bad; base += 64) {
        const uint32_t t = t_ahead_has ? t_ahead : 0u;
        const bool is_lit = (t >> 31) != 0;
        const bool is_raw = !is_lit && (t & TOK_RAW);
        if (__builtin_expect(__ballot(is_raw) != 0, 0)) {
            // ---- a batch with stored bytes in it: token by token (rare: incompressible data, flush markers) --------------------
            const uint32_t nb = min(64u, ntok - base);
            for (uint32_t j = 0; j < nb && err == ST_OK && !bad; ++j) {
                const uint32_t tj = (uint32_t)__builtin_amdgcn_readlane((int)t, (int)j);
                if (tj >> 31) {
                    const uint32_t nl = TEAMS ? 1u + ((tj >> 24) & 3u) : 1u;         // (one literal, or — files of short tokens — two in one token)
                    if (op + nl > vend) { err = ST_BAD_LENGTH; break; }
                    s_win[op & CWMASK] = (uint8_t)tj;
                    if (nl > 1u) s_win[(op + 1u) & CWMASK] = (uint8_t)(tj >> 8);
                    op += nl;
                } else if (tj & TOK_RAW) {
                    uint32_t len = (tj >> 17) & 0x1FFFu;
                    const uint8_t *src = payload + (tj & 0x1FFFFu);
                    if (op + len > vend) { err = ST_BAD_LENGTH; break; }
                    while (len) {
                        const uint32_t n = min(len, (uint32_t)CSEG - (op & (CSEG - 1)));
#pragma clang loop vectorize(disable) unroll(disable)
                        for (uint32_t i = lane; i < n; i += 64) s_win[(op + i) & CWMASK] = src[i];
                        op += n; src += n; len -= n;
                        if (op >= next_evt) { housekeeping(); if (err != ST_OK) break; }
                    }
                } else {
                    const uint32_t len = tj & 511u, dist = ((tj >> 9) & 0x7FFFu) + 1u;
                    if (op + len > vend) { err = ST_BAD_LENGTH; break; }
                    copy_any(op, len, dist);
                    op += len;
                }
                if (op >= next_evt) housekeeping();
            }
            t_ahead = fetch_tokens(base + 64u); t_ahead_has = t_has;
            continue;
        }
#if TCMI_COPY_PHASES >= 2
        PH(5);
#endif
        const uint32_t mylen = is_lit ? (TEAMS ? 1u + ((t >> 24) & 3u) : 1u) : (t & 511u);       // (a literal token carries one byte, or — bgzf_symbols<1, *>, whose files get this kernel's TEAMS variants — two)
        const uint32_t dist = ((t >> 9) & 0x7FFFu) + 1u;
        const uint32_t incl = wave_scan_add(mylen);
        const uint32_t dst = op + incl - mylen;                 // where this lane's token starts
        const uint32_t batch_end = op + (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        if (batch_end > vend) { err = ST_BAD_LENGTH; break; }
        // what the copy loop needs of a match, ready in two registers: ring addresses of its destination and source, its length, and
        // whether it is one of the plain ones — source in the ring, source and destination apart by the match's length at least
        // (a round copies the whole match at once), neither range across the ring's end, and for the dword rounds of a match beyond
        // 64 bytes the source not within the ring's first four bytes.  The others (far, period shorter than the match, across the
        // end) take copy_any.
#if TCMI_COPY_PHASES >= 2
        PH(6);
#endif
        const bool is_match = !is_lit && mylen != 0;
        const uint32_t dm = dst & CWMASK, sm = (dst - dist) & CWMASK;
        const bool plain = dist <= (uint32_t)CNEAR && dist + a0 <= dst && dist >= mylen && dm + mylen <= (uint32_t)CWIN && sm + mylen <= (uint32_t)CWIN && (mylen <= 64u || sm >= 4u);
        const bool far_ok = dist > (uint32_t)CNEAR && dist + a0 <= dst && dm + mylen <= (uint32_t)CWIN;      // (its source is flushed when its turn comes: CNEAR)
        uint32_t vA = (B + dm) | (mylen << 16), vB = (B + sm) | (plain ? 0u : far_ok ? 1u << 16 : 2u << 16);     // (LDS addresses: B + ring index, below 64 K)
        const uint32_t vC = dst - dist;                         // a far match's source, as a position
        // A match that reaches back further than the ring holds reads what this wavefront flushed long ago — from HBM, a microsecond
        // away if it is fetched when the match comes up.  So the far matches of the batch whose sources are flushed already (all of
        // them, unless the batch is several KB of output long) are fetched NOW, every lane its own match's bytes, into a few
        // hundred bytes of LDS next to the ring; to the copy loop below they are plain matches whose source lies there.
#if TCMI_COPY_PHASES == 3
        PH(7);
#endif
        // Teams' batches (short tokens: data that compresses like real data, whose matches are mostly 3 - 8 bytes from anywhere in
        // the 32 KB behind): a far match of up to 8 bytes is FINISHED here — three words from the flushed stream, its bytes straight
        // to their place in the ring (exactly `len` of them: lanes write next to each other) — instead of being parked and copied by
        // a team later: 17 + 12 instructions for all of them, and the teams' rounds are left with the near matches.  (The batch is at
        // most team_bytes long: what these writes replace in the ring was flushed long ago and is further back than CNEAR.)
        const bool use_teams = TEAMS && uni(batch_end - op <= a.team_bytes ? 1u : 0u) != 0u;
        bool done = false;
        const bool far_now = is_match && far_ok && mylen <= 64u && dst - dist + mylen <= flushed;     // far, flushed, and short enough to be fetched here
        const unsigned long long far_mask = __ballot(far_now);
        if (DIRECT && use_teams && far_mask) {
            const uint32_t src = dst - dist;
            done = far_now && mylen <= 8u;
            const unsigned long long dmask = __ballot(done);
            if (dmask) {
                uint32_t w0 = 0, w1 = 0, w2 = 0;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // (this wavefront's own flush stores)
                if (done) {
                    const uint32_t *g = reinterpret_cast<const uint32_t *>(out + (src & ~3u));
                    w0 = g[0]; w1 = g[1];
                    if ((src & 3u) + mylen > 8u) w2 = g[2];
                }
                const uint32_t sh = (src & 3u) * 8u;
                const uint32_t lo = __builtin_amdgcn_alignbit(w1, w0, sh), hi = __builtin_amdgcn_alignbit(w2, w1, sh);
                uint32_t lo8, hi8;
                asm volatile(
                    "s_mov_b64 s[92:93], exec\n"
                    "s_mov_b64 exec, %[dmask]\n"
                    "v_lshrrev_b32 %[lo8], 8, %[lo]\n"
                    "v_lshrrev_b32 %[hi8], 8, %[hi]\n"
                    "ds_write_b8 %[at], %[lo]\n"
                    "ds_write_b8 %[at], %[lo8] offset:1\n"
                    "ds_write_b8_d16_hi %[at], %[lo] offset:2\n"
                    "v_cmpx_lt_u32 vcc, 3, %[len]\n"
                    "ds_write_b8_d16_hi %[at], %[lo8] offset:3\n"
                    "v_cmpx_lt_u32 vcc, 4, %[len]\n"
                    "ds_write_b8 %[at], %[hi] offset:4\n"
                    "v_cmpx_lt_u32 vcc, 5, %[len]\n"
                    "ds_write_b8 %[at], %[hi8] offset:5\n"
                    "v_cmpx_lt_u32 vcc, 6, %[len]\n"
                    "ds_write_b8_d16_hi %[at], %[hi] offset:6\n"
                    "v_cmpx_lt_u32 vcc, 7, %[len]\n"
                    "ds_write_b8_d16_hi %[at], %[hi8] offset:7\n"
                    "s_mov_b64 exec, s[92:93]\n"
                    : [lo8] "=&v"(lo8), [hi8] "=&v"(hi8)
                    : [dmask] "s"(dmask), [lo] "v"(lo), [hi] "v"(hi), [at] "v"(B + dm), [len] "v"(mylen)
                    : "s92", "s93", "vcc", "memory");
            }
        }
        {
            const uint32_t src = dst - dist;                    // (position of the source's first byte)
            const bool fetch = far_now && !done;                // (longer ones: 64 bytes an instruction in the loop)
            if (far_mask && __ballot(fetch)) {
                const uint32_t words = fetch ? (mylen + 3u) >> 2 : 0u;
                const uint32_t end_w = wave_scan_add(words);
                const bool take = fetch && end_w <= (uint32_t)FAR_WORDS;
                if (__ballot(take)) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (this wavefront's own flush stores)
                    const uint32_t *g = reinterpret_cast<const uint32_t *>(out + (src & ~3u));
                    const uint32_t sh = (src & 3u) * 8u;
                    uint32_t *park = s_lds.far + (end_w - words);
                    const uint32_t n = take ? words : 0u;
                    for (uint32_t k = 0; __ballot(k < n); k += 8) {           // eight words a turn, nine loads in flight: a turn is a trip to HBM
                        uint32_t w[9];                                      // (32 bytes and less — most far matches — in one)
#pragma unroll
                        for (int i = 0; i < 9; ++i) w[i] = k + i <= n && k < n ? g[k + i] : 0u;
#pragma unroll
                        for (int i = 0; i < 8; ++i)
                            if (k + i < n) park[k + i] = __builtin_amdgcn_alignbit(w[i + 1], w[i], sh);
                    }
                    if (take) vB = B + (uint32_t)CWIN + 4u * (end_w - words);
                }
            }
        }
        // Matches whose source lies wholly in front of the first match still to be copied do not depend on it: up to eight of them are
        // copied at a time, by a TEAM of eight lanes each (eight bytes a lane and step).  `srcend`: the position behind a match's source
        // (a parked one's lies in flushed output: 0, always ready; one that is not plain never joins a team).
        // (Worth it where tokens are short: a round of teams costs about three single matches' instructions, and in a batch of long
        // matches — the same record 289 bytes back, say — only two or three matches at a time are independent.)
#if TCMI_COPY_PHASES == 2
        PH(7);
#elif TCMI_COPY_PHASES == 3
        PH(3);
#endif
        const bool teamable = is_match && !done && (vB >> 16) == 0u;
        const unsigned long long plain_mask = __ballot(teamable);  // (plain matches, parked far ones included)
        // TCMI_LM_ASM's operands of a plain match.  Up to 64 bytes, a byte a lane: (len - 1) << 16 | (destination - 7) & 0xffff and
        // source - 7 (lane + 7 is added to both).  Longer ones, an ALIGNED destination dword a lane (LDS takes unaligned words at a
        // fifth of the rate): the first dword's address | 8 (destination & 3) << 16; the aligned address of the source dword that
        // holds the first dword's byte 0 | 8 (its place in it) << 16; and 32 - 8 (bytes from the first dword's start to the match's
        // end): + 32 lane = how far a lane's mask of bytes is to be shifted down (< 32: the lane has bytes at all).
        const uint32_t vA2 = ((mylen - 1u) << 16) | ((B + dm - 7u) & 0xFFFFu), vB2 = vB - 7u;
        const uint32_t hoff = dm & 3u, s0 = sm - hoff;
        const uint32_t vXl = ((B + dm) & ~3u) | (hoff * 8u) << 16, vYl = ((B + s0) & 0xFFFCu) | ((s0 & 3u) * 8u) << 16, vKl = 32u - 8u * (hoff + mylen);
        const uint32_t srcend = teamable ? (vB >= B + (uint32_t)CWIN ? 0u : dst - dist + mylen) : 0xFFFFFFFFu;
        const unsigned long long team_mask = plain_mask;
        uint32_t t_cur = 0;
        // (asked for HERE, behind the batch's set-up and its waits for earlier loads, in front of the copy loops: the load is under
        //  way while the batch is copied)
        t_ahead = fetch_tokens(base + 64u); t_ahead_has = t_has;
#ifdef TCMI_COPY_PHASES
        hist[0] += __popcll(__ballot(teamable && mylen < 8u)); hist[1] += __popcll(__ballot(teamable && mylen >= 8u && mylen <= 64u));
        hist[2] += __popcll(__ballot(teamable && mylen > 64u && mylen <= 128u)); hist[3] += __popcll(__ballot(teamable && mylen > 128u && mylen <= 192u));
        hist[4] += __popcll(__ballot(teamable && mylen > 192u && mylen <= 256u)); hist[5] += __popcll(__ballot(teamable && mylen > 256u));
#endif
        PH(0);
        while (t_cur < 64u) {
            // the tokens [t_cur, t_stop) start in front of the next housekeeping stop: their literals at once, their matches in order
            const unsigned long long from = ~0ull << t_cur;
            const unsigned long long ge = __ballot(dst >= next_evt) & from;
            const uint32_t t_stop = ge ? (uint32_t)__builtin_ctzll(ge) : 64u;
            const unsigned long long rng = t_stop < 64u ? from & ~(~0ull << t_stop) : from;
            const bool mine = (rng >> lane) & 1ull;
            if (mine && is_lit) {
                s_win[dm] = (uint8_t)t;
                if (TEAMS && (t & TOK_LIT2)) s_win[(dm + 1u) & CWMASK] = (uint8_t)(t >> 8);
            }
            unsigned long long mm = __ballot(mine && is_match && !done);
            n_match += (uint32_t)__popcll(mm);
            while (mm) {
                if (use_teams) {
                    // Rounds of teams, hand-scheduled (about 50 instructions a round + 10 per further 64 bytes of the longest match; the
                    // compiler's version of the same took ~90): r = the matches whose source ends in front of F, where the first match
                    // still to be copied starts (+ that one itself, if it is plain: its steps of 64 bytes come in order); the first eight
                    // of them leave {vA, vB} in a slot each, every lane reads its team's slot; a match of up to 8 bytes is copied byte by
                    // byte (lane s of the team: byte s), a longer one in 8-byte pieces at min(8 s + 64 k, len - 8).  Leaves when fewer
                    // than two matches are ready (the single-match loop below takes the first one).
                    uint32_t f_, F_, n_;
                    asm volatile(
                        "s_mov_b64 s[92:93], exec\n"
                        "TL%=:\n"
                        "s_ff1_i32_b64 %[f], %[mm]\n"
                        "v_readlane_b32 %[F], %[vdst], %[f]\n"
                        "s_lshl_b64 s[84:85], 1, %[f]\n"
                        "s_and_b64 s[84:85], s[84:85], %[tmask]\n"
                        "v_cmp_ge_u32 vcc, %[F], %[vsrcend]\n"
                        "s_or_b64 s[80:81], vcc, s[84:85]\n"
                        "s_and_b64 s[80:81], s[80:81], %[mm]\n"
                        "s_bcnt1_i32_b64 %[n], s[80:81]\n"
                        "s_cmp_lt_u32 %[n], 2\n"
                        "s_cbranch_scc1 TX%=\n"
                        "v_mbcnt_lo_u32_b32 v48, s80, 0\n"
                        "v_mbcnt_hi_u32_b32 v48, s81, v48\n"
                        "v_cmp_gt_u32 vcc, 8, v48\n"
                        "s_and_b64 s[82:83], vcc, s[80:81]\n"
                        "s_mov_b64 exec, s[82:83]\n"
                        "v_lshl_add_u32 v49, v48, 3, %[sK]\n"
                        "ds_write2_b32 v49, %[vA], %[vB] offset1:1\n"
                        "s_mov_b64 exec, s[92:93]\n"
                        "s_bcnt1_i32_b64 %[n], s[82:83]\n"
                        "s_andn2_b64 %[mm], %[mm], s[82:83]\n"
                        "ds_read2_b32 v[56:57], %[vslot] offset1:1\n"
                        "s_waitcnt lgkmcnt(0)\n"
                        "v_lshrrev_b32 v58, 16, v56\n"
                        "v_and_b32 v59, 0xffff, v56\n"
                        "v_cmp_gt_u32 vcc, %[n], %[vT]\n"
                        "v_cmp_gt_u32 s[84:85], 9, v58\n"
                        "v_cmp_gt_u32 s[86:87], v58, %[vsub]\n"
                        "v_cmp_gt_u32 s[88:89], v58, %[vsub8]\n"
                        "s_and_b64 s[86:87], s[86:87], s[84:85]\n"
                        "s_andn2_b64 s[88:89], s[88:89], s[84:85]\n"
                        "s_and_b64 s[86:87], s[86:87], vcc\n"
                        "s_and_b64 s[88:89], s[88:89], vcc\n"
                        "s_mov_b64 exec, s[86:87]\n"
                        "v_add_u32 v60, v57, %[vsub]\n"
                        "v_add_u32 v61, v59, %[vsub]\n"
                        "ds_read_u8 v62, v60\n"
                        "s_mov_b64 exec, s[88:89]\n"
                        "v_subrev_u32 v50, 8, v58\n"
                        "v_min_u32 v51, v50, %[vsub8]\n"
                        "v_add_u32 v52, v57, v51\n"
                        "v_add_u32 v53, v59, v51\n"
                        "ds_read_b64 v[54:55], v52\n"
                        "s_waitcnt lgkmcnt(0)\n"
                        "ds_write_b64 v53, v[54:55]\n"
                        "s_mov_b64 exec, s[86:87]\n"
                        "ds_write_b8 v61, v62\n"
                        "s_mov_b64 exec, s[88:89]\n"
                        "v_mov_b32 v60, %[vsub8]\n"
                        "TW%=:\n"
                        "v_add_u32 v60, 64, v60\n"
                        "v_cmp_gt_u32 vcc, v58, v60\n"
                        "s_and_b64 exec, exec, vcc\n"
                        "s_cbranch_scc0 TE%=\n"
                        "v_min_u32 v51, v50, v60\n"
                        "v_add_u32 v52, v57, v51\n"
                        "v_add_u32 v53, v59, v51\n"
                        "ds_read_b64 v[54:55], v52\n"
                        "s_waitcnt lgkmcnt(0)\n"
                        "ds_write_b64 v53, v[54:55]\n"
                        "s_branch TW%=\n"
                        "TE%=:\n"
                        "s_mov_b64 exec, s[92:93]\n"
                        "s_cmp_lg_u64 %[mm], 0\n"
                        "s_cbranch_scc1 TL%=\n"
                        "TX%=:\n"
                        "s_mov_b64 exec, s[92:93]\n"
                        : [mm] "+s"(mm), [f] "=&s"(f_), [F] "=&s"(F_), [n] "=&s"(n_)
                        : [vA] "v"(vA), [vB] "v"(vB), [vdst] "v"(dst), [vsrcend] "v"(srcend), [tmask] "s"(team_mask), [vT] "v"(team_of), [vsub] "v"(team_sub),
                          [vsub8] "v"(team_sub8), [vslot] "v"(team_slot), [sK] "s"(team_base)
                        : "s80", "s81", "s82", "s83", "s84", "s85", "s86", "s87", "s88", "s89", "s92", "s93", "vcc", "scc", "memory", "v48", "v49", "v50", "v51", "v52",
                          "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61", "v62");
                    if (!mm) break;
                }
                // the matches of the stretch, one after the other (TCMI_LM_ASM), until one comes up that C++ copies: j says which (-1: none
                // left).  (With teams: one.)
                int j;
                {
                    uint32_t sa, sb, len, t0, t1, t2;
                    // (with teams: this match only — the loop is handed a set of one)
                    const unsigned long long rest = use_teams ? mm & (mm - 1ull) : 0ull;
                    mm ^= rest;
                    PH(1);
                    TCMI_LM_ASM()
                    PH(2);
                    mm |= rest;
                }
                if (j < 0) { if (use_teams) continue; break; }
                mm &= ~(1ull << j);
                copy_any((uint32_t)__builtin_amdgcn_readlane((int)dst, j), (uint32_t)__builtin_amdgcn_readlane((int)mylen, j),
                         (uint32_t)__builtin_amdgcn_readlane((int)dist, j));
                ++n_slow;
                PH(3);
            }
            op = t_stop < 64u ? (uint32_t)__builtin_amdgcn_readlane((int)dst, (int)t_stop) : batch_end;
            t_cur = t_stop;
            ++n_round;
            PH(1);
            if (op >= next_evt) { housekeeping(); if (err != ST_OK) break; }
            PH(4);
            if (bad) break;
        }
    }
    if (bad && err == ST_OK) err = ST_BAD_STREAM;
    if (err == ST_OK && op != vend) err = ST_BAD_LENGTH;
    if (err == ST_OK) {
        housekeeping();
        while (searching && search_pos + 4u <= vend) {           // the block's last 39 bytes: what there is of a record's fixed fields
            const uint32_t c = search_pos + (uint32_t)lane;
            const unsigned long long hit = __ballot(c + 4u <= vend && plausible(c, vend - c));
            if (hit) {
                next_rec = search_pos + (uint32_t)__builtin_ctzll(hit);
                first_rec = next_rec - a0;
                searching = false;
                housekeeping();                                 // (its chain, as far as the block goes)
            } else search_pos += 64u;
        }
        // a record that starts within the block's last three bytes: its start is listed, its size is read from the stream later
        if (next_rec < vend && next_rec + 4 > vend) {
            if (n_rec < (uint32_t)MAX_REC_PER_BLOCK) { if (lane == 0) slots[n_rec] = next_rec - a0; ++n_rec; tail_unknown = true; }
            else err = ST_BAD_RECORD;
        }
        for (uint32_t i = max(flushed, a0) + (uint32_t)lane; i < op; i += 64) out[i] = s_win[i & CWMASK];
        if (do_crc) {
            // ---- the block's CRC-32 against its trailer.  In the linear form crc(A || B) = later(crc(A), |B|) ^ crc(B) and zero bytes in
            // front of a message leave the register at zero: the columns of the flushed segments are joined across the lanes, moved
            // past the tail, and the tail — what lies in the ring behind the last whole segment, cut into CCOL-byte pieces from its END,
            // lane l the piece that ends CCOL (63 - l) bytes in front of the block's end — is joined the same way.
            const uint8_t *e = a.file + d.cin + d.clen;         // the block's trailer: CRC32, ISIZE (little endian)
            const uint32_t want = (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16) | ((uint32_t)e[3] << 24);
            uint32_t got;
            if (ulen < 128u) {                                  // (short blocks — the end-of-file marker's is empty — byte by byte)
                uint32_t t = 0xFFFFFFFFu;
                for (uint32_t i = 0; i < ulen; ++i) t = S.t[0][(t ^ s_win[(a0 + i) & CWMASK]) & 0xFFu] ^ (t >> 8);
                got = ~t;
            } else {
                const int32_t from = (int32_t)max(flushed, a0);
                const int32_t ps = (int32_t)vend - CCOL * (64 - lane);                  // where this lane's piece of the tail starts
                uint32_t tl = 0;
                if (ps + CCOL > from) {
                    const uint4 q0 = make_uint4(ring_u32((uint32_t)ps), ring_u32((uint32_t)ps + 4u), ring_u32((uint32_t)ps + 8u), ring_u32((uint32_t)ps + 12u));
                    tl = crc16(S.t, 0u, crc_masked(q0, ps, from, (int32_t)a0));
                    if (CCOL == 32) {
                        const uint4 q1 = make_uint4(ring_u32((uint32_t)ps + 16u), ring_u32((uint32_t)ps + 20u), ring_u32((uint32_t)ps + 24u), ring_u32((uint32_t)ps + 28u));
                        tl = crc16(S.t, tl, crc_masked(q1, ps + 16, from, (int32_t)a0));
                    }
                }
                uint32_t full = uni(crc_fold(a.crc_ops, crc_acc));
                const uint32_t tail_len = vend - flushed;       // < CSEG
                for (int k = 0; k < 11; ++k)
                    if ((tail_len >> k) & 1u) full = crc_apply(reinterpret_cast<const uint32_t (*)[16]>(a.crc_ops + (size_t)k * 128), full);
                got = ~(full ^ uni(crc_fold(a.crc_ops, tl)));
            }
            if (got != want) err = ST_BAD_CRC;
        }
    }
    if (lane == 0) {
        a.status[blk] = err;
        a.n_rec[blk] = n_rec;
        a.first_rec[blk] = first_rec;
        a.overshoot[blk] = tail_unknown ? 0x7FFFFFFF : first_rec != 0xFFFFFFFFu && next_rec < 0xFFFFFFF0u ? (int32_t)(next_rec - vend) : 0;
    }
    if (a.stamps && lane == 0) {
        uint64_t *st = a.stamps + (size_t)blk * 16;
#ifdef TCMI_COPY_PHASES
        for (int k = 0; k < 5; ++k) st[10 + k] = ph[k];
#if TCMI_COPY_PHASES >= 2
        st[2] = ph[5]; st[3] = ph[6]; st[15] = ph[7];
#else
        st[2] = hist[0] | (uint64_t)hist[1] << 32; st[3] = hist[2] | (uint64_t)hist[3] << 32; st[15] = hist[4] | (uint64_t)hist[5] << 32;
#endif
#endif
        st[1] = __builtin_amdgcn_s_memtime(); st[4] = n_slow; st[5] = n_match; st[6] = n_round; st[7] = ntok; st[8] = n_team; st[9] = n_teamed;
    }
}

// the CRC's operators: "append n zero bytes" is linear on the register — a 32 x 32 matrix over GF(2), built zlib's crc32_combine way
// (one zero bit, squared up).  ops[k][j][n]: the register n << 4 j, 2^k zero bytes later; zeros_seg[i]: bit i, CSEG zero bytes later.
struct CrcTables { uint32_t ops[CRC_NOPS][8][16]; uint32_t zeros_seg[32]; };
static const CrcTables &crc_tables()
{
    static const CrcTables T = [] {
        CrcTables t;
        auto times = [](const uint32_t *mat, uint32_t vec) { uint32_t r = 0; for (int i = 0; vec; vec >>= 1, ++i) if (vec & 1u) r ^= mat[i]; return r; };
        uint32_t a[32], b[32];
        a[0] = 0xEDB88320u;                                     // one zero BIT
        for (int i = 1; i < 32; ++i) a[i] = 1u << (i - 1);
        uint32_t *cur = a, *nxt = b;
        for (int bits = 1; bits <= 8 * 2048; bits <<= 1) {      // `cur` appends `bits` zero bits
            for (int k = 0; k < CRC_NOPS; ++k)
                if (bits == 8 << k)
                    for (int j = 0; j < 8; ++j)
                        for (uint32_t n = 0; n < 16; ++n) t.ops[k][j][n] = times(cur, n << (4 * j));
            if (bits == 8 * CSEG) std::memcpy(t.zeros_seg, cur, sizeof t.zeros_seg);
            for (int i = 0; i < 32; ++i) nxt[i] = times(cur, cur[i]);
            std::swap(cur, nxt);
        }
        return t;
    }();
    return T;
}
// ... in device memory, once per device
static const uint32_t *crc_ops_on_device(tcmi_ctx *ctx)
{
    static std::mutex mu;
    static std::vector<std::pair<int, uint32_t *>> per_device;
    std::lock_guard<std::mutex> lk(mu);
    for (auto &e : per_device) if (e.first == ctx->device) return e.second;
    uint32_t *d = nullptr;
    if (hipMalloc((void **)&d, sizeof(CrcTables::ops)) != hipSuccess) return nullptr;
    if (hipMemcpy(d, crc_tables().ops, sizeof(CrcTables::ops), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return nullptr; }
    per_device.emplace_back(ctx->device, d);
    return d;
}

} // namespace

// Picks the variant and launches it.  bgzf_symbols<1, *> — payloads beyond 4 KB — puts two literals into one token, and only the TEAMS
// variants read those: so every file of large payloads takes a TEAMS variant, whatever its compression ratio says.
int tcmi_bgzf_copy_launch(tcmi_ctx *ctx, const tcmi_bgzf_decode_args &g, size_t b_first, size_t nb, uint64_t *stamps, bool report, bool two_literals)
{
    CopyArgs ca;
    ca.file = g.d_file; ca.blocks = static_cast<const BlockDesc *>(g.d_desc); ca.tokens = g.d_tok - g.tok_base; ca.n_tok = g.d_ntok; ca.out = g.d_out; ca.rec_slot = g.d_slot;
    ca.n_rec = g.d_nrec; ca.overshoot = g.d_over; ca.first_rec = g.d_first; ca.status = g.d_stat; ca.n_blocks = (int32_t)(b_first + nb); ca.first_block = (int32_t)b_first; ca.n_ref = g.n_ref;
    ca.stamps = stamps;
    ca.team_bytes = (uint32_t)TEAM_BATCH_BYTES;
    ca.crc = g.verify_crc ? 1u : 0u;
    ca.crc_ops = nullptr;
    if (ca.crc) {
        ca.crc_ops = crc_ops_on_device(ctx);
        if (!ca.crc_ops) return tcmi_fail(ctx, TCMI_E_NOMEM, "device memory for the CRC operators");
        std::memcpy(ca.zeros_seg, crc_tables().zeros_seg, sizeof ca.zeros_seg);
    }
    if (report) {                               // (diagnostic) how many blocks a compute unit really holds
        int occ = 0;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, reinterpret_cast<const void *>(bgzf_copy<false, false>), 64 * CW, 0);
        std::fprintf(stderr, "[tcmi inflate] bgzf_copy: %d per CU\n", occ * CW);
    }
    const unsigned copy_grid = (unsigned)((nb + CW - 1) / CW);
    tcmi_prof_begin(ctx, TCMI_K_INFLATE_COPY);
    if (g.short_tokens >= 2) hipLaunchKernelGGL((bgzf_copy<true, true>), dim3(copy_grid), dim3(64 * CW), 0, ctx->stream, ca);
    else if (g.short_tokens || two_literals) hipLaunchKernelGGL((bgzf_copy<true, false>), dim3(copy_grid), dim3(64 * CW), 0, ctx->stream, ca);
    else hipLaunchKernelGGL((bgzf_copy<false, false>), dim3(copy_grid), dim3(64 * CW), 0, ctx->stream, ca);
    tcmi_prof_end(ctx, TCMI_K_INFLATE_COPY);
    TCMI_HIP(ctx, hipGetLastError());
    return TCMI_OK;
}

int tcmi_bgzf_decode_launch(tcmi_ctx *ctx, const tcmi_bgzf_decode_args &g)
{
    const size_t nb_all = g.n_blocks;
    const size_t b_first = std::min(g.first_block, nb_all), nb = std::min(g.count, nb_all - b_first);       // this launch's blocks
    if (nb == 0) return TCMI_OK;
    static const char *stamp_path = std::getenv("TCMI_INFLATE_STAMPS");      // diagnostic: phase clocks of both kernels, per block
    uint64_t *d_stamps = nullptr;
    if (stamp_path && nb == nb_all) TCMI_HIP(ctx, hipMalloc((void **)&d_stamps, nb * 16 * 8 * 2));       // (whole-file launches only)
    if (ctx->ev_before_sym) { TCMI_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_before_sym, 0)); ctx->ev_before_sym = nullptr; }      // (sub-ranges of a split step: skewed starts)
    bool two_literals = false;
    if (int rc = tcmi_bgzf_symbols_launch(ctx, g, b_first, nb, d_stamps, stamp_path != nullptr, &two_literals)) return rc;
    if (ctx->after_sym) {
        if (ctx->ev_after_sym) (void)hipEventRecord(ctx->ev_after_sym, ctx->stream);
        auto fn = std::move(ctx->after_sym);
        ctx->after_sym = nullptr;
        fn();
    }
    if (int rc = tcmi_bgzf_copy_launch(ctx, g, b_first, nb, d_stamps ? d_stamps + nb * 16 : nullptr, stamp_path != nullptr, two_literals)) return rc;
    if (d_stamps) {
        std::vector<uint64_t> h(nb * 32);
        TCMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
        TCMI_HIP(ctx, hipMemcpy(h.data(), d_stamps, h.size() * 8, hipMemcpyDeviceToHost));
        (void)hipFree(d_stamps);
        if (FILE *fp = std::fopen(stamp_path, "wb")) { std::fwrite(h.data(), 8, h.size(), fp); std::fclose(fp); }
    }
    return TCMI_OK;
}
