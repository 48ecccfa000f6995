// pack_one_sync.h — DEVICE: the one-sync packer's kernels (tcmi_pack_fused_enqueue; pk_pack and pk_report are pack_device.hip's):
// pk_prefix, pk_index, pk_place / pk_place_bq.  pack_device.hip includes it once, inside its unnamed namespace, behind classify_view and
// pack_bits.h.
// ---- a device-decoded stream -> the packed read set, without a host round trip and without a scan kernel -------------------------
// What rec_scan + the host's chain check + rec_compact + pk_classify + pk_scan + pk_scatter + pk_planes do in seven steps with three
// host round trips, as TWO kernels with none, one workgroup per BGZF block each:
//   pk_index   the records that start in the block (bgzf_copy listed them) get their place in the dense record index — the block's
//              base is the sum of the record counts of the blocks in front of it, which every workgroup adds up for itself (a few
//              thousand 4-byte words from L2: no scan kernel, nobody waits for anybody) —, are classified (classify_view, as
//              pk_classify), and leave 16 bytes each for pk_place; the block leaves its aggregate: kept reads, plane words, and the
//              record chain's transfer function across it
//   pk_place   adds up the aggregates in front of its block the same way, checks that the chain of records arrives at its block
//              where its first record starts (what the host checks block by block on the other path), and writes the kept reads'
//              entries and their bit planes (pk_scatter's and pk_planes' work) at their final places
// A first version did all of this in ONE kernel with a decoupled look-back between the workgroups (Merrill & Garland's single-pass
// scan); alone on the GPU it took 96 us, but a workgroup that waits for its predecessors holds registers and LDS that the kernels
// of other streams want: with eight contexts the pipeline lost 8 %, and with eight hardware queues it collapsed (16 M positions/s).
// Nothing here waits for another workgroup.
// The record chain across block boundaries as a function of "offset in this block at which a record must start": identity (a
// header-only block), subtract the block's length (no record starts in it), a constant (the block's last record runs that far into
// the next).
enum { CH_ID = 0, CH_SUB = 1, CH_CONST = 2 };
constexpr long long CH_BIAS = 1ll << 44;
__device__ inline unsigned long long ch_pack(int kind, long long v) { return ((unsigned long long)kind << 56) | (unsigned long long)(v + CH_BIAS); }
__device__ inline int ch_kind(unsigned long long p) { return (int)((p >> 56) & 3u); }
__device__ inline long long ch_val(unsigned long long p) { return (long long)(p & ((1ull << 56) - 1ull)) - CH_BIAS; }

struct FusedArgs {
    const uint8_t *stream;
    uint64_t stream_len;
    const BlockDesc *blocks;
    const uint32_t *rec_slot;       // [n_blocks][MAX_REC_PER_BLOCK] (bgzf_copy)
    const uint32_t *n_rec;          // [n_blocks]
    const uint32_t *first;          // [n_blocks] offset of the first record start the block found in itself (0xFFFFFFFF: none)
    const int32_t *over;            // [n_blocks] bytes the block's last record runs into the next blocks (0x7FFFFFFF: read its size here)
    const uint32_t *stat;           // [n_blocks] ST_*
    int32_t n_blocks, n_own, ranged;
    uint2 *agg;                     // [n_blocks] pk_index -> pk_place: {kept reads, plane words} of the block
    unsigned long long *fn;         // [n_blocks] ... the chain's transfer function across the block (ch_pack)
    uint32_t *rec_base;             // [n_blocks] ... index of the block's first record
    // files of very many blocks (every workgroup adding up everything in front of it is quadratic): exclusive prefix sums made by
    // pk_prefix between the kernels — records in front of a block (for pk_index), kept reads and plane words (for pk_place); else null
    const unsigned long long *pre_rec, *pre_k, *pre_w;
    uint4 *rrec;                    // [rec_cap] ... per record {word, where SEQ lies (2 words), pos}
    uint64_t *rec_off;              // out [rec_cap]: dense record offsets
    uint32_t rec_cap;
    uint32_t *c_idx; int32_t *c_pos; uint32_t *c_info; uint32_t *c_woff; uint2 *c_seq;     // out [rec_cap]: the kept reads, compacted
    uint32_t *gen_idx;              // out [rec_cap]: reads left to tally_stream_kernel
    PackOut o;                      // plane stream + events (caps inside)
    tcmi_filter_words flt;          // the context's read filter: two uniform words
    unsigned long long *blk_alg;    // out [n_blocks]: algorithmic bytes | longest span << 48
    int32_t *blk_end;               // out [n_blocks]: max end
    PackTotals *tot;
    uint32_t *drop;                 // pk_place_bq: the drop plane [word_cap / 2] and the base-quality floor (behind everything else: the
    uint32_t min_bq;                // other kernels' argument offsets stay)
    PrimerTab pt;                   // pk_place_bq: the primer table (all zero: none) and the mate join's clip (null: off), appended likewise
};

// the sum of v[0 .. n) over the workgroup (every lane gets it); s4: LDS [PB / 64]
__device__ inline unsigned long long block_sum_u32(const uint32_t *v, int n, unsigned long long *s4)
{
    unsigned long long acc = 0;
    for (int i = threadIdx.x; i < n; i += PB) acc += v[i];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += (unsigned long long)__shfl_xor((long long)acc, d, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = acc;
    __syncthreads();
    unsigned long long t = 0;
#pragma unroll
    for (int w = 0; w < PB / 64; ++w) t += s4[w];
    __syncthreads();
    return t;
}

// exclusive prefix sums of v[i * stride] over i < n (entries from n_lim on count as nothing), one workgroup: out[i], out[n] = the total
__global__ __launch_bounds__(1024) void pk_prefix(const uint32_t *v, int stride, int n, int n_lim, unsigned long long *out)
{
    __shared__ unsigned long long s_w[16];
    __shared__ unsigned long long s_run;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_run = 0;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += 1024) {
        const int i = i0 + tid;
        const unsigned long long x = i < n && i < n_lim ? v[(size_t)i * (size_t)stride] : 0ull;
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
        if (i < n) out[i] = before + incl - x;
        __syncthreads();
        if (tid == 1023) s_run = before + incl;
        __syncthreads();
    }
    if (tid == 0) out[n] = s_run;
}

__global__ __launch_bounds__(PB) void pk_index(FusedArgs a)
{
    __shared__ uint2 s_w[PB / 64];
    __shared__ unsigned long long s_alg[PB / 64];
    __shared__ int32_t s_end[PB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = (int)blockIdx.x;
    const BlockDesc d = a.blocks[b];
    const bool mine = b < a.n_own;                                  // (a block taken along for the tail of the last record: its records are not ours)
    const uint32_t n = mine ? a.n_rec[b] : 0u;
    const uint32_t *slots = a.rec_slot + (size_t)b * MAX_REC_PER_BLOCK;
    const uint32_t st = a.stat[b];
    const uint32_t first = mine ? a.first[b] : 0xFFFFFFFFu;
    int32_t over = mine ? a.over[b] : 0;
    if (tid == 0 && st != ST_OK) atomicOr(&a.tot->flags, PKF_STAT);
    // the block's first record's index: the records of the blocks in front of it (all of them ours: b < n_own, or n = 0)
    const unsigned long long base = a.pre_rec ? a.pre_rec[b] : block_sum_u32(a.n_rec, min(b, a.n_own), s_alg);
    if (tid == 0) a.rec_base[b] = (uint32_t)min(base, (unsigned long long)0xFFFFFFFFu);
    const bool room = base + n <= a.rec_cap;
    if (!room && tid == 0) atomicOr(&a.tot->flags, PKF_REC_OVF);
    unsigned long long my_alg = 0;
    int32_t my_end = 0;
    uint32_t my_len = 0, tot_k = 0, tot_w = 0;
    for (uint32_t t0 = 0; t0 < n; t0 += PB) {
        const uint32_t t = t0 + (uint32_t)tid;
        uint32_t word = 0, nwords = 0;
        if (t < n) {
            const uint64_t roff = d.uout + slots[t];
            const uint8_t *rec = a.stream + roff;
            ReadView v = view_rec(rec);
            // (a record that claims to end behind the stream: nothing of it is followed — the chain check will refuse the file)
            if (roff + 4ull + ld_u32(rec) > a.stream_len) { v.bad = true; v.broken = true; v.n_cigar = 0; }
            filter_view(v, a.flt, a.tot);
            const Classified c = classify_view(v, 1, v.tid == 0 ? 0 : -1, 0x7FFFFFFF, false, rec, true, a.tot);
            word = c.word; nwords = c.nwords;
            my_alg += c.alg; my_end = max(my_end, c.end); my_len = max(my_len, c.len);
            if (room) {
                const uint64_t ig = base + t;
                const unsigned long long so = (unsigned long long)(v.seq - a.stream);
                a.rec_off[ig] = roff;
                a.rrec[ig] = make_uint4(word, (uint32_t)so, ((uint32_t)(so >> 32) & 0xFFu) | ((uint32_t)min(v.l_seq, 0xFFFFFF) << 8), (uint32_t)v.pos);
                if (c.longread) a.gen_idx[atomicAdd(&a.tot->n_gen, 1u)] = (uint32_t)ig;
            }
        }
        const uint2 incl = block_scan2(make_uint2(word ? 1u : 0u, nwords), s_w);
        __syncthreads();
        if (tid == PB - 1) s_w[0] = incl;
        __syncthreads();
        tot_k += s_w[0].x; tot_w += s_w[0].y;
        __syncthreads();
    }
    // (the twin of the fold that ends pk_classify: one shared function changes this kernel's code)
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) {
        my_alg += (unsigned long long)__shfl_xor((long long)my_alg, dd, 64);
        my_end = max(my_end, __shfl_xor(my_end, dd, 64));
        my_len = max(my_len, (uint32_t)__shfl_xor((int)my_len, dd, 64));
    }
    if (lane == 0) { s_alg[wave] = my_alg | ((unsigned long long)my_len << 48); s_end[wave] = my_end; }
    __syncthreads();
    if (tid == 0) {
        unsigned long long al = 0, ml = 0;
        int32_t e = 0;
        for (int w = 0; w < PB / 64; ++w) { al += s_alg[w] & 0xFFFFFFFFFFFFull; ml = max(ml, s_alg[w] >> 48); e = max(e, s_end[w]); }
        a.blk_alg[b] = al | (ml << 48);
        a.blk_end[b] = e;
        a.agg[b] = make_uint2(tot_k, tot_w);
        if (mine && over == 0x7FFFFFFF && n) {                      // the last record's size field straddles the block's end: read it from the stream
            const uint32_t at = slots[n - 1];
            const uint32_t bs = ld_u32(a.stream + d.uout + at);
            over = bs - 32u > (1u << 28) - 32u ? -1 : (int32_t)(at + 4u + bs - d.ulen);
        }
        unsigned long long fn;
        if (!mine || d.entry == -1) fn = ch_pack(CH_ID, 0);
        else if (first != 0xFFFFFFFFu) fn = ch_pack(CH_CONST, over);
        else if (d.entry >= 0) fn = ch_pack(CH_CONST, (long long)d.entry - (long long)d.ulen);
        else fn = ch_pack(CH_SUB, d.ulen);
        a.fn[b] = fn;
    }
}

// BQ (pk_place_bq): as planes_body<true> — the floor a.min_bq (0: none) and the primer table a.pt, looked up by every kept read's lane
template <bool BQ>
__device__ __forceinline__ void place_body(const FusedArgs a)
{
    [[maybe_unused]] __shared__ uint32_t s_mask[BQ ? PB : 1];
    [[maybe_unused]] __shared__ int32_t s_tab[BQ ? 3 * PT_LDS : 1];
    __shared__ uint2 s_w[PB / 64];
    __shared__ unsigned long long s_sum[2 * (PB / 64)];
    __shared__ uint32_t s_info[PB], s_word[PB];
    __shared__ int32_t s_pos[PB];
    __shared__ uint2 s_seq[PB];
    __shared__ uint16_t s_owner[PL_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = (int)blockIdx.x;
    const BlockDesc d = a.blocks[b];
    const bool mine = b < a.n_own;
    const uint32_t n = mine ? a.n_rec[b] : 0u;
    const uint32_t st = a.stat[b];
    // ---- the kept reads and words in front of this block: every workgroup adds the aggregates up for itself -------------------------
    unsigned long long ex_k = 0, ex_w = 0;
    {
        if (a.pre_k) { if (tid == 0) { ex_k = a.pre_k[b]; ex_w = a.pre_w[b]; } }
        else for (int i = tid; i < b; i += PB) { const uint2 v = a.agg[i]; ex_k += v.x; ex_w += v.y; }
#pragma unroll
        for (int dd = 32; dd >= 1; dd >>= 1) { ex_k += (unsigned long long)__shfl_xor((long long)ex_k, dd, 64); ex_w += (unsigned long long)__shfl_xor((long long)ex_w, dd, 64); }
        if (lane == 0) { s_sum[wave] = ex_k; s_sum[PB / 64 + wave] = ex_w; }
    }
    // ---- the record chain (wavefront 0): the nearest block in front that fixes the state, minus the lengths of the record-less blocks behind it
    if (wave == 0) {
        int kind = CH_ID;
        long long val = 0, subs = 0;
        for (int hi = b - 1; hi >= 0 && kind != CH_CONST; hi -= 64) {
            const int e = hi - lane;
            const unsigned long long f = e >= 0 ? a.fn[e] : ch_pack(CH_ID, 0);
            const int k = ch_kind(f);
            const unsigned long long cmask = __ballot(k == CH_CONST);
            const int fc = cmask ? (int)__builtin_ctzll(cmask) : 64;
            long long sb = lane < fc && k == CH_SUB ? ch_val(f) : 0;
#pragma unroll
            for (int dd = 32; dd >= 1; dd >>= 1) sb += __shfl_xor(sb, dd, 64);
            subs += sb;
            if (fc < 64) { kind = CH_CONST; val = __shfl(ch_val(f), fc, 64); }
        }
        // in front of the file: expect = -1; in front of a range: OPEN (it starts wherever its first block finds a record)
        const bool open_in = kind != CH_CONST && a.ranged != 0;
        const long long state_in = kind == CH_CONST ? val - subs : -1 - subs;
        if (lane == 0) {
            const uint32_t first = mine ? a.first[b] : 0xFFFFFFFFu;
            const bool has = first != 0xFFFFFFFFu;
            const long long over = ch_val(a.fn[b]);                 // (pk_index resolved a size field that straddles the block's end)
            int ok = 1;
            long long state_out = state_in;
            bool open_out = open_in;
            if (mine && d.entry != -1) {
                if (has) {
                    const long long expect = d.entry >= 0 ? (long long)d.entry : state_in;
                    if (st == ST_BAD_RECORD) ok = 0;
                    if (!open_in || d.entry >= 0) { if ((long long)first != expect) ok = 0; }
                    else a.tot->range_first = d.uout + first + 1ull;      // (the range starts here, unvouched for: the range in front must end here)
                    if (over < 0) ok = 0;
                    state_out = over; open_out = false;
                } else if (!open_in || d.entry >= 0) {
                    const long long expect = d.entry >= 0 ? (long long)d.entry : state_in;
                    if (st == ST_BAD_RECORD) ok = 0;
                    if (expect < (long long)d.ulen) ok = 0;
                    state_out = expect - (long long)d.ulen; open_out = false;
                }
            }
            if (b == a.n_own - 1 || (a.n_own == 0 && b == 0)) {     // the end of the range: the last record must end in it — or in the block taken along
                if (!open_out) {
                    if (a.n_own < a.n_blocks) { if (state_out > (long long)a.blocks[a.n_own].ulen) ok = 0; }
                    else if (state_out > 0) ok = 0;
                    if (mine) a.tot->range_next = (unsigned long long)((long long)(d.uout + d.ulen) + state_out) + 1ull;
                }
            }
            if (!ok) atomicOr(&a.tot->flags, PKF_CHAIN);
        }
    }
    __syncthreads();
    ex_k = 0; ex_w = 0;
#pragma unroll
    for (int w = 0; w < PB / 64; ++w) { ex_k += s_sum[w]; ex_w += s_sum[PB / 64 + w]; }
    const uint2 mine_agg = a.agg[b];
    const uint32_t tot_w = mine_agg.y;
    const unsigned long long ex_r = a.rec_base[b];
    if (b == a.n_blocks - 1 && tid == 0) {
        a.tot->n_rec = ex_r + n; a.tot->n_kept = ex_k + mine_agg.x; a.tot->n_words = ex_w + tot_w;
        if (ex_r + n > 0x7FFFFFFFull || ex_k + mine_agg.x > 0x7FFFFFFFull) atomicOr(&a.tot->flags, PKF_REC_OVF);
    }
    if (n == 0) return;
    // room for this block's records, kept reads and words?  (the arrays are sized from bounds: a file beyond them takes the other path)
    if (ex_r + n > a.rec_cap || ex_w + tot_w + (unsigned long long)PK_WORD_SLACK > a.o.word_cap) {
        if (tid == 0) atomicOr(&a.tot->flags, ex_r + n > a.rec_cap ? PKF_REC_OVF : (uint32_t)PKF_WORD_OVF);
        return;
    }
    // ---- the kept reads' entries and their planes ---------------------------------------------------------------------------------------
    if constexpr (BQ) {
        if (a.pt.n_head + a.pt.n_tail) { stage_table(a.pt, s_tab); __syncthreads(); }     // (uniform: the workgroups that left above hold no records)
    }
    uint32_t run_k = 0, run_w = 0;                                  // kept reads / words of the tiles in front of this one
    for (uint32_t t0 = 0; t0 < n; t0 += PB) {
        const uint32_t t = t0 + (uint32_t)tid;
        uint4 r = make_uint4(0u, 0u, 0u, 0u);
        if (t < n) r = a.rrec[ex_r + t];
        const uint32_t word = r.x, nwords = word ? words_of(word & 1023u) : 0u;
        const uint2 incl = block_scan2(make_uint2(word ? 1u : 0u, nwords), s_w);
        __syncthreads();
        if (tid == PB - 1) s_w[0] = incl;
        __syncthreads();
        const uint32_t tile_k = s_w[0].x, tile_w = s_w[0].y;
        const uint32_t w_first = (uint32_t)ex_w + run_w;            // the tile's first word offset (its reads are contiguous from there)
        [[maybe_unused]] bool masked = false;
        if (word) {
            const uint32_t lk = incl.x - 1u, lwoff = incl.y - nwords;    // the read's place among the tile's kept reads; its first word, from the tile's
            const uint32_t j = (uint32_t)ex_k + run_k + lk, woff = w_first + lwoff;
            const int32_t pos = (int32_t)r.w;
            const uint2 sq = make_uint2(r.y, r.z);
            a.c_idx[j] = (uint32_t)(ex_r + t); a.c_pos[j] = pos; a.c_info[j] = word; a.c_woff[j] = woff; a.c_seq[j] = sq;
            const int npair = (int)((word & 1023u) + 31u) >> 5;
            const bool own = (word & INFO_PROJ) != 0;               // (its lane writes its pairs and the zero pair behind them)
            s_info[lk] = word; s_word[lk] = 2u + woff; s_pos[lk] = pos; s_seq[lk] = sq;
            [[maybe_unused]] uint32_t mw = 0u;
            if constexpr (BQ) {
                mw = mask_word_of(a.pt, s_tab, pos, (int32_t)(word & 1023u));
                masked = mw != 0u;
                mw = clip_merge(mw, a.pt.clip, ex_r + t, word & 1023u);
                s_mask[lk] = mw;
            }
            const uint32_t slot0 = lwoff >> 1;
            for (int q = 0; q < (int)(nwords >> 1); ++q) s_owner[slot0 + q] = own && q <= npair ? (uint16_t)0xFFFFu : (uint16_t)(lk | ((uint32_t)q << 8));
            if (own) pack_read<BQ>(view_rec(a.stream + a.rec_off[ex_r + t]), a.o, a.tot, word, pos, a.o.seq + 2u + woff, BQ ? a.drop + ((2u + woff) >> 1) : nullptr, a.min_bq, mw);
        }
        if constexpr (BQ) { if (a.pt.n_head + a.pt.n_tail) count_masked(masked, a.tot); }
        __syncthreads();
        uint2 *dst = reinterpret_cast<uint2 *>(a.o.seq + 2u + w_first);                      // (word offsets are multiples of 4: 8-byte aligned)
        for (uint32_t k = tid; k < (tile_w >> 1); k += PB) {           // (the twin of pk_planes' loop: one shared function reorders this kernel's code)
            const uint32_t ow = s_owner[k];
            if (ow == 0xFFFFu) continue;
            const int tt = (int)(ow & 255u), q = (int)(ow >> 8);
            const uint32_t info = s_info[tt];
            const int len = (int)(info & 1023u), npair = (len + 31) >> 5;
            uint32_t *ddst = BQ ? a.drop + ((2u + w_first) >> 1) : nullptr;     // (the pair at dst[k] has its drop word at ddst[k])
            if (q >= npair) {
                dst[k] = make_uint2(0u, 0u);
                if constexpr (BQ) ddst[k] = 0u;
                continue;
            }
            const uint2 where = s_seq[tt];
            const int l_seq = (int)(where.y >> 8), y = (int)(info >> 12) + 32 * q;
            const int nb = min(32, len - 32 * q), have = min(nb, l_seq - y);
            uint32_t lo, hi, ok;
            pair_planes(a.stream + ((((unsigned long long)(where.y & 0xFFu) << 32) | where.x) + (uint32_t)(y >> 1)), y & 1, have, lo, hi, ok);
            if constexpr (BQ) {
                const uint32_t dd = skipped32(a.stream + (((unsigned long long)(where.y & 0xFFu) << 32) | where.x) + ((size_t)l_seq + 1) / 2, l_seq, y, nb, a.min_bq,
                                              s_mask[tt], len, 32 * q);
                lo &= ~dd; hi &= ~dd; ok |= dd;
                ddst[k] = dd;
            }
            dst[k] = make_uint2(lo, hi);
            uint32_t miss = (nb >= 32 ? 0xFFFFFFFFu : ((1u << nb) - 1u)) & ~ok;
            while (miss) {
                const int bb = __builtin_ctz(miss);
                push_event(a.o, a.tot, (uint32_t)(s_pos[tt] + 32 * q + bb) | TCMI_F_EV_OTHER);
                miss &= miss - 1;
            }
        }
        run_k += tile_k; run_w += tile_w;
        __syncthreads();
    }
}
__global__ __launch_bounds__(PB) void pk_place(FusedArgs a) { place_body<false>(a); }
__global__ __launch_bounds__(PB, 5) void pk_place_bq(FusedArgs a) { place_body<true>(a); }
