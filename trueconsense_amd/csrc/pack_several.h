// pack_several.h — DEVICE: the several-kernel packer's kernels (tcmi_pack_on_device; pk_pack, which both packers launch, is
// pack_device.hip's): pk_classify, pk_scan, pk_scatter, and pk_planes / pk_planes_bq.  pack_device.hip includes it once, inside its unnamed
// namespace, behind classify_view and pack_bits.h.
// ---- classify: one lane per read ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PB) void pk_classify(PackSrc s, uint32_t *info, uint2 *rd_seq, int32_t *rd_pos, uint2 *blk_sum, unsigned long long *blk_alg,
                                                  int32_t *blk_end, PackTotals *tot, uint32_t *gen_idx)
{
    __shared__ uint2 s_w[PB / 64];
    __shared__ unsigned long long s_alg[PB / 64];
    __shared__ int32_t s_end[PB / 64];
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    uint32_t word = 0, nwords = 0;
    unsigned long long my_alg = 0;
    int32_t my_end = 0;
    uint32_t my_len = 0;
    int32_t my_tid = -1, my_lend = 0;
    bool dropped = false;
    if (i < s.n) {
        ReadView v = view(s, i);
        if (filter_on(s.flt)) filter_view(v, s.flt, tot);
        const int32_t shift = shift_of(s, v.tid);
        const Classified c = classify_view(v, s.mode, shift, shift >= 0 ? slot_end_of(s, v.tid) : 0, s.n_lay != 0,
                                           s.mode == 1 ? s.stream + s.rec_off[i] : nullptr, gen_idx != nullptr, tot);
        if (c.end > 0) { my_tid = v.tid; my_lend = c.end - shift; }
        if (c.slot_ovf) atomicMax(&tot->slot_ovf, ((unsigned long long)(i + 1) << 24) | (unsigned long long)min(v.tid, 0xFFFFFF));   // (the read the host names)
        dropped = s.n_lay && shift < 0 && !(v.flag & 0x4u) && v.tid >= 0 && v.pos >= 0;
        if (c.longread) gen_idx[atomicAdd(&tot->n_gen, 1u)] = (uint32_t)i;
        word = c.word; nwords = c.nwords; my_alg = c.alg; my_end = c.end; my_len = c.len;
        info[i] = word;
        // where the read's SEQ starts (bytes from the stream's / the SEQ array's first byte; low word | high byte) and l_seq:
        // pk_pack goes straight there instead of chasing record offset -> header -> CIGAR -> SEQ through four dependent loads
        const unsigned long long so = (unsigned long long)(v.seq - (s.mode == 0 ? s.seq : s.stream));
        rd_seq[i] = make_uint2((uint32_t)so, ((uint32_t)(so >> 32) & 0xFFu) | ((uint32_t)min(v.l_seq, 0xFFFFFF) << 8));
        rd_pos[i] = c.word ? v.pos + shift : v.pos;     // (pk_scatter's copy, on the axis: it need not go back to the record)
    }
    if (s.n_lay) {
        ref_extent_max(s.lay_ext, my_tid, my_lend);
        const unsigned long long m = __ballot(dropped);            // (one atomic per wavefront that holds dropped reads)
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(&tot->n_dropped, (unsigned long long)__popcll(m));
    }
    const uint2 incl = block_scan2(make_uint2(word ? 1u : 0u, nwords), s_w);
    if (threadIdx.x == PB - 1) blk_sum[blockIdx.x] = incl;
    // algorithmic bytes and extent: per-workgroup partials that pk_scan folds (same-address atomics serialise in L2:
    // 31 000 of them cost 0.39 ms); the twin of the fold that ends pk_index
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        my_alg += (unsigned long long)__shfl_xor((long long)my_alg, d, 64);
        my_end = max(my_end, __shfl_xor(my_end, d, 64));
        my_len = max(my_len, (uint32_t)__shfl_xor((int)my_len, d, 64));
    }
    // (the longest span rides in the top 16 bits of the byte sum: a workgroup's reads are < 2^48 bytes)
    if ((threadIdx.x & 63) == 0) { s_alg[threadIdx.x >> 6] = my_alg | ((unsigned long long)my_len << 48); s_end[threadIdx.x >> 6] = my_end; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long a = 0;
        int32_t e = 0;
        unsigned long long ml = 0;
        for (int w = 0; w < PB / 64; ++w) { a += s_alg[w] & 0xFFFFFFFFFFFFull; ml = max(ml, s_alg[w] >> 48); e = max(e, s_end[w]); }
        blk_alg[blockIdx.x] = a | (ml << 48);
        blk_end[blockIdx.x] = e;
    }
}

// ---- 2: exclusive scan of the workgroup sums (one workgroup, any number of entries) ---------------------------------
__global__ __launch_bounds__(1024) void pk_scan(uint2 *blk_sum, const unsigned long long *blk_alg, const int32_t *blk_end, int64_t n_blk,
                                                PackTotals *tot)
{
    __shared__ unsigned long long s_x[16], s_y[16];
    const int t = threadIdx.x;
    const int64_t per = (n_blk + 1023) / 1024, b0 = t * per, b1 = min(b0 + per, n_blk);
    unsigned long long sx = 0, sy = 0, alg = 0;
    int32_t mend = 0;
    uint32_t mlen = 0;
    for (int64_t b = b0; b < b1; ++b) {
        sx += blk_sum[b].x; sy += blk_sum[b].y; alg += blk_alg[b] & 0xFFFFFFFFFFFFull; mlen = max(mlen, (uint32_t)(blk_alg[b] >> 48)); mend = max(mend, blk_end[b]);
    }
    if (alg) atomicAdd(&tot->alg_bytes, alg);                  // (at most 1024 of these)
    if (mlen) atomicMax(&tot->max_len, mlen);
    if (mend) atomicMax(&tot->max_end, mend);
    // inclusive scan of the 1024 partials: within the wavefronts by shuffles, then the sixteen wavefront totals (two barriers;
    // ten rounds of Hillis-Steele through LDS cost twenty, and this kernel is one workgroup's latency from end to end)
    unsigned long long ix = sx, iy = sy;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long ox = (unsigned long long)__shfl_up((long long)ix, d, 64), oy = (unsigned long long)__shfl_up((long long)iy, d, 64);
        if ((t & 63) >= d) { ix += ox; iy += oy; }
    }
    if ((t & 63) == 63) { s_x[t >> 6] = ix; s_y[t >> 6] = iy; }
    __syncthreads();
    for (int w = 0; w < (t >> 6); ++w) { ix += s_x[w]; iy += s_y[w]; }
    unsigned long long bx = ix - sx, by = iy - sy;          // exclusive base of this lane's range
    for (int64_t b = b0; b < b1; ++b) {
        const uint2 v = blk_sum[b];
        blk_sum[b] = make_uint2((uint32_t)bx, (uint32_t)by);
        bx += v.x; by += v.y;
    }
    if (t == 1023) { tot->n_kept = ix; tot->n_words = iy; tot->n_chunks = 0; tot->n_events = 0; tot->n_runs = 0; tot->word_cursor = 0; }   // (the counters pk_pack / pk_planes take from)
}

// ---- 3: scatter: compacted index + word offset of every kept read -----------------------------------------------------
__global__ __launch_bounds__(PB) void pk_scatter(PackSrc s, const uint32_t *info, const uint2 *rd_seq, const int32_t *rd_pos, const uint2 *blk_base, uint32_t *c_idx,
                                                 int32_t *c_pos, uint32_t *c_info, uint32_t *c_woff, uint2 *c_seq)
{
    __shared__ uint2 s_w[PB / 64];
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    const uint32_t w = i < s.n ? info[i] : 0u;
    const uint2 mine = make_uint2(w ? 1u : 0u, w ? words_of(w & 1023u) : 0u);
    const uint2 incl = block_scan2(mine, s_w);
    if (w) {
        const uint2 base = blk_base[blockIdx.x];
        const uint32_t j = base.x + incl.x - 1u;
        c_idx[j] = (uint32_t)i;
        c_pos[j] = rd_pos[i];
        c_info[j] = w;
        c_woff[j] = base.y + incl.y - mine.y;
        c_seq[j] = rd_seq[i];
    }
}

// ---- 5: planes: one lane per 32 bases --------------------------------------------------------------------------------------
// A workgroup takes PB consecutive kept reads.  Every read's lane notes, for each of the read's pairs (and the zero pair behind
// them), "read t, pair q" in an LDS list indexed by the pair's place in the workgroup's stretch of the word stream; then the
// lanes take the places of that list in order: a lane loads ITS 16 bytes of SEQ, makes its pair and stores it — consecutive
// lanes read consecutive 16-byte pieces of a read and store consecutive 8-byte pairs (a read per lane, five pairs one after
// the other, kept 22 uncoalesced dword loads per lane in flight and the kernel at 16 waves a CU waiting for them).
// Reads that need their CIGAR walked (INFO_PROJ) are packed by their own lane, as before, straight to where they go.
// BQ (pk_planes_bq): under a base-quality floor Q — a pair also gets its word of the drop plane (drop[seq word / 2]): the 32 QUAL bytes
// behind SEQ compared with Q (dropped32), the skipped bases out of lo / hi and out of the OTHER events.  Q = 0: no floor, a primer
// table alone; pt: the table (every read's lane looks its mask word up once and leaves it in LDS beside s_info)
template <bool BQ>
__device__ __forceinline__ void planes_body(const PackSrc src, const PackOut o, const uint32_t *c_idx, const int32_t *c_pos, const uint32_t *c_info,
                                   const uint32_t *c_woff, const uint2 *c_seq, uint32_t n_kept, uint32_t n_words, PackTotals *tot, uint32_t *drop, uint32_t Q,
                                   [[maybe_unused]] const PrimerTab pt)
{
    __shared__ uint32_t s_info[PB], s_word[PB];
    [[maybe_unused]] __shared__ uint32_t s_mask[BQ ? PB : 1];
    [[maybe_unused]] __shared__ int32_t s_tab[BQ ? 3 * PT_LDS : 1];
    __shared__ int32_t s_pos[PB];
    __shared__ uint2 s_seq[PB];
    __shared__ uint16_t s_owner[PL_SLOTS];
    const int tid = threadIdx.x;
    const uint32_t r0 = (uint32_t)blockIdx.x * PB;
    const int n = (int)min((uint32_t)PB, n_kept - r0);
    const uint32_t w_first = c_woff[r0], w_end = r0 + (uint32_t)n < n_kept ? c_woff[r0 + n] : n_words;
    [[maybe_unused]] bool masked = false;
    if constexpr (BQ) {
        if (pt.n_head + pt.n_tail) { stage_table(pt, s_tab); __syncthreads(); }      // (uniform)
    }
    if (tid < n) {
        const uint32_t g = r0 + (uint32_t)tid, info = c_info[g], word = 2u + c_woff[g];      // (the read's place in the plane stream)
        const int32_t pos = c_pos[g];
        const int npair = (int)((info & 1023u) + 31u) >> 5;
        const uint32_t slot0 = (c_woff[g] - w_first) >> 1;
        const bool own = (info & INFO_PROJ) != 0;                       // (its lane writes its pairs and the zero pair behind them)
        const int n_slot = (int)(words_of(info & 1023u) >> 1);
        s_info[tid] = info; s_word[tid] = word; s_pos[tid] = pos; s_seq[tid] = c_seq[g];
        [[maybe_unused]] uint32_t mw = 0u;
        if constexpr (BQ) {
            mw = mask_word_of(pt, s_tab, pos, (int32_t)(info & 1023u));
            masked = mw != 0u;
            mw = clip_merge(mw, pt.clip, c_idx[g], info & 1023u);
            s_mask[tid] = mw;
        }
        for (int q = 0; q < n_slot; ++q) s_owner[slot0 + q] = own && q <= npair ? (uint16_t)0xFFFFu : (uint16_t)(tid | (q << 8));
        if (own) pack_read<BQ>(view(src, c_idx[g]), o, tot, info, pos, o.seq + word, BQ ? drop + (word >> 1) : nullptr, Q, mw);
    }
    if constexpr (BQ) { if (pt.n_head + pt.n_tail) count_masked(masked, tot); }
    __syncthreads();
    const uint8_t *bytes = src.mode == 0 ? src.seq : src.stream;
    const uint32_t n_slots = (w_end - w_first) >> 1;
    for (uint32_t k = tid; k < n_slots; k += PB) {                  // (the twin of pk_place's loop over its tile's places)
        const uint32_t ow = s_owner[k];
        if (ow == 0xFFFFu) continue;
        const int t = (int)(ow & 255u), q = (int)(ow >> 8);
        const uint32_t info = s_info[t];
        const int len = (int)(info & 1023u), npair = (len + 31) >> 5;
        uint2 *dst = reinterpret_cast<uint2 *>(o.seq + s_word[t]) + q;                  // (even word offsets: 8-byte aligned)
        if (q >= npair) {
            *dst = make_uint2(0u, 0u);
            if constexpr (BQ) drop[(s_word[t] >> 1) + q] = 0u;
            continue;
        }
        const uint2 where = s_seq[t];
        const int l_seq = (int)(where.y >> 8), y = (int)(info >> 12) + 32 * q;
        const int nb = min(32, len - 32 * q), have = min(nb, l_seq - y);
        uint32_t lo, hi, ok;
        const uint8_t *sq = bytes + (((unsigned long long)(where.y & 0xFFu) << 32) | where.x);
        pair_planes(sq + (uint32_t)(y >> 1), y & 1, have, lo, hi, ok);
        if constexpr (BQ) {
            const uint32_t d = skipped32(sq + ((size_t)l_seq + 1) / 2, l_seq, y, nb, Q, s_mask[t], len, 32 * q);
            lo &= ~d; hi &= ~d; ok |= d;
            drop[(s_word[t] >> 1) + q] = d;
        }
        *dst = make_uint2(lo, hi);
        uint32_t miss = (nb >= 32 ? 0xFFFFFFFFu : ((1u << nb) - 1u)) & ~ok;
        while (miss) {
            const int b = __builtin_ctz(miss);
            push_event(o, tot, (uint32_t)(s_pos[t] + 32 * q + b) | TCMI_F_EV_OTHER);
            miss &= miss - 1;
        }
    }
}
__global__ __launch_bounds__(PB) void pk_planes(PackSrc src, PackOut o, const uint32_t *c_idx, const int32_t *c_pos, const uint32_t *c_info,
                                                const uint32_t *c_woff, const uint2 *c_seq, uint32_t n_kept, uint32_t n_words,
                                                PackTotals *tot)
{
    planes_body<false>(src, o, c_idx, c_pos, c_info, c_woff, c_seq, n_kept, n_words, tot, nullptr, 0u, PrimerTab{nullptr, 0, 0, nullptr});
}
// (8 / 5 waves per SIMD asked of the two BQ kernels: what they ran at before they took the table — the mask word would otherwise cost
//  them a wave each, 67 and 99 vector registers; no scratch and no vector spill either way, scalar spills to lanes: DESIGN 6)
__global__ __launch_bounds__(PB, 8) void pk_planes_bq(PackSrc src, PackOut o, const uint32_t *c_idx, const int32_t *c_pos, const uint32_t *c_info,
                                                   const uint32_t *c_woff, const uint2 *c_seq, uint32_t n_kept, uint32_t n_words,
                                                   PackTotals *tot, uint32_t *drop, uint32_t Q, PrimerTab pt)
{
    planes_body<true>(src, o, c_idx, c_pos, c_info, c_woff, c_seq, n_kept, n_words, tot, drop, Q, pt);
}
