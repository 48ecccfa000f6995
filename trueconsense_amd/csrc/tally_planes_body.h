// tally_planes_body.h — the body of tally_planes_kernel and of tally_planes_drop_kernel (tally_planes.hip includes it once behind
// each kernel's head, with TCMI_TALLY_DROP 0 / 1).  One text, two kernels — and an include rather than a template function: the
// kernel without a drop plane keeps the machine code it had before there was a second one (tools/isa_diff.sh), which a shared
// device function called from two wrappers did not give.
{
    constexpr bool DROP = TCMI_TALLY_DROP != 0;
    constexpr int NVEC = DROP ? 4 : 3;          // lo, hi, lo & hi(, drop)
    constexpr int NREG = NVEC * 8;              // byte-counter registers per lane after the spread
    constexpr int HSLOTS = DROP ? 768 : 576;    // header slots (TCMI_P_SUB + the dummy); the buffer later holds the window counters
    constexpr int DCAP = TCMI_F_SEQCAP / 2;     // staged drop words: one per pair of the stage buffer
    static_assert(TCMI_P_SUB <= 2 * FB && TCMI_P_SUB < HSLOTS && HSLOTS * 8 >= NVEC * MAXPOS * 2, "s_hdr doubles as the 16-bit window counters");
    static_assert(4 * (FB / 2) <= HSLOTS - 3, "a lone four-read body of the widest slice layout must stay inside the header array");
    static_assert(NREG * FB <= TCMI_F_SEQCAP + (DROP ? DCAP : 0), "slice partials must fit the stage buffer");
    // staged planes(, behind them the staged drop words and two zero words); later the slice partials
    __shared__ __attribute__((aligned(16))) uint32_t s_seq[TCMI_F_SEQCAP + (DROP ? DCAP + 4 : 0)];
    __shared__ __attribute__((aligned(8))) uint2 s_hdr[HSLOTS];              // {pos - P0 | pairs << 16, byte offset in s_seq}
    __shared__ int32_t s_cov[MAXPOS + 8];                                     // coverage difference array
    __shared__ int s_scan[FB / 64];

    const int tid = threadIdx.x;
    if ((int)blockIdx.x < a.n_call2) {           // ride-along call of an earlier step's matrix (first in the grid: done early)
        call_other_tile(a, (int)blockIdx.x);
        return;
    }
    // then the tail blocks (event words) — in FRONT of the chunk blocks: behind them they started only when chunk blocks had left
    // (the chunk blocks of a 1M-read BAM fill every slot of the chip) and ran on their own at the launch's end
    const int b1 = (int)blockIdx.x - a.n_call2;
    if (b1 < a.n_tail) {
        tally_tail_block(a, b1, a.dev_counts ? (int64_t)min(a.dev_counts[1], (uint32_t)a.n_events) : a.n_events);
        return;
    }
    // A chunk block takes the chunks b, b + n_chunk_blocks, ..: when the counts are still on the device (the one-sync file path) the
    // grid is sized from the resident slots, not from the packer's CAPACITY — 5 700 blocks for the ~1 100 chunks of a 1M-read BAM, each
    // of the idle ones a trip to memory for the count while it held a slot (LDS and registers) that a chunk block was waiting for.
    const int n_real = a.dev_counts ? (int)min(a.dev_counts[0], (uint32_t)a.n_chunks) : a.n_chunks;
    for (int bid = b1 - a.n_tail; bid < n_real; bid += a.n_chunk_blocks) {
    const tcmi_fast_chunk *chp = a.chunks + bid;
    const int64_t read0 = chp->read0, word0 = chp->word0;
    const int n_reads = chp->n_reads, P0 = chp->P0, Wn = chp->Wn, sub_reads = chp->sub_reads;
    const int npos = Wn * 8;
    const int Gn = max(2, (npos + 31) >> 5);    // lane groups of 32 positions (at least two: S <= 128 keeps a body's four
                                                // header slots of a lane inside the header array)
    const int S = FB / Gn;                      // depth slices
    const int s = tid / Gn, gi = tid - s * Gn;
    const int base32p = gi * 32 + 32;           // first owned position relative to P0, + 32
    const int n_stage = (n_reads + sub_reads - 1) / sub_reads;

    for (int i = tid; i <= npos; i += FB) s_cov[i] = 0;
    // the last three header slots: a dummy read far to the right (no pairs: every lane is outside it) for the lanes
    // beyond the last depth slice and for the unused slots of a short stage, and 16 bytes of zeros that a lane outside
    // a read loads instead of the read's pairs
    if (tid < 3) s_hdr[HSLOTS - 3 + tid] = make_uint2(tid == 0 ? 0x7FFFu : 0u, 0u);
    [[maybe_unused]] uint32_t *const s_drop = s_seq + TCMI_F_SEQCAP;
    if constexpr (DROP) { if (tid < 2) s_drop[DCAP + tid] = 0u; }   // (what a lane outside a read loads instead of the read's drop words)
    const int zero_off = (int)(reinterpret_cast<const char *>(&s_hdr[HSLOTS - 2]) - reinterpret_cast<const char *>(s_seq));
    const int hb_first = s < S ? s * 8 : (HSLOTS - 3) * 8;       // byte offset of the lane's first header of a stage
    const int hb_step = s < S ? S * 8 : 0;
    __syncthreads();                            // before any wave adds coverage runs into it

    Planes cnt[NVEC];
#pragma unroll
    for (int v = 0; v < NVEC; ++v) {
#pragma unroll
        for (int k = 0; k < NPL; ++k) cnt[v].p[k] = 0;
    }

    // ---- prefetch registers: the next stage's headers (two slots per lane) and planes --------------
    uint32_t h_lo0 = 0, h_lo1 = 0;              // packed headers: position - P0 | len << 10 | pair offset in the stage << 20
    uint4 pre0 = {}, pre1 = {}, pre2 = {}, pre3 = {}, pre4 = {}, pre5 = {};
    [[maybe_unused]] uint2 dpre[6] = {};        // (DROP) the drop words of the same pairs: 8 bytes where the pairs take 16
    int st_begin = 0, st_end = chp->stage_end[0];   // word range of the stage (from word0)
    int st_end_next = chp->stage_end[1];            // fetched one stage ahead (a scalar load: its round trip hides under a stage)
    // Uniform base pointers + 32-bit lane offsets: the loads take the scalar-base form (no 64-bit address math
    // per lane).  Every lane loads (indices clamped into the stage): no exec-masked branch, so the loads stay in
    // flight across the inner loop.  (A macro, not a lambda: a closure kept the registers in scratch memory.)
    const uint32_t *lenoff_base = a.lenoff + read0;
    const uint32_t *seq_base = a.seq + word0;
    [[maybe_unused]] const uint32_t *drop_base = DROP ? a.drop + (word0 >> 1) : nullptr;      // (word0 is a multiple of 4)
#define TCMI_ISSUE_STAGE(stage_, begin_, end_)                                                        \
    do {                                                                                              \
        const uint32_t r0_ = (uint32_t)min((stage_) * sub_reads + tid, n_reads - 1);                  \
        const uint32_t r1_ = (uint32_t)min((stage_) * sub_reads + FB + tid, n_reads - 1);             \
        h_lo0 = lenoff_base[r0_];                                                                     \
        h_lo1 = lenoff_base[r1_];                                                                     \
        const int mis_ = (begin_) & 3; /* keep the 16-byte loads aligned (word0 is a multiple of 4) */ \
        const uint4 *src_ = reinterpret_cast<const uint4 *>(seq_base + ((begin_) - mis_));            \
        const uint32_t last_ = (uint32_t)(((end_) - (begin_) + mis_ + 3) / 4 - 1);                    \
        pre0 = src_[min((uint32_t)(0 * FB + tid), last_)];                                            \
        pre1 = src_[min((uint32_t)(1 * FB + tid), last_)];                                            \
        pre2 = src_[min((uint32_t)(2 * FB + tid), last_)];                                            \
        pre3 = src_[min((uint32_t)(3 * FB + tid), last_)];                                            \
        pre4 = src_[min((uint32_t)(4 * FB + tid), last_)];                                            \
        pre5 = src_[min((uint32_t)(5 * FB + tid), last_)];                                            \
        if constexpr (DROP) {                                                                         \
            const uint2 *dsrc_ = reinterpret_cast<const uint2 *>(drop_base + (((begin_) - mis_) >> 1)); \
            _Pragma("unroll") for (int k_ = 0; k_ < 6; ++k_) dpre[k_] = dsrc_[min((uint32_t)(k_ * FB + tid), last_)]; \
        }                                                                                             \
    } while (0)
    static_assert(NLD == 6, "six 16-byte loads per lane cover a stage");
    TCMI_ISSUE_STAGE(0, st_begin, st_end);
    // coverage: the packer lists the chunk's reads as runs of equal (position, length) — a few dozen words for a few
    // thousand reads of a sorted BAM; each becomes a (+n, -n) pair in the difference array (prefix-summed at the end)
    {
        const uint32_t *runs = a.covrun + chp->run0;
        const int n_runs = chp->n_runs;
        for (int i = tid; i < n_runs; i += FB) {
            const uint32_t w = runs[i];
            const int rel = (int)(w & 1023u), len = (int)((w >> 10) & 1023u), n = (int)(w >> 20);
            atomicAdd(&s_cov[rel], n);
            atomicAdd(&s_cov[rel + len], -n);
        }
    }

    for (int stage = 0; stage < n_stage; ++stage) {
        const int ns = min(sub_reads, n_reads - stage * sub_reads);
        const int mis = st_begin & 3;
        // ---- A: headers, coverage runs and planes of this stage -> LDS ------------------------------
        const bool valid0 = tid < ns, valid1 = tid + FB < ns;
        // header slots up to the end of the stage's last inner-loop body: real reads, then dummies
        const int Rs = (ns + S - 1) / S;
        const int k_end = Rs <= 4 ? 4 : Rs <= 8 ? 8 : (Rs + 3) & ~3;   // bodies: 8, 8, ..., then 4 (mirrors the loop below)
        const int pad_end = k_end * S;
        {
            uint2 h0 = make_uint2(0x7FFFu, 0u), h1 = h0;
            if (valid0) {
                const int rel0 = (int)(h_lo0 & 1023u), len0 = (int)((h_lo0 >> 10) & 1023u);
                const int off = (int)(h_lo0 >> 20) * 2 + mis;          // word index of the read in s_seq (even)
                h0 = make_uint2((uint32_t)rel0 | ((uint32_t)(len0 + 31) >> 5) << 16, (uint32_t)(off - 2) * 4u);
            }
            if (valid1) {
                const int rel1 = (int)(h_lo1 & 1023u), len1 = (int)((h_lo1 >> 10) & 1023u);
                const int off = (int)(h_lo1 >> 20) * 2 + mis;
                h1 = make_uint2((uint32_t)rel1 | ((uint32_t)(len1 + 31) >> 5) << 16, (uint32_t)(off - 2) * 4u);
            }
            if (tid < pad_end) s_hdr[tid] = h0;
            if (tid + FB < pad_end) s_hdr[tid + FB] = h1;
        }
        {   // all six stores, whatever the stage's length: the loads were clamped into the stage, the buffer holds
            // 6 * 256 * 16 bytes, and nothing reads past the stage's last zero pair
            uint4 *dst = reinterpret_cast<uint4 *>(s_seq);
            {
                dst[0 * FB + tid] = pre0;
                dst[1 * FB + tid] = pre1;
                dst[2 * FB + tid] = pre2;
                dst[3 * FB + tid] = pre3;
                dst[4 * FB + tid] = pre4;
                dst[5 * FB + tid] = pre5;
            }
            if constexpr (DROP) {
                uint2 *ddst = reinterpret_cast<uint2 *>(s_drop);
#pragma unroll
                for (int k_ = 0; k_ < 6; ++k_) ddst[k_ * FB + tid] = dpre[k_];
            }
        }
        // ---- B: issue the next stage's loads at once — in front of the barrier, so that this workgroup has loads in
        //      flight while it waits there (the LDS stores above have read their registers); they complete while C runs
        if (stage + 1 < n_stage) {
            st_begin = st_end - 2;                               // the zero pair behind the last read comes along
            st_end = st_end_next;
            st_end_next = chp->stage_end[min(stage + 2, TCMI_F_MAXSTAGE - 1)];
            TCMI_ISSUE_STAGE(stage + 1, st_begin, st_end);
        }
        __syncthreads();
        // ---- C: this lane's slice of the staged reads: r = s, s + S, s + 2S, ...  Branch-free bodies of eight
        //      reads, then at most one body of four (a stage holds S * 4 * m reads); the slots past the stage's reads
        //      hold dummy headers.
        const int Rc = Rs;
        int hb = hb_first;                                       // byte offset of the lane's next header
#define TCMI_FETCH4(lo_, hi_, both_, dr_, at_)                                                                         \
    do {                                                                                                          \
        uint2 h_[4];                                                                                              \
        _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                                           \
            h_[u] = *reinterpret_cast<const uint2 *>(reinterpret_cast<const char *>(s_hdr) + hb);                 \
            hb += hb_step;                                                                                        \
        }                                                                                                         \
        _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                                           \
            /* d = first owned position relative to the read start; t = pair holding it, + 1 */                    \
            const int dp_ = base32p - (int)(h_[u].x & 0xFFFFu);  /* d + 32 */                                       \
            const int t_ = dp_ >> 5;                                                                              \
            /* one zero pair lies on either side of a read: pairs t - 1 and t are loaded for 0 <= t <= pairs; a   \
               lane further out (clamped index) is outside the read altogether and loads the 16 zero bytes */       \
            const int tc_ = max(0, min(t_, (int)(h_[u].x >> 16)));                                                \
            const int at_b_ = tc_ == t_ ? (int)h_[u].y + tc_ * 8 : zero_off;                                      \
            const uint2 *wp_ = reinterpret_cast<const uint2 *>(reinterpret_cast<const char *>(s_seq) + at_b_);    \
            const uint2 w0_ = wp_[0], w1_ = wp_[1];             /* {lo, hi} of pairs t - 1 and t */                 \
            lo_[(at_) + u] = __builtin_amdgcn_alignbit(w1_.x, w0_.x, (uint32_t)dp_);   /* bits [4:0] = d mod 32 */  \
            hi_[(at_) + u] = __builtin_amdgcn_alignbit(w1_.y, w0_.y, (uint32_t)dp_);                               \
            both_[(at_) + u] = lo_[(at_) + u] & hi_[(at_) + u];                                                   \
            if constexpr (DROP) {                                                                                 \
                const int dat_b_ = tc_ == t_ ? ((int)h_[u].y + tc_ * 8) >> 1 : DCAP * 4;                          \
                const uint32_t *dp2_ = reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(s_drop) + dat_b_); \
                dr_[(at_) + u] = __builtin_amdgcn_alignbit(dp2_[1], dp2_[0], (uint32_t)dp_);                      \
            }                                                                                                     \
        }                                                                                                         \
    } while (0)
        int k = 0;
        for (; TCMI_P_BODY8 && Rc - k > 4; k += 8) {
            uint32_t lo[8], hi[8], both[8];
            [[maybe_unused]] uint32_t dr[8];
            TCMI_FETCH4(lo, hi, both, dr, 0);
            TCMI_FETCH4(lo, hi, both, dr, 4);
            add8(cnt[0], lo);
            add8(cnt[1], hi);
            add8(cnt[2], both);
            if constexpr (DROP) add8(cnt[NVEC - 1], dr);
        }
        for (; k < Rc; k += 4) {
            uint32_t lo[4], hi[4], both[4];
            [[maybe_unused]] uint32_t dr[4];
            TCMI_FETCH4(lo, hi, both, dr, 0);
            add4(cnt[0], lo);
            add4(cnt[1], hi);
            add4(cnt[2], both);
            if constexpr (DROP) add4(cnt[NVEC - 1], dr);
        }
#undef TCMI_FETCH4
        __syncthreads();                                        // every lane is done with this stage's LDS
    }
    // ---- planes -> byte counters -> LDS, layout [register j][lane] (conflict-free both ways) ---------
    uint32_t *s_part = s_seq;
    uint16_t (*s_fin)[MAXPOS] = reinterpret_cast<uint16_t (*)[MAXPOS]>(s_hdr);   // window counters of lo, hi, lo&hi(, drop)
    {
        const int per_lane = n_stage * ((sub_reads + S - 1) / S);                  // bound on the reads per lane (dummies count nothing)
        // planes that can be non-zero: one uniform branch, then straight-line code (few reads per lane leave the top
        // planes empty)
        if (per_lane < 32) spread_all<5>(cnt, s_part, tid);
        else if (per_lane < 64) spread_all<6>(cnt, s_part, tid);
        else if (per_lane < 128) spread_all<(NPL < 7 ? NPL : 7)>(cnt, s_part, tid);
        else spread_all<NPL>(cnt, s_part, tid);
    }
    __syncthreads();
    // ---- sum the slices; register j of group g holds 4 positions (j%8 + 8 i) of one vector ------------
    for (int item = tid; item < Gn * NREG; item += FB) {
        const int j = item / Gn, g = item - j * Gn;
        uint32_t e = 0, o = 0;                                  // bytes 0,2 and bytes 1,3 as 16-bit sums
        const uint32_t *row = s_part + j * FB + g;
        for (int t = 0; t < S; t += 4) {                        // four independent LDS loads in flight
            const uint32_t v0 = row[t * Gn];
            const uint32_t v1 = t + 1 < S ? row[(t + 1) * Gn] : 0u;
            const uint32_t v2 = t + 2 < S ? row[(t + 2) * Gn] : 0u;
            const uint32_t v3 = t + 3 < S ? row[(t + 3) * Gn] : 0u;
            e += (v0 & 0x00FF00FFu) + (v1 & 0x00FF00FFu) + (v2 & 0x00FF00FFu) + (v3 & 0x00FF00FFu);
            o += ((v0 >> 8) & 0x00FF00FFu) + ((v1 >> 8) & 0x00FF00FFu) + ((v2 >> 8) & 0x00FF00FFu) + ((v3 >> 8) & 0x00FF00FFu);
        }
        const int v = j >> 3;
        const int p = g * 32 + (j & 7);                         // byte i of the register <-> position p + 8 i
        uint16_t *f = &s_fin[v][p];
        if (p < npos) f[0] = (uint16_t)(e & 0xFFFFu);
        if (p + 8 < npos) f[8] = (uint16_t)(o & 0xFFFFu);
        if (p + 16 < npos) f[16] = (uint16_t)(e >> 16);
        if (p + 24 < npos) f[24] = (uint16_t)(o >> 16);
    }
    // ---- coverage: inclusive prefix sum of the difference array, CPL entries per lane ----------------
    {
        const int i0 = tid * CPL;
        int d[CPL], sum = 0;
#pragma unroll
        for (int k = 0; k < CPL; ++k) { d[k] = i0 + k < npos ? s_cov[i0 + k] : 0; sum += d[k]; }
        int run = block_scan_incl(sum, s_scan) - sum;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            run += d[k];
            if (i0 + k < npos) s_cov[i0 + k] = run;
        }
    }
    __syncthreads();
    if constexpr (DROP) {                       // coverage = runs - n(drop): the skipped tokens are absent from their columns
        for (int p = tid; p < npos; p += FB) s_cov[p] -= (int32_t)s_fin[NVEC - 1][p];
        __syncthreads();
    }
    // ---- global atomics: coverage, C, G, T of TWO adjacent positions per 64-bit add (the columns never go
    //      negative and never carry out of 32 bits), A one position at a time (the tail blocks subtract from it, so
    //      it may be transiently negative and a carry would spill into the neighbour) ---------------------------
#ifdef TCMI_TALLY_NO_ATOMICS                        // (diagnostic build: the kernel without its adds to the matrix — how much of its time they are)
    if (a.L < 0) {
#else
    if (a.pair_ok) {
#endif
        for (int p = 2 * tid; p < npos; p += 2 * FB) {
            const int gp = P0 + p;                                  // even: P0 is a multiple of 8
            if (gp >= a.L) continue;
            const bool two = gp + 1 < a.L;                          // (npos is a multiple of 8: p + 1 is inside the window)
            const int cv0 = s_cov[p], cv1 = two ? s_cov[p + 1] : 0;
            if ((cv0 | cv1) == 0) continue;
            const int nT0 = s_fin[2][p], nC0 = s_fin[0][p] - nT0, nG0 = s_fin[1][p] - nT0;
            const int nT1 = two ? s_fin[2][p + 1] : 0, nC1 = two ? s_fin[0][p + 1] - nT1 : 0, nG1 = two ? s_fin[1][p + 1] - nT1 : 0;
            const int nA0 = cv0 - nC0 - nG0 - nT0, nA1 = cv1 - nC1 - nG1 - nT1;   // include the class-less positions (tail blocks)
            auto add2 = [&](int col, int v0, int v1) {
                if (v0 | v1)
                    atomicAdd(reinterpret_cast<unsigned long long *>(&a.counts[(int64_t)col * a.ld + gp]),
                              (unsigned long long)(uint32_t)v0 | ((unsigned long long)(uint32_t)v1 << 32));
            };
            add2(TCMI_COV, cv0, cv1);
            add2(TCMI_C, nC0, nC1);
            add2(TCMI_G, nG0, nG1);
            add2(TCMI_T, nT0, nT1);
            if (nA0) atomicAdd(&a.counts[(int64_t)TCMI_A * a.ld + gp], nA0);
            if (nA1) atomicAdd(&a.counts[(int64_t)TCMI_A * a.ld + gp + 1], nA1);
        }
#ifdef TCMI_TALLY_NO_ATOMICS
    } else if (a.L < 0) {
#else
    } else {
#endif
        for (int p = tid; p < npos; p += FB) {
            const int gp = P0 + p;
            if (gp >= a.L) continue;
            const int cv = s_cov[p];
            if (cv == 0) continue;
            const int nT = s_fin[2][p], nC = s_fin[0][p] - nT, nG = s_fin[1][p] - nT;
            const int nA = cv - nC - nG - nT;                       // includes the class-less positions, taken out by the tail blocks
            atomicAdd(&a.counts[(int64_t)TCMI_COV * a.ld + gp], cv);
            if (nA) atomicAdd(&a.counts[(int64_t)TCMI_A * a.ld + gp], nA);
            if (nC) atomicAdd(&a.counts[(int64_t)TCMI_C * a.ld + gp], nC);
            if (nG) atomicAdd(&a.counts[(int64_t)TCMI_G * a.ld + gp], nG);
            if (nT) atomicAdd(&a.counts[(int64_t)TCMI_T * a.ld + gp], nT);
        }
    }
    __syncthreads();                            // (the next chunk's set-up writes what the adds above read)
    }
}
#undef TCMI_ISSUE_STAGE
