// indel_events.hip — --indel-table on gfx950: one event per insertion or deletion at given columns, with its length, its bases and the
// number of records that carry it, counted in the inflated BAM stream a device-decoded read set left in the context's arena
// (include/tcmi.h: tcmi_readset_indel_events).  What an event is, its key and hash, and which event is reported: indel_rule.h.  The
// per-column walk and the token rule (open_walk, token_at, first_at_or_above): stream_walk.h; which record is kept (kept_span), the wave
// join: pack_device.h; the residency refusals, the scratch, the launch shape, the workgroup's counter frame: stream_count.h.
//
// Unlike the counting kernels the answer is no fixed array: which lengths and which sequences there are is only known once the records
// have been read.  So the counters live in an open-addressing table in device memory, keys[S] | rep[S] | cnt[S], S a power of two:
//   pass 1, count    one lane per record, 256-lane workgroups that stride over the records, the grid of the counting kernels.  Per
//                    round (each lane's next queried column) a lane has at most one DEL and one INS.  The lanes of a wavefront with the
//                    same key are joined (wave_join: a real indel in a sorted BAM puts all 64 lanes on one key) and the group's leader
//                    alone goes to the table: linear probing from a mix of the key, at most MAX_PROBE steps; an empty slot (0) is
//                    claimed with a 64-bit atomicCAS; the group's popcount is added to the slot's 32-bit counter; a 64-bit atomicMin
//                    of (record index << 16 | op index) makes the first record in file order the slot's representative.  The
//                    per-column totals go through the workgroup's CountFrame.  A probe that runs out, or a full table, sets a flag.
//                    NO LANE EVER WAITS for another lane's store: a slot's key changes once, from 0, and a lane that sees 0 asks the
//                    CAS, which tells the truth; sums and a minimum do not depend on the order of arrival.
//   pass 2, verify   the same walk.  A DEL's key is exact.  An INS finds its slot — it must be there — and compares its length and
//                    its nibbles with the representative's, whose record is walked again to its query index.  A mismatch — two
//                    different insertions of one column under one hash — is counted; the host then starts over with another seed.
//   pass 3, gather   one lane per slot.  An occupied slot that passes the rule is appended to the event list (an atomic counter: the
//                    list's order is arbitrary, the host sorts it), an insertion's letters are copied from the representative's SEQ
//                    into the text buffer.  Nothing is gathered from a table that overflowed or collided.
// One bracket (TCMI_K_INDEL_EVENTS) around the launches of an attempt, one wait per attempt, one more for the download.
#include <algorithm>
#include <cstring>
#include <vector>

#include "stream_count.h"
#include "stream_walk.h"
#include "indel_rule.h"

namespace {

constexpr int BLOCK = SC_BLOCK;
constexpr int LDS_N = TCMI_INDEL_LDS;
constexpr int MAX_PROBE = 64;
constexpr int64_t MAX_N = 1 << 20;
constexpr int MAX_SLOTS_LOG = 24;
constexpr int64_t MAX_INS = 1 << 30;     // a longer insertion (no l_seq admits it: the bases would all read as N) is refused

using u64 = unsigned long long;

struct IeHdr {                          // what an attempt tells the host (zeroed in front of it)
    uint32_t overflow, collisions, missing, too_long;
    uint32_t n_events, pad;
    u64 text_used;
};

struct IeArgs {
    PackSrc src;                        // the resident stream, the read set's filter, floor and layout
    tcmi_primer_tab pt;                 // the primer table the read set was built under (none: zeros)
    const int32_t *cols;                // [n] ascending
    const int32_t *cov;                 // [n]
    int32_t *totals;                    // [n][2]: ins_total, del_total
    int32_t n;
    uint32_t seed;
    int32_t bits;
    uint32_t slot_mask;                 // S - 1
    u64 *keys, *rep;                    // [S]
    uint32_t *cnt;                      // [S]
    IeHdr *hdr;
    // pass 3
    tcmi_var_rule rule;
    int32_t apply_rule;
    uint32_t ev_cap;
    tcmi_indel_event *events;           // [ev_cap]
    char *text;                         // [text_cap]
    u64 text_cap;
};

struct CgLd {                           // CIGAR word j of a record in the stream (any byte address)
    const uint8_t *cg;
    __device__ uint32_t operator()(uint32_t j) const { return ld_u32(cg + 4 * (size_t)j); }
};

__device__ inline uint32_t nib_of(const ReadView &v, int64_t qi) { return qi < (int64_t)v.l_seq ? nib_at(v.seq, (int32_t)qi) : 15u; }

// the events of the record at the column token_at just answered `bits` for: w.k is the op that holds it
struct ColEvents {
    bool del, ins;
    int32_t del_len;
    int64_t y_ins;                      // the query index behind op w.k
};
__device__ inline ColEvents events_at(const Walk &w, int32_t c, uint32_t bits)
{
    ColEvents e = {false, false, 0, 0};
    if (bits == 0u) return e;
    const uint32_t cw = ld_u32(w.v.cigar + 4 * (size_t)w.k), op = cw & 0xFu;
    const int32_t len = (int32_t)(cw >> 4);
    e.del = op == 2 && c == w.x;
    e.del_len = len;
    e.ins = (bits >> TCMI_I) & 1u;
    e.y_ins = (int64_t)w.y + (is_match(op) ? len : 0);
    return e;
}

// the insertion behind op k of record v: its hash, and its length
__device__ inline uint64_t ins_hash(const ReadView &v, uint32_t k, int64_t y, uint32_t seed, int bits, int64_t &len)
{
    tcmi_ins_iter<CgLd> it(CgLd{v.cigar}, v.n_cigar, k, y);
    uint64_t h = tcmi_indel_hash_begin(seed);
    len = 0;
    for (int64_t qi; (qi = it.next()) >= 0; ++len) h = tcmi_indel_hash_step(h, nib_of(v, qi));
    return tcmi_indel_hash_end(h, len, bits);
}

// the slot of `key`, claimed when nobody has: -1 when MAX_PROBE steps (or the whole table) hold other keys
__device__ inline int64_t slot_claim(const IeArgs &a, u64 key)
{
    const uint32_t steps = a.slot_mask + 1u < (uint32_t)MAX_PROBE ? a.slot_mask + 1u : (uint32_t)MAX_PROBE;
    uint32_t s = (uint32_t)tcmi_indel_slot0(key) & a.slot_mask;
    for (uint32_t t = 0; t < steps; ++t, s = (s + 1u) & a.slot_mask) {
        u64 cur = *(volatile const u64 *)&a.keys[s];       // (a key is written once, over 0: what is not 0 is final)
        if (cur == 0ull) {
            cur = atomicCAS(&a.keys[s], 0ull, key);
            if (cur == 0ull) cur = key;
        }
        if (cur == key) return (int64_t)s;
    }
    return -1;
}
// ... behind pass 1: the slot that holds `key`, -1 when none does
__device__ inline int64_t slot_find(const IeArgs &a, u64 key)
{
    const uint32_t steps = a.slot_mask + 1u < (uint32_t)MAX_PROBE ? a.slot_mask + 1u : (uint32_t)MAX_PROBE;
    uint32_t s = (uint32_t)tcmi_indel_slot0(key) & a.slot_mask;
    for (uint32_t t = 0; t < steps; ++t, s = (s + 1u) & a.slot_mask) {
        const u64 cur = a.keys[s];
        if (cur == key) return (int64_t)s;
        if (cur == 0ull) return -1;
    }
    return -1;
}

// the frame of passes 1 and 2: f(i, w, c, ci, e) for every queried column c = cols[ci] of kept record i, every lane of a wavefront
// together (have: the lane has a column in this round)
template <class F> __device__ inline void each_column(const IeArgs &a, const int32_t *cols, F f)
{
    const uint32_t Q = a.src.min_bq;
    each_record(a.src.n, [&](int64_t i) {
        Walk w;
        int32_t ci = 0;
        bool have = i < a.src.n && open_walk(a.src, a.pt, i, w);
        if (have) {
            ci = first_at_or_above(cols, a.n, w.x);
            have = ci < a.n && cols[ci] <= w.q;
        }
        while (__ballot(have)) {                            // one round per queried column of the wavefront's busiest record
            ColEvents e = {false, false, 0, 0};
            if (have) e = events_at(w, cols[ci], token_at(w, cols[ci], Q));
            f(i, w, ci, e);
            if (have) {
                ++ci;
                have = ci < a.n && cols[ci] <= w.q;
            }
        }
    });
}

__global__ __launch_bounds__(BLOCK) void indel_count_kernel(IeArgs a)
{
    __shared__ int32_t s_cols[LDS_N];
    __shared__ uint32_t s_cnt[2 * LDS_N];
    const int tid = threadIdx.x, lane = tid & 63;
    const CountFrame<int32_t> tot = {s_cnt, a.totals, a.n <= LDS_N};
    if (tot.staged) {
        for (int k = tid; k < a.n; k += BLOCK) s_cols[k] = a.cols[k];
        tot.zero(2 * a.n);
        __syncthreads();
    }
    const int32_t *cols = tot.staged ? s_cols : a.cols;
    each_column(a, cols, [&](int64_t i, const Walk &w, int32_t ci, const ColEvents &e) {
        bool ins = e.ins;
        u64 kd = 0ull, ki = 0ull, me = 0ull;
        if (e.del || e.ins) me = ((u64)i << 16) | (u64)w.k;
        if (e.del) kd = tcmi_indel_key(cols[ci], TCMI_INDEL_DEL, (uint64_t)e.del_len);
        if (e.ins) {
            int64_t len;
            const uint64_t h = ins_hash(w.v, w.k, e.y_ins, a.seed, a.bits, len);
            if (len > MAX_INS) { a.hdr->too_long = 1u; ins = false; }
            ki = tcmi_indel_key(cols[ci], TCMI_INDEL_INS, h);
        }
        // one pass per distinct key of the round; the leader is the group's lowest lane, so its record is the group's first
        const auto join = [&](bool todo, u64 key, int which) {
            wave_join(todo, key, [&](int lead, u64 lk, bool same) {
                const u64 m = __ballot(same);
                if (lane != lead) return;
                const int c = __popcll(m);
                tot.add(2 * (int64_t)ci + which, c);
                const int64_t s = slot_claim(a, lk);
                if (s < 0) { a.hdr->overflow = 1u; return; }
                atomicAdd(&a.cnt[s], (uint32_t)c);
                atomicMin(&a.rep[s], me);
            });
        };
        join(ins, ki, 0);
        join(e.del, kd, 1);
    });
    tot.flush(2 * a.n);
}

__global__ __launch_bounds__(BLOCK) void indel_verify_kernel(IeArgs a)
{
    if (a.hdr->overflow | a.hdr->too_long) return;          // (uniform: the host starts over anyway)
    each_column(a, a.cols, [&](int64_t i, const Walk &w, int32_t ci, const ColEvents &e) {
        if (!e.ins) return;
        int64_t len;
        const uint64_t h = ins_hash(w.v, w.k, e.y_ins, a.seed, a.bits, len);
        const int64_t s = slot_find(a, tcmi_indel_key(a.cols[ci], TCMI_INDEL_INS, h));
        if (s < 0) { atomicAdd(&a.hdr->missing, 1u); return; }
        const u64 rep = a.rep[s];
        const int64_t r = (int64_t)(rep >> 16);
        const uint32_t rk = (uint32_t)(rep & 0xFFFFull);
        if (r == i && rk == w.k) return;                    // (the representative itself)
        if (r >= a.src.n) { atomicAdd(&a.hdr->missing, 1u); return; }
        const ReadView rv = view_rec(a.src.stream + a.src.rec_off[r]);
        if (rk >= rv.n_cigar) { atomicAdd(&a.hdr->missing, 1u); return; }
        int64_t ry = 0;                                     // the representative's query index behind its op rk
        for (uint32_t j = 0; j <= rk; ++j) {
            const uint32_t cw = ld_u32(rv.cigar + 4 * (size_t)j);
            if (consumes_query(cw & 0xFu)) ry += cw >> 4;
        }
        tcmi_ins_iter<CgLd> mine(CgLd{w.v.cigar}, w.v.n_cigar, w.k, e.y_ins), its(CgLd{rv.cigar}, rv.n_cigar, rk, ry);
        bool equal = true;
        for (;;) {
            const int64_t qa = mine.next(), qb = its.next();
            if (qa < 0 || qb < 0) { equal = qa < 0 && qb < 0; break; }
            if (nib_of(w.v, qa) != nib_of(rv, qb)) { equal = false; break; }
        }
        if (!equal) atomicAdd(&a.hdr->collisions, 1u);
    });
}

__global__ __launch_bounds__(BLOCK) void indel_gather_kernel(IeArgs a)
{
    if (a.hdr->overflow | a.hdr->too_long | a.hdr->collisions | a.hdr->missing) return;
    const int64_t S = (int64_t)a.slot_mask + 1;
    for (int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x; s < S; s += (int64_t)gridDim.x * BLOCK) {
        const u64 key = a.keys[s];
        if (key == 0ull) continue;
        const int32_t col = tcmi_indel_key_col(key), count = (int32_t)a.cnt[s];
        const int kind = tcmi_indel_key_kind(key);
        const int32_t ci = first_at_or_above(a.cols, a.n, col);
        const int32_t cov = ci < a.n ? a.cov[ci] : 0;
        if (a.apply_rule && !tcmi_indel_rule_passes(count, cov, a.rule)) continue;
        const u64 rep = a.rep[s];
        const int64_t r = (int64_t)(rep >> 16);
        const uint32_t rk = (uint32_t)(rep & 0xFFFFull);
        int64_t len = (int64_t)tcmi_indel_key_h(key), off = -1;
        if (kind == TCMI_INDEL_INS) {
            if (r >= a.src.n) continue;
            const ReadView rv = view_rec(a.src.stream + a.src.rec_off[r]);
            if (rk >= rv.n_cigar) continue;
            int64_t ry = 0;
            for (uint32_t j = 0; j <= rk; ++j) {
                const uint32_t cw = ld_u32(rv.cigar + 4 * (size_t)j);
                if (consumes_query(cw & 0xFu)) ry += cw >> 4;
            }
            tcmi_ins_iter<CgLd> n_it(CgLd{rv.cigar}, rv.n_cigar, rk, ry);
            for (len = 0; n_it.next() >= 0;) ++len;
            off = (int64_t)atomicAdd(&a.hdr->text_used, (u64)len);
            if ((u64)(off + len) <= a.text_cap) {
                tcmi_ins_iter<CgLd> it(CgLd{rv.cigar}, rv.n_cigar, rk, ry);
                int64_t t = off;
                for (int64_t qi; (qi = it.next()) >= 0; ++t) a.text[t] = tcmi_indel_letter(nib_of(rv, qi));
            }
        }
        const uint32_t idx = atomicAdd(&a.hdr->n_events, 1u);
        if (idx < a.ev_cap) {
            tcmi_indel_event ev;
            ev.pos = col; ev.kind = kind; ev.len = (int32_t)len; ev.count = count; ev.cov = cov; ev.reserved = 0; ev.text_off = off;
            a.events[idx] = ev;
        }
    }
}

// One read set on its own context -> its events (any order) and, added into tot[2 n], its per-column totals.  `opt`: the context the
// call was made on (its options, its counters).  rule = nullptr: every event (a part of a read set of sub-ranges).
int indel_events_one(tcmi_ctx *opt, tcmi_ctx *ctx, const tcmi_readset *rs, const std::vector<int32_t> &c32, const int32_t *cov, const tcmi_var_rule *rule,
                     tcmi_indel_list &out, std::vector<int64_t> &tot)
{
    const char *what = "indel events";
    if (const int rc = tcmi_stream_countable(ctx, rs, what)) return rc < 0 ? rc : TCMI_OK;
    TCMI_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = c32.size();
    int slots_log = opt->indel_slots;
    uint32_t seed = 0;
    size_t ev_cap = 4096, text_cap = 64u << 10;
    IeHdr hdr;
    for (;;) {
        const size_t S = (size_t)1 << slots_log;
        const size_t b_in = tcmi_align256(8 * n), b_tot = tcmi_align256(8 * n), b_hdr = 256, b_keys = tcmi_align256(8 * S), b_cnt = tcmi_align256(4 * S),
                     b_rep = b_keys, b_ev = tcmi_align256(ev_cap * sizeof(tcmi_indel_event)), b_text = tcmi_align256(text_cap);
        const size_t b_zero = b_tot + b_hdr + b_keys + b_cnt, total = b_in + b_zero + b_rep + b_ev + b_text;
        if (!tcmi_grow_dev(ctx, ctx->count_dev, ctx->count_dev_cap, total, 64u << 10))
            return tcmi_fail(ctx, TCMI_E_NOMEM, "%s: device scratch (%zu bytes)", what, total + (64u << 10));
        char *pin = static_cast<char *>(tcmi_ctx_pinned(ctx, b_in + b_hdr + b_tot));
        if (!pin) return tcmi_fail(ctx, TCMI_E_NOMEM, "%s: pinned scratch", what);
        std::memcpy(pin, c32.data(), 4 * n);
        std::memcpy(pin + 4 * n, cov, 4 * n);
        char *d = ctx->count_dev;
        IeArgs a = {};
        a.src = stream_src(rs);
        a.src.lay = rs->d_lay; a.src.n_lay = rs->n_lay;
        a.pt = tcmi_mask_args(rs);
        a.cols = reinterpret_cast<const int32_t *>(d);
        a.cov = a.cols + n;
        a.totals = reinterpret_cast<int32_t *>(d + b_in);
        a.hdr = reinterpret_cast<IeHdr *>(d + b_in + b_tot);
        a.keys = reinterpret_cast<u64 *>(d + b_in + b_tot + b_hdr);
        a.cnt = reinterpret_cast<uint32_t *>(d + b_in + b_tot + b_hdr + b_keys);
        a.rep = reinterpret_cast<u64 *>(d + b_in + b_zero);
        a.events = reinterpret_cast<tcmi_indel_event *>(d + b_in + b_zero + b_rep);
        a.text = d + b_in + b_zero + b_rep + b_ev;
        a.n = (int32_t)n;
        a.seed = seed;
        a.bits = opt->indel_hash_bits;
        a.slot_mask = (uint32_t)(S - 1);
        if (rule) a.rule = *rule;
        a.apply_rule = rule != nullptr;
        a.ev_cap = (uint32_t)ev_cap;
        a.text_cap = text_cap;
        TCMI_HIP(ctx, hipMemcpyAsync(d, pin, 8 * n, hipMemcpyHostToDevice, ctx->stream));
        TCMI_HIP(ctx, hipMemsetAsync(d + b_in, 0, b_zero, ctx->stream));
        TCMI_HIP(ctx, hipMemsetAsync(a.rep, 0xFF, b_rep, ctx->stream));     // (a minimum starts at the largest value)
        if (rs->n_reads > 0) {
            const int64_t wgs = (int64_t)std::max(ctx->n_cu, 1) * SC_WG_PER_CU;
            const unsigned grid = (unsigned)std::min<int64_t>((rs->n_reads + BLOCK - 1) / BLOCK, wgs);
            const unsigned grid3 = (unsigned)std::min<int64_t>(((int64_t)S + BLOCK - 1) / BLOCK, wgs);
            (void)hipGetLastError();                        // drop any stale error of this thread
            tcmi_prof_begin(ctx, TCMI_K_INDEL_EVENTS);
            hipLaunchKernelGGL(indel_count_kernel, dim3(grid), dim3(BLOCK), 0, ctx->stream, a);
            hipLaunchKernelGGL(indel_verify_kernel, dim3(grid), dim3(BLOCK), 0, ctx->stream, a);
            hipLaunchKernelGGL(indel_gather_kernel, dim3(grid3), dim3(BLOCK), 0, ctx->stream, a);
            tcmi_prof_end(ctx, TCMI_K_INDEL_EVENTS);
            TCMI_HIP(ctx, hipGetLastError());
        }
        // the header and the totals in one copy (they lie side by side: totals | header)
        TCMI_HIP(ctx, hipMemcpyAsync(pin + b_in, d + b_in, b_tot + b_hdr, hipMemcpyDeviceToHost, ctx->stream));
        TCMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
        std::memcpy(&hdr, pin + b_in + b_tot, sizeof hdr);
        if (hdr.too_long)
            return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "%s: a record inserts more than 2^30 bases at one column", what);
        if (hdr.overflow) {
            if (slots_log >= MAX_SLOTS_LOG)
                return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "%s: the device table overflowed at its largest size, 2^%d slots: too many distinct events at the queried columns", what, MAX_SLOTS_LOG);
            slots_log = std::min(slots_log + 3, MAX_SLOTS_LOG);
            ++opt->stat_indel_grown;
            continue;
        }
        if (hdr.collisions | hdr.missing) {
            if (hdr.missing && !hdr.collisions)
                return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "%s: %u insertions did not find the slot they were counted in", what, hdr.missing);
            if (++seed >= (uint32_t)TCMI_INDEL_SEEDS)
                return tcmi_fail(ctx, TCMI_E_UNSUPPORTED, "%s: different insertions of one column shared a %d-bit hash under each of %d seeds", what, opt->indel_hash_bits, (int)TCMI_INDEL_SEEDS);
            ++opt->stat_indel_retried;
            continue;
        }
        if (hdr.n_events > ev_cap || hdr.text_used > text_cap) {   // (the lists outgrew their room: once more with what they need)
            ev_cap = std::max<size_t>(ev_cap, hdr.n_events);
            text_cap = std::max<size_t>(text_cap, (size_t)hdr.text_used);
            continue;
        }
        const int32_t *got = reinterpret_cast<const int32_t *>(pin + b_in);
        for (size_t k = 0; k < 2 * n; ++k) tot[k] += got[k];
        // the download: what the attempt found
        const size_t e_bytes = (size_t)hdr.n_events * sizeof(tcmi_indel_event), t_bytes = (size_t)hdr.text_used;
        if (e_bytes == 0) return TCMI_OK;
        char *pin2 = static_cast<char *>(tcmi_ctx_pinned(ctx, e_bytes + t_bytes));
        if (!pin2) return tcmi_fail(ctx, TCMI_E_NOMEM, "%s: pinned scratch", what);
        TCMI_HIP(ctx, hipMemcpyAsync(pin2, a.events, e_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (t_bytes) TCMI_HIP(ctx, hipMemcpyAsync(pin2 + e_bytes, a.text, t_bytes, hipMemcpyDeviceToHost, ctx->stream));
        TCMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
        try {
            out.ev.resize(hdr.n_events);
            std::memcpy(out.ev.data(), pin2, e_bytes);
            out.text.assign(pin2 + e_bytes, t_bytes);
        } catch (...) {                                     // (no exception may cross the C ABI)
            return tcmi_fail(ctx, TCMI_E_NOMEM, "%s: no host memory for %u events", what, hdr.n_events);
        }
        return TCMI_OK;
    }
}

} // namespace

extern "C" int tcmi_readset_indel_events(tcmi_ctx *ctx, const tcmi_readset *rs, int64_t n, const int64_t *cols, const int32_t *cov, int64_t num, int64_t den,
                                         int32_t min_alt_depth, int32_t min_depth, tcmi_indel_event *events, int64_t cap, int64_t *n_found, char *text,
                                         int64_t text_cap, int64_t *text_len, tcmi_indel_totals *totals)
{
    if (n_found) *n_found = 0;
    if (text_len) *text_len = 0;
    if (!ctx || !rs) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    if (n < 1 || n > MAX_N) return tcmi_fail(ctx, TCMI_E_ARG, "indel events: %lld columns: 1..1048576 are allowed", (long long)n);
    if (!cols || !cov || !totals || !n_found || !text_len || cap < 0 || text_cap < 0 || (cap > 0 && !events) || (text_cap > 0 && !text))
        return tcmi_fail(ctx, TCMI_E_ARG, "indel events: null argument or negative capacity");
    const tcmi_var_rule rule = {num, den, min_alt_depth, min_depth};
    if (!tcmi_indel_rule_ok(rule))
        return tcmi_fail(ctx, TCMI_E_ARG, "indel events: min_af %lld / %lld, min_alt_depth %d, min_depth %d: den in 1..10^6, num in 0..den, min_alt_depth >= 1, min_depth >= 0",
                         (long long)num, (long long)den, min_alt_depth, min_depth);
    for (int64_t i = 0; i < n; ++i)
        if (cov[i] < 0) return tcmi_fail(ctx, TCMI_E_ARG, "indel events: the coverage of column %lld is negative (%d)", (long long)i, cov[i]);
    std::vector<int32_t> c32;
    if (const int rc = tcmi_count_columns(ctx, "indel events", n, cols, c32)) return rc;
    tcmi_indel_list merged;
    std::vector<int64_t> tot;
    try {
        tot.assign(2 * (size_t)n, 0);
        std::vector<tcmi_indel_list> lists(std::max<size_t>(rs->parts.size(), 1));
        if (rs->parts.empty()) {
            if (const int rc = indel_events_one(ctx, ctx, rs, c32, cov, &rule, lists[0], tot)) return rc;
        } else {
            // sub-ranges: whether an event is reported takes its count over all parts — every part without the rule, on its own
            // context, where its stream lives; a part's error is worded on the caller's context
            size_t k = 0;
            for (const tcmi_readset::Part &pt : rs->parts) {
                const int rc = indel_events_one(ctx, pt.cx, pt.rs, c32, cov, nullptr, lists[k++], tot);
                if (rc) return pt.cx == ctx ? rc : tcmi_fail(ctx, rc, "%s", pt.cx->err.c_str());
            }
        }
        if (!tcmi_indel_merge(lists, rs->parts.empty() ? nullptr : &rule, merged))
            return tcmi_fail(ctx, TCMI_E_HIP, "indel events: the device's event list does not fit its text");
    } catch (...) {                                         // (no exception may cross the C ABI)
        return tcmi_fail(ctx, TCMI_E_NOMEM, "indel events: no host memory");
    }
    for (int64_t i = 0; i < n; ++i) {
        totals[i].pos = (int32_t)cols[i];
        totals[i].ins_total = (int32_t)tot[2 * (size_t)i];
        totals[i].del_total = (int32_t)tot[2 * (size_t)i + 1];
        totals[i].reserved = 0;
    }
    *n_found = (int64_t)merged.ev.size();
    *text_len = (int64_t)merged.text.size();
    if (*n_found > cap || *text_len > text_cap) {
        if (!events && !text && cap == 0 && text_cap == 0) return TCMI_OK;   // the sizing call
        return tcmi_fail(ctx, TCMI_E_ARG, "indel events: %lld events and %lld letters do not fit the buffers (%lld, %lld)", (long long)*n_found, (long long)*text_len,
                         (long long)cap, (long long)text_cap);
    }
    if (*n_found) std::memcpy(events, merged.ev.data(), merged.ev.size() * sizeof(tcmi_indel_event));
    if (*text_len) std::memcpy(text, merged.text.data(), merged.text.size());
    return TCMI_OK;
}
