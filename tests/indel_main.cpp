// indel_main.cpp — a program of its own over csrc/indel_rule.h, csrc/cigar_host.h and csrc/indels_text.cpp and nothing else (no HIP, no
// GPU): tests/test_indel_rule.py builds it plain and with AddressSanitizer + UBSan and runs it as a program.  All numbers int64 unless said.
//   indel_main passes IN OUT   IN: n, then n x {count, cov, num, den, min_alt_depth, min_depth}.  OUT: n int32, tcmi_indel_passes' answers
//                              (checked here against the header's rule).
//   indel_main hash IN OUT     IN: n, then n x {seed, bits, len, len bytes (one nibble each)}.  OUT: n uint64, tcmi_indel_hash's answers
//                              (checked here against the header's base-by-base form).
//   indel_main walk IN OUT     IN: n, then n x {n_cigar, k, y, n_cigar uint32 words}.  OUT: per case len, then len query indices: the host
//                              twin of the kernels' walk over the inserted bases (tcmi_cigar::ins_bases); len must be indel_after's.
//   indel_main merge IN OUT    IN: {n_parts, with_rule, num, den, min_alt_depth, min_depth}, per part {n, text_len, n tcmi_indel_event,
//                              text}.  OUT: {ok, n, text_len}, the merged events, their text (tcmi_indel_merge).
//   indel_main text IN OUT     IN: {n, text_len, n_cols, n_records, pos_offset, n_region, n_ref}, the region's bytes, the reference's,
//                              the text, n tcmi_indel_event, n_cols tcmi_indel_totals, n_records tcmi_variant.  OUT: "rc len\n" of the
//                              call with a buffer of exactly the sizing call's length, then the rows.  The sizing call, a buffer one
//                              byte short (TCMI_E_ARG, the same *len) and a buffer with room to spare whose tail must stay untouched
//                              are checked here.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../trueconsense_amd/csrc/cigar_host.h"
#include "../trueconsense_amd/csrc/indel_rule.h"

static bool read_all(const char *path, std::vector<char> &buf)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    char tmp[65536];
    size_t m;
    while ((m = std::fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + m);
    std::fclose(f);
    return true;
}

static int fail(const char *what)
{
    std::printf("FAILED: %s\n", what);
    return 1;
}

// the input, taken piece by piece; ok turns false for good when a piece is not there
struct In {
    std::vector<char> buf;
    size_t at = 0;
    bool ok = true;
    const char *take(size_t m)
    {
        if (!ok || m > buf.size() - at) { ok = false; return nullptr; }
        const char *p = buf.data() + at;
        at += m;
        return p;
    }
    int64_t i64()
    {
        int64_t v = 0;
        if (const char *p = take(8)) std::memcpy(&v, p, 8);
        return v;
    }
    template <class T> bool array(std::vector<T> &out, int64_t n)
    {
        if (n < 0 || (uint64_t)n > buf.size()) { ok = false; return false; }
        out.resize((size_t)n);
        const char *p = take((size_t)n * sizeof(T));
        if (p && n) std::memcpy(out.data(), p, (size_t)n * sizeof(T));
        return ok;
    }
};

int main(int argc, char **argv)
{
    if (argc != 4) return fail("usage: indel_main passes|hash|walk|merge|text IN OUT");
    In in;
    if (!read_all(argv[2], in.buf)) return fail("cannot read IN");
    FILE *out = std::fopen(argv[3], "wb");
    if (!out) return fail("cannot open OUT");
    const std::string mode = argv[1];
    if (mode == "passes") {
        const int64_t n = in.i64();
        std::vector<int64_t> v;
        if (!in.array(v, 6 * n)) return fail("passes: IN is short");
        std::vector<int32_t> got((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            const int64_t *c = v.data() + 6 * i;
            got[(size_t)i] = tcmi_indel_passes((int32_t)c[0], (int32_t)c[1], c[2], c[3], (int32_t)c[4], (int32_t)c[5]);
            const tcmi_var_rule r = {c[2], c[3], (int32_t)c[4], (int32_t)c[5]};
            if (got[(size_t)i] >= 0 && got[(size_t)i] != (int)tcmi_indel_rule_passes((int32_t)c[0], (int32_t)c[1], r)) return fail("the ABI's answer is not the header's");
        }
        std::fwrite(got.data(), 4, got.size(), out);
        std::printf("ok %lld rules\n", (long long)n);
    } else if (mode == "hash") {
        const int64_t n = in.i64();
        std::vector<uint64_t> got;
        for (int64_t i = 0; i < n; ++i) {
            const int64_t seed = in.i64(), bits = in.i64(), len = in.i64();
            std::vector<uint8_t> nib;
            if (!in.array(nib, len)) return fail("hash: IN is short");
            got.push_back(tcmi_indel_hash((uint32_t)seed, (int32_t)len, nib.data(), (int32_t)bits));
            uint64_t h = tcmi_indel_hash_begin((uint32_t)seed);
            for (uint8_t b : nib) h = tcmi_indel_hash_step(h, b);
            if (tcmi_indel_hash_end(h, len, (int)bits) != got.back()) return fail("the ABI's hash is not the header's");
            if (got.back() >> 34) return fail("a hash of more than 34 bits");
        }
        std::fwrite(got.data(), 8, got.size(), out);
        std::printf("ok %lld hashes\n", (long long)n);
    } else if (mode == "walk") {
        const int64_t n = in.i64();
        for (int64_t i = 0; i < n; ++i) {
            const int64_t n_cigar = in.i64(), k = in.i64(), y = in.i64();
            std::vector<uint32_t> cg;
            if (!in.array(cg, n_cigar) || k < 0 || k >= n_cigar) return fail("walk: IN is short");
            std::vector<int64_t> idx;
            const int64_t len = tcmi_cigar::ins_bases(cg.data(), n_cigar, k, y, [&](int64_t qi) { idx.push_back(qi); });
            const int64_t peek = tcmi_cigar::indel_after(cg.data(), n_cigar, k);
            if (len != (int64_t)idx.size() || len != (peek > 0 ? peek : 0)) return fail("the walk's length is not indel_after's");
            std::fwrite(&len, 8, 1, out);
            std::fwrite(idx.data(), 8, idx.size(), out);
        }
        std::printf("ok %lld walks\n", (long long)n);
    } else if (mode == "merge") {
        const int64_t n_parts = in.i64(), with_rule = in.i64();
        tcmi_var_rule rule;
        rule.num = in.i64(); rule.den = in.i64(); rule.min_alt_depth = (int32_t)in.i64(); rule.min_depth = (int32_t)in.i64();
        if (!in.ok || n_parts < 0 || n_parts > 64) return fail("merge: IN has no header");
        std::vector<tcmi_indel_list> parts((size_t)n_parts);
        for (tcmi_indel_list &p : parts) {
            const int64_t n = in.i64(), text_len = in.i64();
            std::vector<char> text;
            if (!in.array(p.ev, n) || !in.array(text, text_len)) return fail("merge: IN is short");
            p.text.assign(text.data(), text.size());
        }
        tcmi_indel_list merged;
        const int64_t ok = tcmi_indel_merge(parts, with_rule ? &rule : nullptr, merged);
        const int64_t head[3] = {ok, (int64_t)merged.ev.size(), (int64_t)merged.text.size()};
        std::fwrite(head, 8, 3, out);
        if (ok) {
            std::fwrite(merged.ev.data(), sizeof(tcmi_indel_event), merged.ev.size(), out);
            std::fwrite(merged.text.data(), 1, merged.text.size(), out);
        }
        std::printf("ok %lld parts\n", (long long)n_parts);
    } else if (mode == "text") {
        int64_t h[7];
        for (int64_t &v : h) v = in.i64();
        std::vector<char> region, text;
        std::vector<uint8_t> ref;
        std::vector<tcmi_indel_event> ev;
        std::vector<tcmi_indel_totals> tot;
        std::vector<tcmi_variant> recs;
        if (!in.ok || !in.array(region, h[5]) || !in.array(ref, h[6]) || !in.array(text, h[1]) || !in.array(ev, h[0]) || !in.array(tot, h[2]) || !in.array(recs, h[3]))
            return fail("text: IN is short");
        region.push_back(0);
        const auto call = [&](char *buf, int64_t cap, int64_t *len) {
            return tcmi_indels_text(ev.empty() ? nullptr : ev.data(), h[0], text.empty() ? nullptr : text.data(), h[1], tot.empty() ? nullptr : tot.data(), h[2],
                                    recs.empty() ? nullptr : recs.data(), h[3], region.data(), h[4], ref.empty() ? nullptr : ref.data(), h[6], buf, cap, len);
        };
        int64_t need = -1;
        const int rc0 = call(nullptr, 0, &need);
        if (rc0) {
            if (need != 0) return fail("a refused call left a length");
            std::fprintf(out, "%d 0\n", rc0);
        } else {
            std::vector<char> exact((size_t)need + 1, '#'), spare((size_t)need + 64, '#');
            int64_t len = -1;
            const int rc = call(exact.data(), need, &len);
            if (rc || len != need || exact[(size_t)need] != '#') return fail("the exact buffer");
            if (need > 0) {
                std::vector<char> tight((size_t)need, '#');
                int64_t len1 = -1;
                if (call(tight.data(), need - 1, &len1) != TCMI_E_ARG || len1 != need || tight[(size_t)need - 1] != '#') return fail("a buffer one byte short");
            }
            int64_t len2 = -1;
            if (call(spare.data(), need + 63, &len2) || len2 != need || std::memcmp(spare.data(), exact.data(), (size_t)need)) return fail("the spare buffer");
            for (size_t k = (size_t)need; k < spare.size(); ++k)
                if (spare[k] != '#') return fail("the spare buffer's tail was written");
            std::fprintf(out, "%d %lld\n", rc, (long long)len);
            std::fwrite(exact.data(), 1, (size_t)need, out);
        }
        std::printf("ok text\n");
    } else return fail("passes, hash, walk, merge or text");
    std::fclose(out);
    return 0;
}
