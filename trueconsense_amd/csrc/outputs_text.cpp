// outputs_text.cpp — HOST: the coverage TSV, the corrected GFF and the VCF of one sample as text, and the file they go to
// (outputs_text.h).  The native writers of --batch: pipeline.cpp's walk stage calls them, tests/outputs_main.cpp runs them alone.
#include "outputs_text.h"

#include <algorithm>
#include <cctype>
#include <cstdarg>
#include <cstdio>

namespace {

// the code, with the words as tcmi_fail would keep them
int refuse(std::string &why, int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    why = buf;
    return code;
}

void vcf_row(std::string &o, const std::string &ref_id, int64_t pos, const std::string &ref_allele, const std::string &alt, long long dp, bool indel)
{
    o += ref_id; o.push_back('\t'); tcmi_put_int(o, pos); o += "\t.\t"; o += ref_allele; o.push_back('\t'); o += alt;
    o += "\t.\tPASS\tDP="; tcmi_put_int(o, dp); o += indel ? ";INDEL\n" : "\n";
}

} // namespace

void tcmi_put_int(std::string &o, long long v)
{
    char b[24];
    int n = 0;
    const bool neg = v < 0;
    unsigned long long u = neg ? 0ull - (unsigned long long)v : (unsigned long long)v;
    do { b[n++] = (char)('0' + u % 10); u /= 10; } while (u);
    if (neg) o.push_back('-');
    while (n) o.push_back(b[--n]);
}

void tcmi_coverage_tsv_text(const int32_t *cov, int64_t L, std::string &o)
{
    o.clear();
    o.reserve((size_t)L * 12);
    for (int64_t i = 0; i < L; ++i) { tcmi_put_int(o, i + 1); o.push_back('\t'); tcmi_put_int(o, cov[i]); o.push_back('\n'); }
}

void tcmi_gff_text(const std::string &head, const std::vector<std::string> &row_cols, const char *name, const std::vector<int64_t> &ns,
                   const std::vector<int64_t> &ne, std::string &o)
{
    o = head;
    for (size_t k = 0; k < ns.size(); ++k) {
        const std::string *c = &row_cols[6 * k];            // source, type, score, strand, phase, attributes
        o += name; o.push_back('\t'); o += c[0]; o.push_back('\t'); o += c[1]; o.push_back('\t');
        tcmi_put_int(o, ns[k]); o.push_back('\t'); tcmi_put_int(o, ne[k]); o.push_back('\t');
        o += c[2]; o.push_back('\t'); o += c[3]; o.push_back('\t'); o += c[4]; o.push_back('\t'); o += c[5]; o.push_back('\n');
    }
}

// One left-to-right scan.  The quirks are upstream's: raw reference characters against the upper-cased insert-free
// consensus, DP from the FOLLOWING position, POS of indel records one less than their index + 1, an insert matched by 0-based index ==
// its 1-based position, Python's index -1 (the last element) for a deletion at the very first position.  -> TCMI_E_KEYERROR where
// upstream raises (a deletion run that reaches the end of the consensus: IndexError; a coverage look-up beyond the index: KeyError).
int tcmi_vcf_text(const std::string &head, const std::string &ref_id, const std::string &ref, const std::string &cons_noinsert,
                  const int32_t *cov, int64_t L, int32_t mincov, const tcmi_inserts &ins, std::string &o, std::string &why)
{
    std::string cons = cons_noinsert;
    for (char &c : cons) c = (char)std::toupper((unsigned char)c);
    const int64_t n = (int64_t)ref.size(), nc = (int64_t)cons.size();
    o = head;
    auto coverage = [&](int64_t pos1, long long *out) {
        if (pos1 >= 1 && pos1 <= L) { *out = cov[pos1 - 1]; return TCMI_OK; }
        return refuse(why, TCMI_E_KEYERROR, "VCF: no coverage for position %lld (KeyError upstream)", (long long)pos1);
    };
    size_t next_ins = 0;
    int64_t i = 0;
    while (i < n) {
        if (i >= nc) return refuse(why, TCMI_E_KEYERROR, "VCF: the consensus ends at %lld, the reference at %lld (IndexError upstream)", (long long)nc, (long long)n);
        const char here = cons[(size_t)i];
        int64_t step = 1;
        long long dp = 0;
        if (here == '-') {
            int64_t j = i;
            while (j < nc && cons[(size_t)j] == '-') ++j;
            if (j >= nc) return refuse(why, TCMI_E_KEYERROR, "VCF: a deletion runs to the end of the consensus (IndexError upstream)");
            if (coverage(i + 1, &dp)) return TCMI_E_KEYERROR;
            // (a Python slice: cut at the reference's end)
            vcf_row(o, ref_id, i, ref[(size_t)((i - 1 + n) % n)] + ref.substr((size_t)i, (size_t)(std::min(j, n) - i)),
                    std::string(1, cons[(size_t)((i - 1 + nc) % nc)]), dp, true);
            step = j - i;
        } else if (here != ref[(size_t)i]) {
            if (coverage(std::max<int64_t>(i, 1) + 1, &dp)) return TCMI_E_KEYERROR;
            vcf_row(o, ref_id, i + 1, std::string(1, ref[(size_t)i]), std::string(1, here), dp, false);
        }
        while (next_ins < ins.pos.size() && ins.pos[next_ins] < i) ++next_ins;
        if (next_ins < ins.pos.size() && ins.pos[next_ins] == i) {
            if (coverage(i + 1, &dp)) return TCMI_E_KEYERROR;
            if (dp > mincov)
                vcf_row(o, ref_id, i, std::string(1, ref[(size_t)i]),
                        here + ins.seq.substr((size_t)ins.off[next_ins], (size_t)(ins.off[next_ins + 1] - ins.off[next_ins])), dp, true);
        }
        i += step;
    }
    return TCMI_OK;
}

int tcmi_write_file(const char *path, const std::string &text, std::string &why)
{
    FILE *fp = std::fopen(path, "wb");
    if (!fp) return refuse(why, TCMI_E_IO, "cannot write %s", path);
    const size_t w = std::fwrite(text.data(), 1, text.size(), fp);
    if (std::fclose(fp) != 0 || w != text.size()) return refuse(why, TCMI_E_IO, "short write to %s", path);
    return TCMI_OK;
}
