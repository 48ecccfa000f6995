// outputs_main.cpp — csrc/outputs_text.cpp (the native writers of --batch) as a program of its own (tests/test_outputs_text.py
// builds it with a plain compiler under AddressSanitizer + UBSan and runs it as a child process; no GPU, no HIP header, no other
// product source).
//   outputs_main < CASE
// CASE: lines "key value"; in a value "\n", "\t" and "\\" are spelled with a backslash.  The first line is "mode M":
//   int    ints V...                                                            tcmi_put_int of each, one per line
//   tsv    ints COV...                                                          tcmi_coverage_tsv_text (L = their number)
//   gff    head, name, ns V..., ne V..., col (6 per row, in order)              tcmi_gff_text
//   vcf    head, refid, ref, cons, ints COV..., mincov, inspos, insoff, insseq  tcmi_vcf_text
//   write  path, text                                                           tcmi_write_file
// Output: "code N\n", "why WORDS\n" (escaped alike), then the text as it is, to the end of the output.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../trueconsense_amd/csrc/outputs_text.h"

static std::string unescape(const std::string &s)
{
    std::string o;
    for (size_t i = 0; i < s.size(); ++i) {
        if (s[i] != '\\' || i + 1 == s.size()) { o.push_back(s[i]); continue; }
        const char c = s[++i];
        o.push_back(c == 'n' ? '\n' : c == 't' ? '\t' : c);
    }
    return o;
}

static std::string escape(const std::string &s)
{
    std::string o;
    for (char c : s) {
        if (c == '\n') o += "\\n";
        else if (c == '\t') o += "\\t";
        else if (c == '\\') o += "\\\\";
        else o.push_back(c);
    }
    return o;
}

static std::vector<long long> ints(const std::string &s)
{
    std::vector<long long> v;
    std::istringstream in(s);
    std::string w;
    while (in >> w) v.push_back(std::strtoll(w.c_str(), nullptr, 10));
    return v;
}

int main()
{
    std::map<std::string, std::string> one;
    std::vector<std::string> cols;
    std::string line;
    while (std::getline(std::cin, line)) {
        const size_t sp = line.find(' ');
        const std::string key = line.substr(0, sp), value = sp == std::string::npos ? "" : unescape(line.substr(sp + 1));
        if (key == "col") cols.push_back(value);
        else one[key] = value;
    }
    const std::string mode = one["mode"];
    std::vector<int32_t> cov;
    for (long long v : ints(one["ints"])) cov.push_back((int32_t)v);
    std::string text, why;
    int rc = TCMI_OK;
    if (mode == "int") {
        for (long long v : ints(one["ints"])) { tcmi_put_int(text, v); text.push_back('\n'); }
    } else if (mode == "tsv") {
        text = "left over";                                     // (the writer starts from nothing)
        tcmi_coverage_tsv_text(cov.data(), (int64_t)cov.size(), text);
    } else if (mode == "gff") {
        std::vector<int64_t> ns, ne;
        for (long long v : ints(one["ns"])) ns.push_back(v);
        for (long long v : ints(one["ne"])) ne.push_back(v);
        if (ns.size() != ne.size() || cols.size() != 6 * ns.size()) { std::fprintf(stderr, "gff: %zu starts, %zu ends, %zu columns\n", ns.size(), ne.size(), cols.size()); return 2; }
        tcmi_gff_text(one["head"], cols, one["name"].c_str(), ns, ne, text);
    } else if (mode == "vcf") {
        tcmi_inserts ins;
        for (long long v : ints(one["inspos"])) ins.pos.push_back(v);
        for (long long v : ints(one["insoff"])) ins.off.push_back(v);
        ins.seq = one["insseq"];
        if (ins.off.size() != ins.pos.size() + 1 || ins.off.back() != (int64_t)ins.seq.size()) { std::fprintf(stderr, "vcf: inconsistent inserts\n"); return 2; }
        rc = tcmi_vcf_text(one["head"], one["refid"], one["ref"], one["cons"], cov.data(), (int64_t)cov.size(), (int32_t)std::atoi(one["mincov"].c_str()), ins,
                           text, why);
        if (rc) text.clear();                                   // (what a refused scan had written so far is nobody's)
    } else if (mode == "write") {
        rc = tcmi_write_file(one["path"].c_str(), one["text"], why);
    } else {
        std::fprintf(stderr, "unknown mode '%s'\n", mode.c_str());
        return 2;
    }
    std::printf("code %d\nwhy %s\n", rc, escape(why).c_str());
    std::fwrite(text.data(), 1, text.size(), stdout);
    return 0;
}
