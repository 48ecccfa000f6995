// outputs_text.h — HOST: the three other outputs of the command line as text, the way --batch writes them per sample without Python
// (pipeline.cpp's walk stage): the coverage TSV (Coverage.py:1-16), the corrected GFF (Outputs.py:13-71) and the VCF (Outputs.py:104-180).
// Plain inputs, plain text out: no HIP header, no context, nothing of tcmi_internal.h, re-entrant — so a program of its own runs them
// under a sanitizer (tests/outputs_main.cpp, tests/test_outputs_text.py).  A writer that can fail returns the code and leaves the
// words in `why`; the caller hands them to tcmi_fail.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/tcmi.h"

// the accepted inserts of a walk: 1-based positions in ascending order, insert k's bases at seq[off[k] .. off[k + 1])
struct tcmi_inserts {
    std::vector<int64_t> pos, off;
    std::string seq;
};

void tcmi_put_int(std::string &o, long long v);

// Coverage.BuildCoverage: "{pos}\t{coverage}\n" for every position of the index
void tcmi_coverage_tsv_text(const int32_t *cov, int64_t L, std::string &o);

// Outputs.WriteGFF: the header text verbatim, then one line per row — seqid = the sample's name (TrueConsense.py:240), start / end as
// the walk corrected them, the other columns as the caller folded them (Outputs.py:32-58): 6 strings per row
void tcmi_gff_text(const std::string &head, const std::vector<std::string> &row_cols, const char *name, const std::vector<int64_t> &ns,
                   const std::vector<int64_t> &ne, std::string &o);

// Outputs.py:115-180 (the Python twin: trueconsense_amd/Outputs.py vcf_text) -> TCMI_OK, or TCMI_E_KEYERROR where upstream raises
int tcmi_vcf_text(const std::string &head, const std::string &ref_id, const std::string &ref, const std::string &cons_noinsert,
                  const int32_t *cov, int64_t L, int32_t mincov, const tcmi_inserts &ins, std::string &o, std::string &why);

// -> TCMI_OK or TCMI_E_IO
int tcmi_write_file(const char *path, const std::string &text, std::string &why);
