// variants_text.cpp — the ONE writer of the variant table's rows (include/tcmi.h: tcmi_variants_text).  HOST only, re-entrant, no
// HIP header: the command line calls it through the C ABI, the file runner's walker threads call it directly, and
// tests/variants_main.cpp links it into a program of its own.
#include <cstdio>
#include <cstring>

#include "../../include/tcmi.h"

extern "C" int tcmi_variants_text(const tcmi_variant *records, int64_t n, const char *region, int64_t pos_offset, const uint8_t *ref,
                                  int64_t n_ref, char *text, int64_t cap, int64_t *len)
{
    if (len) *len = 0;
    if (n < 0 || cap < 0 || n_ref < 0 || pos_offset < 0 || !region || !len || (n > 0 && (!records || !ref)) || (cap > 0 && !text)) return TCMI_E_ARG;
    static const char alt_of[TCMI_NCOL] = {0, 'A', 'T', 'C', 'G', '*', '+'};
    const size_t n_region = std::strlen(region);
    int64_t used = 0;
    bool fits = true;
    for (int64_t i = 0; i < n; ++i) {
        const tcmi_variant &v = records[i];
        if (v.pos < pos_offset || v.pos >= n_ref || v.allele < TCMI_A || v.allele > TCMI_I || v.cov <= 0) return TCMI_E_ARG;
        char row[96];               // (everything behind the region: at most 3 numbers of 11 characters, a frequency below 2^31 and six separators)
        const int m = std::snprintf(row, sizeof row, "\t%lld\t%c\t%c\t%d\t%d\t%.6f\n", (long long)(v.pos - pos_offset + 1), (char)(ref[v.pos] & ~0x20),
                                    alt_of[v.allele], (int)v.count, (int)v.cov, (double)v.count / (double)v.cov);
        if (m < 0 || m >= (int)sizeof row) return TCMI_E_ARG;
        const int64_t need = (int64_t)n_region + m;
        if (fits && used + need <= cap) {
            std::memcpy(text + used, region, n_region);
            std::memcpy(text + used + n_region, row, (size_t)m);
        } else fits = false;
        used += need;
    }
    *len = used;
    return fits || !text ? TCMI_OK : TCMI_E_ARG;        // (text == NULL with cap = 0 is the sizing call: *len, and no refusal)
}
