// amplicons_text.cpp — the ONE writer of the amplicon table's rows (include/tcmi.h: tcmi_amplicons_text).  HOST only, re-entrant, no
// HIP header: the command line calls it through the C ABI, and tests/amplicons_main.cpp links it into a program of its own.
#include <cstdio>
#include <cstring>

#include "../../include/tcmi.h"

extern "C" int tcmi_amplicons_text(const tcmi_interval_stat *records, int64_t n, const char *sample, const char *region, const char *const *names,
                                   const char *const *pools, const int64_t *start, int64_t pos_offset, char *text, int64_t cap, int64_t *len)
{
    if (len) *len = 0;
    if (n < 0 || cap < 0 || pos_offset < 0 || !sample || !region || !len || (n > 0 && (!records || !names || !pools || !start)) || (cap > 0 && !text))
        return TCMI_E_ARG;
    const size_t n_sample = std::strlen(sample), n_region = std::strlen(region);
    int64_t used = 0;
    bool fits = true;
    for (int64_t i = 0; i < n; ++i) {
        const tcmi_interval_stat &v = records[i];
        if (!names[i] || !pools[i] || start[i] < pos_offset || v.n < 0) return TCMI_E_ARG;
        if (v.n > 0 && (v.min_pos < start[i] || v.min_pos >= start[i] + v.n)) return TCMI_E_ARG;
        const long long first = (long long)(start[i] - pos_offset + 1);
        char row[192];              // (everything behind the pool: at most 7 integers of 20 characters, a mean below 2^31 and eight separators)
        int m;
        if (v.n == 0)
            m = std::snprintf(row, sizeof row, "\t%lld\t%lld\t0\tNA\tNA\tNA\tNA\t0\n", first, first - 1);
        else
            m = std::snprintf(row, sizeof row, "\t%lld\t%lld\t%d\t%.2f\t%d\t%d\t%lld\t%d\n", first, first + v.n - 1, (int)v.n, (double)v.sum / (double)v.n,
                              (int)v.median, (int)v.min, (long long)(v.min_pos - pos_offset + 1), (int)v.below);
        if (m < 0 || m >= (int)sizeof row) return TCMI_E_ARG;
        const size_t n_name = std::strlen(names[i]), n_pool = std::strlen(pools[i]);
        const int64_t need = (int64_t)(n_sample + 1 + n_region + 1 + n_name + 1 + n_pool) + m;
        if (fits && used + need <= cap) {
            char *w = text + used;
            std::memcpy(w, sample, n_sample); w += n_sample; *w++ = '\t';
            std::memcpy(w, region, n_region); w += n_region; *w++ = '\t';
            std::memcpy(w, names[i], n_name); w += n_name; *w++ = '\t';
            std::memcpy(w, pools[i], n_pool); w += n_pool;
            std::memcpy(w, row, (size_t)m);
        } else fits = false;
        used += need;
    }
    *len = used;
    return fits || !text ? TCMI_OK : TCMI_E_ARG;        // (text == NULL with cap = 0 is the sizing call: *len, and no refusal)
}
