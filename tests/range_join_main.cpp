// range_join_main.cpp — csrc/range_join.h as a program of its own (tests/test_range_join.py builds it with AddressSanitizer + UBSan).
// stdin: range tables, each `world inflated` and then `world` lines `first_block n_blocks first next`.
// stdout: one line per table: `ok`, or the rule's message, a tab and `who at want`.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../trueconsense_amd/csrc/range_join.h"

int main()
{
    int world = 0;
    int64_t inflated = 0;
    while (std::scanf("%d %" SCNd64, &world, &inflated) == 2) {
        if (world < 0) return 2;
        std::vector<int64_t> rg((size_t)world * 4);             // exactly the table: a read beyond it is the sanitizer's to find
        for (int64_t &v : rg)
            if (std::scanf("%" SCNd64, &v) != 1) return 2;
        int who = -1;
        int64_t at = -1, want = -1;
        const char *why = tcmi_ranges_join(reinterpret_cast<const int64_t (*)[4]>(rg.data()), world, inflated, &who, &at, &want);
        if (why) std::printf("%s\t%d %" PRId64 " %" PRId64 "\n", why, who, at, want);
        else std::printf("ok\n");
    }
    return 0;
}
