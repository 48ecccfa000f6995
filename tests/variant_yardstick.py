"""The variant table's rule (include/tcmi.h, tcmi_variants_dev) in plain Python integers: the yardstick of tests/test_variant_*.py.
It shares no code with the product."""
import numpy as np

DTYPE = np.dtype([("pos", np.int32), ("allele", np.int32), ("count", np.int32), ("cov", np.int32)])
ALT = "?ATCG*+"                     # a record's ALT by plane (coverage, A, T, C, G, X, I)


def records(counts, ref, num, den, min_alt_depth, min_depth):
    """counts [L, 7], ref bytes on the same axis, min_af = num / den -> [(pos, allele, count, cov)], by position, then allele"""
    out = []
    for p in range(min(len(counts), len(ref))):
        base = chr(ref[p]).upper()
        row = [int(x) for x in counts[p]]
        cov = row[0]
        if base not in "ACGT" or cov < max(min_depth, 1):
            continue
        for a in range(1, 7):
            if ALT[a] != base and row[a] >= min_alt_depth and row[a] * den >= num * cov:
                out.append((p, a, row[a], cov))
    return out


def as_array(recs):
    return np.array(recs, DTYPE) if len(recs) else np.zeros(0, DTYPE)


def text(recs, region, ref, pos_offset=0):
    """the table's rows (no header) for records on the axis of `ref`"""
    return "".join("%s\t%d\t%s\t%s\t%d\t%d\t%s\n" % (region, p - pos_offset + 1, chr(ref[p]).upper(), ALT[a], c, t, f"{c / t:.6f}")
                   for p, a, c, t in recs)
