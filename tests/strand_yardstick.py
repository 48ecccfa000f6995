"""The yardstick of --variant-strand (tcmi_readset_strand_counts, tcmi_strand_verdict, tcmi_variants_strand_text), from committed
yardsticks only: the strand counts are tests/primer_yardstick.counts applied to the records without FLAG 0x10 and to those with it, the
verdict is the rule of include/tcmi.h in Python's integers, the text is tests/variant_yardstick.text with seven more fields."""
import numpy as np

from tests import primer_yardstick as py
from tests import variant_yardstick as vy

PER_READ = ("pos", "flag", "l_qseq", "tid", "mapq", "next_tid", "next_pos", "tlen")
RAGGED = (("cigar_off", "cigar"), ("seq_off", "seq"), ("qual_off", "qual"), ("name_off", "names"))
VERDICTS = ("PASS", "BIAS", "LOW")
DTYPE = np.dtype([("fwd", np.int32, (7,)), ("rev", np.int32, (7,)), ("pos", np.int32), ("reserved", np.int32)])


def subset(rd, keep):
    """the flat arrays (tcmi_reads layout) of the records at which the boolean array `keep` is true, in their order"""
    idx = np.nonzero(np.asarray(keep, bool))[0]
    out = {"n_reads": len(idx)}
    for k in PER_READ:
        if k in rd:
            out[k] = np.ascontiguousarray(np.asarray(rd[k])[idx])
    for off, data in RAGGED:
        if off not in rd:
            continue
        o = np.asarray(rd[off]).astype(np.int64)
        pieces = [np.asarray(rd[data])[o[i]:o[i + 1]] for i in idx]
        out[off] = np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).astype(np.uint64)
        out[data] = np.concatenate(pieces).astype(np.asarray(rd[data]).dtype) if pieces else np.zeros(0, np.asarray(rd[data]).dtype)
    return out


def at(matrix, cols):
    """rows `cols` of an [extent, 7] matrix, zeros beyond its extent -> int32 [n, 7]"""
    out = np.zeros((len(cols), 7), np.int32)
    for k, c in enumerate(cols):
        if 0 <= c < len(matrix):
            out[k] = matrix[c]
    return out


def counts(arrays, cols, L, table=(), q=0, slack=0, shift=0):
    """-> (fwd, rev) int32 [n, 7] at the columns `cols` (the reference's own): primer_yardstick.counts of the FLAG-0x10-clear records
    and of the FLAG-0x10-set records, everything else equal"""
    rev = (np.asarray(arrays["flag"]) & 0x10) != 0
    return tuple(at(py.counts(subset(arrays, m), L, table, q, slack, shift)[0], cols) for m in (~rev, rev))


def records(cols, fwd, rev):
    out = np.zeros(len(cols), DTYPE)
    if len(cols):
        out["fwd"], out["rev"], out["pos"] = fwd, rev, cols
    return out


def verdict(alt_fwd, alt_rev, tot_fwd, tot_rev, min_strand_depth, num, den):
    if tot_fwd < min_strand_depth or tot_rev < min_strand_depth:
        return 2
    x, y = alt_fwd * tot_rev, alt_rev * tot_fwd
    return 1 if min(x, y) * den < max(x, y) * num else 0


def verdict_in_64_bits(alt_fwd, alt_rev, tot_fwd, tot_rev, min_strand_depth, num, den):
    """the same rule with its last two products wrapped to 64 bits: what an implementation without 128-bit arithmetic computes"""
    if tot_fwd < min_strand_depth or tot_rev < min_strand_depth:
        return 2
    x, y = alt_fwd * tot_rev, alt_rev * tot_fwd
    return 1 if (min(x, y) * den) % (1 << 64) < (max(x, y) * num) % (1 << 64) else 0


def text(recs, strand, region, ref, min_strand_depth, num, den, pos_offset=0):
    """recs: [(pos, allele, count, cov)] ascending; strand: {pos: (fwd[7], rev[7])} -> the rows of --variant-strand"""
    plane = {"A": 1, "T": 2, "C": 3, "G": 4}
    rows = []
    for (pos, allele, count, cov), line in zip(recs, vy.text(recs, region, ref, pos_offset).splitlines()):
        fwd, rev = strand[pos]
        rp = plane.get(chr(ref[pos]).upper())
        v = verdict(int(fwd[allele]), int(rev[allele]), int(fwd[0]), int(rev[0]), min_strand_depth, num, den)
        rows.append("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n" % (line, fwd[rp] if rp else 0, rev[rp] if rp else 0, fwd[allele], rev[allele], fwd[0], rev[0], VERDICTS[v]))
    return "".join(rows)
