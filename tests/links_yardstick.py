"""The yardstick of --variant-links (tcmi_readset_link_counts, tcmi_link_phase, tcmi_variants_links_text), from committed yardsticks
only: the class of a record's token at a column is read off tests/primer_yardstick.counts applied to that single record
(tests/strand_yardstick.subset) — no second statement of the token rule —, the joint counts are accumulated here, the phase is the rule
of include/tcmi.h in Python's integers, the text builds on tests/variant_yardstick.text's spellings."""
import numpy as np

from tests import primer_yardstick as py
from tests import strand_yardstick as sy
from tests import variant_yardstick as vy

PHASES = ("CIS", "TRANS", "MIXED", "NONE", "LOW")
DTYPE = np.dtype([("j", np.int32, (7, 7)), ("a", np.int32), ("b", np.int32), ("reserved", np.int32)])
HEADER = "REGION\tPOS_A\tREF_A\tALT_A\tPOS_B\tREF_B\tALT_B\tSPAN\tBOTH\tONLY_A\tONLY_B\tNEITHER\tPHASE\n"


def classes(rd, L, table=(), q=0, slack=0, shift=0, n_pos=None):
    """-> uint8 [records, n_pos]: per record of the flat arrays `rd` and per column of the reference the class of its token: 0 none, 1..4
    counted on plane A, T, C, G, 5 on X, 6 on coverage and none of those — from the matrix primer_yardstick.counts gives for that
    record alone.  n_pos: the columns wanted (default: the extent of all records)."""
    n = int(rd["n_reads"])
    if n_pos is None:
        n_pos = len(py.counts(rd, L, table, q, slack, shift)[0])
    out = np.zeros((n, n_pos), np.uint8)
    keep = np.zeros(n, bool)
    for i in range(n):
        keep[:] = False
        keep[i] = True
        m = py.counts(sy.subset(rd, keep), L, table, q, slack, shift)[0][:n_pos]
        assert m.max(initial=0) <= 1 and (m[:, 1:6].sum(1) <= m[:, 0]).all(), "one record adds at most one token a column, to coverage and at most one plane of A..X"
        cls = np.where(m[:, 0] == 0, 0, np.where(m[:, 1:6].any(1), 1 + np.argmax(m[:, 1:6], axis=1), 6))
        out[i, :len(cls)] = cls
    return out


def joint(cls, cols, k):
    """class matrix [records, n_pos], ascending columns (beyond n_pos: class 0 for everybody), k -> int32 [len(cols) * k, 7, 7]:
    entry i * k + d - 1 is the pair (cols[i], cols[i + d]); j[0][0] is 0; all zero where i + d >= len(cols)"""
    n = len(cols)
    at = np.zeros((cls.shape[0], n), np.int64)
    for c_i, c in enumerate(cols):
        if 0 <= c < cls.shape[1]:
            at[:, c_i] = cls[:, c]
    j = np.zeros((n * k, 49), np.int64)
    for d in range(1, k + 1):
        if n - d <= 0:
            continue
        key = (np.arange(n - d)[None, :] * k + d - 1) * 49 + at[:, :n - d] * 7 + at[:, d:]
        j += np.bincount(key.reshape(-1), minlength=n * k * 49).reshape(n * k, 49)
    j[:, 0] = 0
    return j.reshape(n * k, 7, 7).astype(np.int32)


def records(cols, k, j):
    n = len(cols)
    out = np.zeros(n * k, DTYPE)
    for i in range(n):
        for d in range(1, k + 1):
            out[i * k + d - 1] = (j[i * k + d - 1], cols[i], cols[i + d] if i + d < n else -1, 0)
    return out


def marginals(j, cols, k):
    """-> (first, second): int64 [n * k, 7] the row sums (classes at the pair's first column) and the column sums (at its second)"""
    return j.astype(np.int64).sum(2), j.astype(np.int64).sum(1)


def classes_of_matrix(matrix, cols):
    """rows `cols` of an [extent, 7] count matrix -> int64 [n, 7]: what the marginals of a pair must be at that column in classes 1..6
    (index 0 is left 0: the records without a token there are not in the matrix)"""
    m = sy.at(matrix, cols).astype(np.int64)
    out = np.zeros((len(cols), 7), np.int64)
    out[:, 1:6] = m[:, 1:6]
    out[:, 6] = m[:, 0] - m[:, 1:6].sum(1)
    return out


def invariant(recs, k, matrix):
    """'' when every pair with b >= 0 of the link records adds up to the count matrix at both its columns, else the first that does not"""
    recs = np.asarray(recs)
    for r in recs:
        if r["b"] < 0:
            if r["j"].any():
                return "pair (%d, -1) holds counts" % r["a"]
            continue
        j = r["j"].astype(np.int64)
        for name, col, got in (("a", int(r["a"]), j.sum(1)), ("b", int(r["b"]), j.sum(0))):
            want = classes_of_matrix(matrix, [col])[0]
            if got[1:].tolist() != want[1:].tolist():
                return "pair (%d, %d): classes 1..6 at %s = %d sum to %r, the matrix says %r" % (r["a"], r["b"], name, col, got[1:].tolist(), want[1:].tolist())
        if j[0, 0]:
            return "pair (%d, %d): j[0][0] = %d" % (r["a"], r["b"], j[0, 0])
    return ""


def phase(both, only_a, only_b, span, min_depth, num, den):
    if span < min_depth:
        return 4
    m = min(both + only_a, both + only_b)
    if m == 0:
        return 3
    if both * den >= num * m:
        return 0
    if both * den <= (den - num) * m:
        return 1
    return 2


def sums(j, a, b):
    """a pair's 7 x 7 counts, the two alleles' classes -> (span, both, only_a, only_b, neither)"""
    j = [[int(v) for v in row] for row in j]
    span = sum(j[x][y] for x in range(1, 7) for y in range(1, 7))
    both = j[a][b]
    only_a = sum(j[a][y] for y in range(1, 7) if y != b)
    only_b = sum(j[x][b] for x in range(1, 7) if x != a)
    return span, both, only_a, only_b, span - both - only_a - only_b


def text(recs, links, k, region, ref, min_depth, num, den, pos_offset=0):
    """recs: [(pos, allele, count, cov)] ascending; links: {(pos_a, pos_b): 7 x 7 counts} -> the rows of --variant-links: one per pair
    of records at most k distinct positions apart, both alleles in planes 1..5"""
    pos = sorted({p for p, *_ in recs})
    lines = vy.text(recs, region, ref, pos_offset).splitlines()
    field = [ln.split("\t") for ln in lines]                    # REGION POS REF ALT ...: the spellings
    rows = []
    for i1, (p1, a1, *_) in enumerate(recs):
        for i2, (p2, a2, *_) in enumerate(recs):
            d = pos.index(p2) - pos.index(p1)
            if not 1 <= d <= k or a1 > 5 or a2 > 5:
                continue
            span, both, only_a, only_b, neither = sums(links[(p1, p2)], a1, a2)
            rows.append("\t".join(field[i1][:4] + field[i2][1:4] + [str(v) for v in (span, both, only_a, only_b, neither)] +
                                  [PHASES[phase(both, only_a, only_b, span, min_depth, num, den)]]) + "\n")
    return "".join(rows)
