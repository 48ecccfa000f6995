"""The yardstick of --variant-evidence (tcmi_readset_evidence_counts, tcmi_evidence_verdict, tcmi_variants_evidence_text) in Python's
integers.  The counts come from a CIGAR walk of its own over the flat arrays of the records: per kept record (column, planes, quality,
MAPQ, end distance) as include/tcmi.h states them.  The walk is tied to the committed yardsticks wherever it is used: its (column,
quality) sequence must equal tc_oracle.read_tokens(..., with_qual=True) for every record, and its token counts must equal
tests/primer_yardstick.counts for every file (the mask is primer_yardstick.read_mask, the floor the same test).  The verdict and the
text are the rules of include/tcmi.h; the text's first seven fields are tests/variant_yardstick.text.  No tests in here."""
import numpy as np

from oracle import c_oracle
from oracle import tc_oracle as orc
from tests import primer_yardstick as py
from tests import strand_yardstick as sy
from tests import variant_yardstick as vy

DTYPE = np.dtype([("qual", np.int64, (7,)), ("mapq", np.int64, (7,)), ("dist", np.int64, (7,)), ("n", np.int32, (7,)), ("pos", np.int32)])
NAMES = ("LOWQ", "LOWMQ", "END")
COV, X, I = 0, 5, 6
PLANE_OF_NIBBLE = {1: 1, 8: 2, 2: 3, 4: 4}                                      # A T C G as BAM packs them -> the matrix's plane
M, INS, D, N, S, H, P, EQ, XM = range(9)
REF_OPS, QUERY_OPS, MATCH_OPS = (M, D, N, EQ, XM), (M, INS, S, EQ, XM), (M, EQ, XM)
CAP = 255
NONE = (0, 0, 0)                                                                # the read filter that filters nothing


def aligned_part(cigar):
    """[(op, length)] -> (a0, a1): a0 the S ops in front of the first op that is neither S nor H, a1 all query-consuming ops minus the S
    ops behind the last op that is neither S nor H"""
    inner = [k for k, (op, _) in enumerate(cigar) if op not in (S, H)]
    a0 = sum(n for op, n in cigar[:inner[0]] if op == S)
    tail = sum(n for op, n in cigar[inner[-1] + 1:] if op == S)
    return a0, sum(n for op, n in cigar if op in QUERY_OPS) - tail


def inserted_after(cigar, k):
    """the inserted bases reported on the last column of op k: the I ops behind it up to the next op that is neither I nor P when an I
    op follows directly, up to the next reference-consuming op when a P op follows"""
    if k + 1 >= len(cigar):
        return 0
    nxt = cigar[k + 1][0]
    tot = 0
    if nxt == INS:
        for op, n in cigar[k + 1:]:
            if op == INS:
                tot += n
            elif op != P:
                break
    elif nxt == P:
        for op, n in cigar[k + 2:]:
            if op == INS:
                tot += n
            elif op in REF_OPS:
                break
    return tot


def end_distance(qi, a0, a1):
    return min(CAP, max(0, min(qi - a0, a1 - 1 - qi)))


def tokens(rd, i):
    """record i (it piles up) -> [(column, planes, quality, MAPQ, end distance)] in column order, before floor and mask"""
    cigar = orc.read_cigar(rd, i)
    a0, a1 = aligned_part(cigar)
    l_seq, mapq = int(rd["l_qseq"][i]), int(rd["mapq"][i])
    q0 = int(rd["qual_off"][i])
    out = []
    x, y = int(rd["pos"][i]), 0
    for k, (op, n) in enumerate(cigar):
        if op in REF_OPS:
            ins = inserted_after(cigar, k) > 0
            for j in range(n):
                qi = y + j if op in MATCH_OPS else y
                planes = [COV]
                last_ins = ins and j == n - 1
                if op in MATCH_OPS:
                    nib = orc.read_base(rd, i, qi) if qi < l_seq else 15
                    if nib in PLANE_OF_NIBBLE:
                        planes.append(PLANE_OF_NIBBLE[nib])
                elif op == D and not last_ins:
                    planes.append(X)
                if last_ins:
                    planes.append(I)
                out.append((x + j, tuple(planes), int(rd["qual"][q0 + qi]) if qi < l_seq else 0, mapq, end_distance(qi, a0, a1)))
            x += n
        if op in QUERY_OPS:
            y += n
    want = [(c, q) for c, _, q in orc.read_tokens(rd, i, with_qual=True)]
    assert [(c, q) for c, _, q, _, _ in out] == want, ("the walk's columns and qualities are not the oracle's", i, cigar)
    return out


def passes(rd, i, f):
    """the read filter (min_mapq, require_flags, exclude_flags) on record i"""
    flag = int(rd["flag"][i])
    return int(rd["mapq"][i]) >= f[0] and (flag & f[1]) == f[1] and (flag & f[2]) == 0


def kept_tokens(rd, table=(), q=0, slack=0, shift=0, f=NONE):
    """every token the matrix counts, as (record index, token), record by record: of a record that piles up and passes the read
    filter, outside the record's primer mask and at or above the floor"""
    for i in range(int(rd["n_reads"])):
        if not orc.read_piles_up(rd, i) or not passes(rd, i, f):
            continue
        toks = tokens(rd, i)
        head_end, tail_start = py.read_mask(toks[0][0] + shift, toks[-1][0] + shift, table, slack)
        for t in toks:
            if head_end <= t[0] + shift < tail_start and t[2] >= q:
                yield i, t


def whole(rd, L, table=(), q=0, slack=0, shift=0, f=NONE):
    """-> (n, qual, mapq, dist) int64 [extent, 7] over every column of the reference's own axis, and per column the tokens at
    distance 0 and at the cap (int64 [extent] each); n must be primer_yardstick.counts of the records that pass f"""
    ok = [passes(rd, i, f) for i in range(int(rd["n_reads"]))]
    want = py.counts(rd if all(ok) else sy.subset(rd, ok), L, table, q, slack, shift)[0]
    n_pos = max(len(want), c_oracle.extent(rd, L))
    out = np.zeros((4, n_pos, 7), np.int64)
    marks = np.zeros((2, n_pos), np.int64)
    for _, (c, planes, qual, mapq, dist) in kept_tokens(rd, table, q, slack, shift, f):
        for pl in planes:
            out[:, c, pl] += (1, qual, mapq, dist)
        marks[0, c] += dist == 0
        marks[1, c] += dist == CAP
    assert np.array_equal(out[0][:len(want)], want) and not out[0][len(want):].any(), "the walk's token counts are not primer_yardstick.counts"
    return tuple(out), marks


def at(sums, cols):
    """rows `cols` of whole()'s four matrices (of any matrices of one shape), zeros beyond their extent -> as many int64 [n, 7]"""
    out = np.zeros((len(sums), len(cols), sums[0].shape[1]), np.int64)
    for k, c in enumerate(cols):
        if 0 <= c < len(sums[0]):
            out[:, k] = [m[c] for m in sums]
    return tuple(out)


def counts(rd, cols, L, table=(), q=0, slack=0, shift=0, f=NONE):
    """-> (n, qual, mapq, dist) int64 [len(cols), 7] at the columns `cols` (the reference's own)"""
    return at(whole(rd, L, table, q, slack, shift, f)[0], cols)


def records(cols, sums):
    out = np.zeros(len(cols), DTYPE)
    if len(cols):
        out["n"], out["qual"], out["mapq"], out["dist"], out["pos"] = sums[0], sums[1], sums[2], sums[3], cols
    return out


def verdict(n, qual, mapq, dist, min_qual, min_mapq, min_dist):
    return (1 if qual < min_qual * n else 0) | (2 if mapq < min_mapq * n else 0) | (4 if dist < min_dist * n else 0)


def verdict_in_32_bits(n, qual, mapq, dist, min_qual, min_mapq, min_dist):
    """the same rule with its products wrapped to 32 bits: what an implementation with int32 products computes"""
    wrap = lambda v: (v + (1 << 31)) % (1 << 32) - (1 << 31)
    return (1 if qual < wrap(min_qual * n) else 0) | (2 if mapq < wrap(min_mapq * n) else 0) | (4 if dist < wrap(min_dist * n) else 0)


def mean(total, n):
    t = 10 * int(total) // int(n) if n else 0
    return "%d.%d" % (t // 10, t % 10)


def word(bits):
    return ",".join(w for k, w in enumerate(NAMES) if bits >> k & 1) or "PASS"


def text(recs, ev, region, ref, min_qual, min_mapq, min_dist, pos_offset=0):
    """recs: [(pos, allele, count, cov)] ascending; ev: {pos: (n[7], qual[7], mapq[7], dist[7])} -> the rows of --variant-evidence"""
    plane = {"A": 1, "T": 2, "C": 3, "G": 4}
    rows = []
    for (pos, allele, count, cov), line in zip(recs, vy.text(recs, region, ref, pos_offset).splitlines()):
        n, qual, mapq, dist = ev[pos]
        assert n[allele] == count and n[COV] == cov, (pos, allele)
        rp = plane.get(chr(ref[pos]).upper())
        cells = []
        for s in (qual, mapq, dist):
            cells += [mean(s[rp], n[rp]) if rp else "0.0", mean(s[allele], n[allele])]
        v = verdict(int(n[allele]), int(qual[allele]), int(mapq[allele]), int(dist[allele]), min_qual, min_mapq, min_dist)
        rows.append("%s\t%s\t%s\n" % (line, "\t".join(cells), word(v)))
    return "".join(rows)


def as_dict(cols, sums):
    return {int(c): tuple(m[k] for m in sums) for k, c in enumerate(cols)}
