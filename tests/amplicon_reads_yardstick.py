"""The yardstick of --amplicon-reads (include/tcmi.h: tcmi_readset_amplicon_reads) in plain Python integers: for every record a loop
over ALL amplicons that counts the containments — no sorting, no table, nothing shared with csrc/amplicon_reads_rule.h.

A record is KEPT iff it is mapped (not FLAG 0x4), passes the read filter, its reference has a slot (shift >= 0), pos >= 0 and its
CIGAR's reference span (M, D, N, =, X) is > 0.  Its columns are p = pos + shift .. q = p + span - 1.  Amplicon i = (fs, le, rs, fe)
with slack s contains it iff fs - s <= p and q < fe + s.  Exactly one: reads[i] += 1, and full[i] += 1 iff p < le and q >= rs; two or
more: ambiguous += 1; none: unassigned += 1."""
import numpy as np

HEADER = "SAMPLE\tREGION\tAMPLICON\tPOOL\tREADS\tFULL_LENGTH\n"
REF_OPS = (0, 2, 3, 7, 8)           # M D N = X


def classify(p, q, amps4, slack):
    """-> (index of the one amplicon that contains [p, q], full-length?), (-2, False) for two or more, (-1, False) for none"""
    hits = [i for i, (fs, le, rs, fe) in enumerate(amps4) if fs - slack <= p and q < fe + slack]
    if not hits:
        return -1, False
    if len(hits) > 1:
        return -2, False
    fs, le, rs, fe = amps4[hits[0]]
    return hits[0], p < le and q >= rs


def span_of(cigar_words):
    return sum(int(w) >> 4 for w in cigar_words if (int(w) & 15) in REF_OPS)


def kept_columns(rd, shift=None, read_filter=None, mapq=None):
    """flat arrays (tcmi_reads layout) -> [(p, q)] of the kept records.  shift: per reference (None: reference 0 at 0, others have no
    slot); read_filter = (min_mapq, require, exclude) with mapq the records' MAPQ (None: 255 everywhere)."""
    out = []
    n = int(rd["n_reads"])
    tid = rd.get("tid")
    for i in range(n):
        flag, pos = int(rd["flag"][i]), int(rd["pos"][i])
        t = int(tid[i]) if tid is not None else 0
        if flag & 4 or pos < 0:
            continue
        if read_filter is not None:
            mq, req, exc = read_filter
            m = 255 if mapq is None else int(mapq[i])
            if m < mq or (flag & req) != req or (flag & exc):
                continue
        if shift is None:
            sh = 0 if t == 0 else -1
        else:
            sh = int(shift[t]) if 0 <= t < len(shift) else -1
        if sh < 0:
            continue
        span = span_of(rd["cigar"][int(rd["cigar_off"][i]):int(rd["cigar_off"][i + 1])])
        if span <= 0:
            continue
        out.append((pos + sh, pos + sh + span - 1))
    return out


def counts(columns, amps4, slack):
    """[(p, q)] of the kept records -> int64 [n + 2, 2]: {reads, full} per amplicon, then ambiguous, then unassigned"""
    n = len(amps4)
    out = np.zeros((n + 2, 2), np.int64)
    for p, q in columns:
        i, full = classify(p, q, amps4, slack)
        out[n if i == -2 else n + 1 if i == -1 else i, 0] += 1
        if full:
            out[i, 1] += 1
    return out


def text(sample, cnt, chroms, names, pools, header=True):
    """the table's text from the yardstick's counts (the writer's format, written out once more)"""
    n = len(names)
    rows = ["%s\t%s\t%s\t%s\t%d\t%d\n" % (sample, chroms[i], names[i], pools[i], cnt[i][0], cnt[i][1]) for i in range(n)]
    rows.append("%s\t*\t*ambiguous\t*\t%d\t0\n" % (sample, cnt[n][0]))
    rows.append("%s\t*\t*unassigned\t*\t%d\t0\n" % (sample, cnt[n + 1][0]))
    return (HEADER if header else "") + "".join(rows)
