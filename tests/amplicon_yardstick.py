"""The amplicon table's yardstick in plain Python integers: the record of an interval of the coverage plane, the table's text and the
scheme rule (primer names -> amplicons -> the reported interval).  Written from the contract in include/tcmi.h and the documented
rule of io/primers.py, sharing no code with either."""
import numpy as np

DTYPE = np.dtype([("sum", np.int64), ("n", np.int32), ("min", np.int32), ("min_pos", np.int32), ("median", np.int32), ("below", np.int32),
                  ("reserved", np.int32)])
HEADER = "SAMPLE\tREGION\tAMPLICON\tPOOL\tSTART\tEND\tLEN\tMEAN\tMEDIAN\tMIN\tMIN_POS\tBELOW\n"
EMPTY = (0, 0, 0, -1, 0, 0, 0)


def record(cov, start, end, min_depth):
    """cov: the coverage plane's L depths (anything int() takes); a position at or beyond L has depth 0.  The columns behind L are
    counted, not listed (an interval may end at 2^29): z zeros whose first position is max(start, L)."""
    n = end - start
    if n <= 0:
        return EMPTY
    L = len(cov)
    d = [int(x) for x in cov[min(start, L):min(end, L)]]
    z = n - len(d)
    lo = min(d + [0]) if z else min(d)
    lo_pos = start + d.index(lo) if lo in d else max(start, L)
    order = sorted(d)
    k, neg = (n - 1) // 2, sum(1 for x in d if x < 0)
    if k < neg:
        median = order[k]
    elif k < neg + z + d.count(0):      # the z zeros sort behind the negatives, among the zeros
        median = 0
    else:
        median = order[k - z]
    return (sum(d), n, lo, lo_pos, median, sum(1 for x in d if x < min_depth) + (z if 0 < min_depth else 0), 0)


def record_listed(cov, start, end, min_depth):
    """the same by listing every column (short intervals only): what `record` is pinned against"""
    n = end - start
    if n <= 0:
        return EMPTY
    d = [int(cov[p]) if p < len(cov) else 0 for p in range(start, end)]
    return (sum(d), n, min(d), start + d.index(min(d)), sorted(d)[(n - 1) // 2], sum(1 for x in d if x < min_depth), 0)


def records(cov, intervals, min_depth):
    return [record(cov, int(s), int(e), min_depth) for s, e in intervals]


def as_array(recs):
    return np.array([tuple(r) for r in recs], DTYPE) if len(recs) else np.zeros(0, DTYPE)


def text(recs, sample, region, names, pools, starts, pos_offset=0):
    out = []
    for (total, n, lo, lo_pos, med, below, _), name, pool, s in zip(recs, names, pools, starts):
        first = s - pos_offset + 1
        if n == 0:
            cols = [first, first - 1, 0, "NA", "NA", "NA", "NA", 0]
        else:
            cols = [first, first + n - 1, n, "%.2f" % (total / n), med, lo, lo_pos - pos_offset + 1, below]
        out.append("\t".join([sample, region, name, pool] + [str(c) for c in cols]) + "\n")
    return "".join(out)


# ---- the scheme rule: rows are (chrom, start, end, name, pool, strand) -------------------------------------------------------
def split_name(name):
    f = name.split("_")
    sides = [k for k, x in enumerate(f) if x.upper() in ("LEFT", "RIGHT")]
    if not sides:
        return None
    return "_".join(f[:sides[-1]]), f[sides[-1]].upper()


def scheme(rows, region="insert"):
    """-> [(chrom, key, pool, start, end)] ordered by (the chrom's order in the file, full start, key); rows must be well-formed"""
    chroms, amp = [], {}
    for chrom, s, e, name, pool, strand in rows:
        key, side = split_name(name)
        if chrom not in chroms:
            chroms.append(chrom)
        a = amp.setdefault(key, dict(chrom=chrom, pool=pool, L=[], R=[]))
        a["L" if side == "LEFT" else "R"].append((s, e))
    full = {k: (min(s for s, _ in a["L"]), max(e for _, e in a["R"])) for k, a in amp.items()}
    insert = {}
    for k, a in amp.items():
        s, e = max(e for _, e in a["L"]), min(s for s, _ in a["R"])
        insert[k] = (s, e if e >= s else s)
    out = []
    for k in sorted(amp, key=lambda k: (chroms.index(amp[k]["chrom"]), full[k][0], k)):
        if region == "full":
            iv = full[k]
        elif region == "insert":
            iv = insert[k]
        else:                                           # column by column: what no other amplicon's full covers, its longest run
            free = [p for p in range(*insert[k]) if not any(full[o][0] <= p < full[o][1] for o in amp if o != k and amp[o]["chrom"] == amp[k]["chrom"])]
            runs, run = [], []
            for p in free:
                if run and p != run[-1] + 1:
                    runs.append(run)
                    run = []
                run.append(p)
            if run:
                runs.append(run)
            best = max(runs, key=len) if runs else None     # (max keeps the first of equals)
            iv = (best[0], best[-1] + 1) if best else (insert[k][0], insert[k][0])
        out.append((amp[k]["chrom"], k, amp[k]["pool"], iv[0], iv[1]))
    return out
