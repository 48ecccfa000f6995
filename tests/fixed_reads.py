"""Reads of one fixed length with one M op each, by the million (bamwriter.write_bam_fast), and what the step and the three counting
calls must give for them, restated in numpy (the read filter, the base-quality floor and the primer mask included): the positions are sorted, so the reads over
a column are one slice of the arrays.  The
restatement is pinned to the committed yardsticks (strand_yardstick, links_yardstick, amplicon_reads_yardstick) on 2 000 records in
tests/test_repeat_bam.py; tests/test_stream_scale.py then uses it at record counts those yardsticks cannot afford.  No GPU, no tests
in here."""
import numpy as np

from trueconsense_amd.io import bamwriter

LEN = 20                                                                        # every read is 20M
L = 2400
NIBBLES = np.array([1, 8, 2, 4, 15], np.uint8)                                  # A T C G N as BAM writes them ...
PLANE = np.zeros(16, np.uint8)                                                  # ... -> the class of links_yardstick: 1..4 A T C G, 6 coverage only
PLANE[:] = 6
PLANE[[1, 8, 2, 4]] = (1, 2, 3, 4)
QUALS = np.array([2, 12, 13, 14, 30, 40], np.uint8)                             # around the floor of 13
MAPQS = np.array([0, 19, 20, 60], np.uint8)
MQ = (20, 0, 0)                                                                 # the MAPQ filter the tests use
# seven amplicons of 400 columns every 300 (test_amplicon_reads.tiled(7): neighbours overlap by 100 — ambiguous reads; nothing below
# column 30 or beyond 2 230 — unassigned ones) and one of 24 columns behind them that a read of 20 spans from primer zone to primer zone
SCHEME = [(30 + 300 * k, 54 + 300 * k, 406 + 300 * k, 430 + 300 * k) for k in range(7)] + [(2300, 2310, 2315, 2324)]


def generate(n, seed=1):
    """-> dict(pos int32 [n] sorted, flag uint16 [n] (0 or 16), base uint8 [n, LEN] (nibbles, an N now and then), qual uint8 [n, LEN],
    mapq uint8 [n]): n reads spread over L columns, the strands and the qualities at random"""
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.integers(0, L - LEN + 1, n)).astype(np.int32)
    flag = (rng.integers(0, 3, n) == 0).astype(np.uint16) * 16
    base = NIBBLES[rng.choice(5, (n, LEN), p=(0.24, 0.24, 0.24, 0.24, 0.04))]
    qual = QUALS[rng.integers(0, len(QUALS), (n, LEN))]
    mapq = MAPQS[rng.integers(0, len(MAPQS), n)]
    return dict(pos=pos, flag=flag, base=base, qual=qual, mapq=mapq)


def head(rd, n):
    return {k: v[:n] for k, v in rd.items()}


def write(path, rd):
    packed = (rd["base"][:, 0::2] << 4) | rd["base"][:, 1::2]
    bamwriter.write_bam_fast(str(path), rd["pos"], rd["flag"], packed, LEN, ref_len=L, qual=rd["qual"], mapq=rd["mapq"])
    return str(path)


def kept(rd, f=(0, 0, 0)):
    """bool [n]: the records that pass the read filter (none of them is unmapped)"""
    flag = rd["flag"].astype(np.int64)
    return (rd["mapq"] >= f[0]) & ((flag & f[1]) == f[1]) & ((flag & f[2]) == 0)


def read_mask(rd, table=(), slack=0):
    """primer_yardstick.read_mask for every read at once -> (head_end, tail_start) int64 [n]"""
    p = rd["pos"].astype(np.int64)
    q = p + LEN - 1
    head_end, tail_start = p.copy(), q + 1
    for s, e, rev in table:
        if rev:
            hit = (s <= q) & (q < e + slack)
            tail_start[hit] = np.minimum(tail_start[hit], s)
        else:
            hit = (s - slack <= p) & (p < e)
            head_end[hit] = np.maximum(head_end[hit], e)
    return head_end, tail_start


def masked_reads(rd, f=(0, 0, 0), table=(), slack=0):
    """the kept reads with a non-empty head or tail mask"""
    head_end, tail_start = read_mask(rd, table, slack)
    p = rd["pos"].astype(np.int64)
    return int((kept(rd, f) & ((head_end > p) | (tail_start <= p + LEN - 1))).sum())


def column(rd, keep, mask, c, q):
    """-> (lo, hi, cls): the records lo..hi-1 are those that start in (c - LEN, c]; cls uint8 [hi - lo] is the class of each one's token
    at column c — 0: none (filtered, below the floor or masked), 1..4: A T C G, 6: coverage only"""
    lo, hi = int(np.searchsorted(rd["pos"], c - LEN + 1, "left")), int(np.searchsorted(rd["pos"], c, "right"))
    i = np.arange(lo, hi)
    off = c - rd["pos"][lo:hi]
    cls = PLANE[rd["base"][i, off]]
    cls[~keep[lo:hi] | (rd["qual"][i, off] < q) | (c < mask[0][lo:hi]) | (c >= mask[1][lo:hi])] = 0
    return lo, hi, cls


def strand(rd, cols, q=0, f=(0, 0, 0), table=(), slack=0):
    """-> (fwd, rev) int32 [len(cols), 7] (coverage, A, T, C, G, X, I): per offset into the reads one bincount over (strand, column,
    class) of the tokens that are kept, at or above the floor and outside the read's primer mask"""
    keep, minus, p = kept(rd, f), (rd["flag"] & 16 != 0).astype(np.int64), rd["pos"].astype(np.int64)
    head_end, tail_start = read_mask(rd, table, slack)
    n = np.zeros(2 * L * 8, np.int64)
    for o in range(LEN):
        ok = keep & (rd["qual"][:, o] >= q) & (head_end <= p + o) & (p + o < tail_start)
        n += np.bincount((((minus * L + p + o) << 3) + PLANE[rd["base"][:, o]])[ok], minlength=len(n))
    n = n.reshape(2, L, 8)
    out = np.zeros((2, len(cols), 7), np.int32)
    inside = [k for k, c in enumerate(cols) if 0 <= c < L]
    at = [cols[k] for k in inside]
    out[:, inside, 0] = n[:, at, 1:].sum(2)
    out[:, inside, 1:5] = n[:, at, 1:5]
    return out[0], out[1]


def matrix(rd, n_pos, q=0, f=(0, 0, 0), table=(), slack=0):
    fwd, rev = strand(rd, range(n_pos), q, f, table, slack)
    return fwd + rev


def links(rd, cols, k, q=0, f=(0, 0, 0), table=(), slack=0):
    """-> int32 [len(cols) * k, 7, 7] in the order of links_yardstick.joint"""
    keep, mask = kept(rd, f), read_mask(rd, table, slack)
    at = [column(rd, keep, mask, c, q) for c in cols]
    n = len(cols)
    out = np.zeros((n * k, 49), np.int64)
    for i in range(n):
        for d in range(1, k + 1):
            if i + d >= n:
                continue
            (alo, ahi, a), (blo, bhi, b) = at[i], at[i + d]
            j = out[i * k + d - 1]
            if blo >= ahi:                                                      # no record reaches both columns
                j[0::7] += np.bincount(a, minlength=7)
                j[:7] += np.bincount(b, minlength=7)
            else:                                                               # (sorted: alo <= blo and ahi <= bhi)
                x, y = (np.zeros(bhi - alo, np.int64) for _ in range(2))
                x[:ahi - alo], y[blo - alo:] = a, b
                j += np.bincount(x * 7 + y, minlength=49)
            j[0] = 0
    return out.reshape(n * k, 7, 7).astype(np.int32)


def amplicon_reads(rd, amps4, slack, f=(0, 0, 0)):
    """-> int64 [n + 2, 2] in the order of amplicon_reads_yardstick.counts; per amplicon the records it contains are one slice"""
    keep = kept(rd, f)
    n, m = len(rd["pos"]), len(amps4)
    p = rd["pos"].astype(np.int64)
    hits, which = (np.zeros(n + 1, np.int64) for _ in range(2))
    for i, (fs, le, rs, fe) in enumerate(amps4):                               # fs - slack <= p and p + LEN - 1 < fe + slack
        lo, hi = np.searchsorted(p, fs - slack, "left"), np.searchsorted(p, fe + slack - LEN, "right")
        if hi > lo:
            hits[lo] += 1
            hits[hi] -= 1
            which[lo] += i
            which[hi] -= i
    hits, which = np.cumsum(hits)[:n], np.cumsum(which)[:n]
    out = np.zeros((m + 2, 2), np.int64)
    one = keep & (hits == 1)
    out[:m, 0] = np.bincount(which[one], minlength=m)
    le, rs = (np.array([a[k] for a in amps4], np.int64) for k in (1, 2))
    full = one & (p < le[which * (hits == 1)]) & (p + LEN - 1 >= rs[which * (hits == 1)])
    out[:m, 1] = np.bincount(which[full], minlength=m)
    out[m, 0], out[m + 1, 0] = (keep & (hits > 1)).sum(), (keep & (hits == 0)).sum()
    return out
