"""The yardstick of --indel-table (tcmi_readset_indel_events, tcmi_indel_passes, tcmi_indel_hash, tcmi_indels_text): the rule of
include/tcmi.h restated in plain Python over read_specs records (dicts of pos, flag, cigar, seq, qual), written from the rule's words —
not from the kernel.  Which columns of a record are masked is tests/primer_yardstick.read_mask; the floor is "the quality at the
token's query index, 0 at or beyond len(SEQ), must be at least Q"; the rest is a walk over the CIGAR.  No tests in here."""
from fractions import Fraction

import numpy as np

from tests import primer_yardstick as py
from tests import read_specs as rs
from tests import synth_small as ss

INS, DEL = 1, 2
M, I, D, N, S, H, P, EQ, X = range(9)
REF_OPS, QUERY_OPS, MATCH_OPS = (M, D, N, EQ, X), (M, I, S, EQ, X), (M, EQ, X)
EVENT_DTYPE = np.dtype([("pos", np.int32), ("kind", np.int32), ("len", np.int32), ("count", np.int32), ("cov", np.int32),
                        ("reserved", np.int32), ("text_off", np.int64)])
TOTALS_DTYPE = np.dtype([("pos", np.int32), ("ins_total", np.int32), ("del_total", np.int32), ("reserved", np.int32)])
HEADER = "REGION\tPOS\tTYPE\tLEN\tSEQ\tCOUNT\tTOTAL_DP\tFREQ\n"
MASK64 = (1 << 64) - 1


def kept(r, flt=(0, 0, 0)):
    """does the record pile up under the read filter: mapped, through the filter, on a reference, with a reference span"""
    ops = ss.parse_cigar(r["cigar"])
    return not r["flag"] & 4 and rs.passes(r, flt) and r.get("tid", 0) >= 0 and r["pos"] >= 0 and sum(n for op, n in ops if op in REF_OPS) > 0


def inserted(ops, k, y):
    """the query indices of the insertion reported behind op k (y: the query index behind op k), [] when there is none.  An I op right
    behind op k: that op and every further I op with nothing but P ops between.  A P op behind op k, with another op behind it: every
    I op up to the next reference-consuming op; S ops on the way consume query, H and P ops do not."""
    if k + 1 >= len(ops):
        return []
    first = ops[k + 1][0]
    if first != I and not (first == P and k + 2 < len(ops)):
        return []
    out = []
    for op, n in ops[k + 1:]:
        if op == I:
            out += range(y, y + n)
            y += n
        elif first == I and op != P:
            break
        elif first == P and op in REF_OPS:
            break
        elif op == S:
            y += n
    return out


def record_events(r, table=(), q=0, slack=0, shift=0, clip=0):
    """the events of one kept record -> [(column, kind, len, bases)]: a DEL at the first column of every D op, an INS at the last column
    of every reference-consuming op with an insertion behind it — each iff the token on that column is counted at all: the column lies
    in [head_end, tail_start) and the quality at the token's query index (a matched base: its own; a D / N op: the index at which the
    op starts) is at least q.  clip: the record's first `clip` columns are its mate's, or all of them a duplicate's (--mate-overlap,
    --dedup): head_end = max(head_end, p + clip)"""
    ops = ss.parse_cigar(r["cigar"])
    seq = "" if r["seq"] == "*" else r["seq"].upper()
    qual = list(r["qual"]) if seq else []
    span = sum(n for op, n in ops if op in REF_OPS)
    p = r["pos"] + shift
    head_end, tail_start = py.read_mask(p, p + span - 1, table, slack)
    head_end = max(head_end, p + clip)

    def counted(c, qi):
        return head_end <= c < tail_start and (q == 0 or (qual[qi] if qi < len(seq) else 0) >= q)

    out = []
    x, y = p, 0
    for k, (op, n) in enumerate(ops):
        if op in REF_OPS and n > 0:
            if op == D and counted(x, y):
                out.append((x - shift, DEL, n, ""))
            last_q = y + n - 1 if op in MATCH_OPS else y
            if counted(x + n - 1, last_q):
                idx = inserted(ops, k, y + n if op in MATCH_OPS else y)
                if idx:
                    out.append((x + n - 1 - shift, INS, len(idx), "".join(seq[t] if t < len(seq) else "N" for t in idx)))
        if op in REF_OPS:
            x += n
        if op in QUERY_OPS:
            y += n
    return out


def events(records, table=(), q=0, slack=0, flt=(0, 0, 0), shift=0, clip=None):
    """-> ({(column, kind, len, bases): records}, {column: [ins_total, del_total]}) over the kept records; clip: one per record"""
    counts, totals = {}, {}
    assert clip is None or len(clip) == len(records)
    for i, r in enumerate(records):
        if not kept(r, flt):
            continue
        for ev in record_events(r, table, q, slack, shift, 0 if clip is None else int(clip[i])):
            counts[ev] = counts.get(ev, 0) + 1
            totals.setdefault(ev[0], [0, 0])[ev[1] - 1] += 1
    return counts, totals


def passes(count, cov, num, den, min_alt_depth, min_depth):
    return cov >= max(min_depth, 1) and count >= min_alt_depth and Fraction(count, cov) >= Fraction(num, den)


def reported(counts, cols, cov, num=0, den=1, min_alt_depth=1, min_depth=0):
    """the events on the queried columns that pass the rule, in THE order -> [(column, kind, len, bases, count, cov)]"""
    cov_of = dict(zip((int(c) for c in cols), (int(c) for c in cov)))
    out = [ev + (n, cov_of[ev[0]]) for ev, n in counts.items() if ev[0] in cov_of and passes(n, cov_of[ev[0]], num, den, min_alt_depth, min_depth)]
    return sorted(out, key=lambda t: t[:4])


def arrays(rep):
    """reported() -> (events as EVENT_DTYPE, text bytes): what tcmi_readset_indel_events returns"""
    ev = np.zeros(len(rep), EVENT_DTYPE)
    text = b""
    for i, (col, kind, ln, bases, n, cov) in enumerate(rep):
        ev[i] = (col, kind, ln, n, cov, 0, len(text) if kind == INS else -1)
        text += bases.encode()
    return ev, text


def totals_at(totals, cols):
    out = np.zeros(len(cols), TOTALS_DTYPE)
    for i, c in enumerate(cols):
        out[i] = (c, totals.get(int(c), [0, 0])[0], totals.get(int(c), [0, 0])[1], 0)
    return out


def unpack(ev, text):
    """the library's (events, text) -> [(column, kind, len, bases, count, cov)]"""
    text = bytes(text)
    return [(int(e["pos"]), int(e["kind"]), int(e["len"]), text[int(e["text_off"]):int(e["text_off"]) + int(e["len"])].decode() if e["kind"] == INS else "",
             int(e["count"]), int(e["cov"])) for e in ev]


def hash_(seed, nibbles, bits):
    """tcmi_indel_hash restated: FNV-1a's prime with a fold per nibble from a seeded start, the length mixed in at the end, two
    multiply-folds, the `bits` low bits"""
    h = 0xCBF29CE484222325 ^ ((seed * 0x9E3779B97F4A7C15) & MASK64)
    for nib in nibbles:
        h = ((h ^ (nib & 15)) * 0x100000001B3) & MASK64
        h ^= h >> 29
    h = ((h ^ len(nibbles)) * 0xD6E8FEB86659FD93) & MASK64
    h ^= h >> 32
    h = (h * 0xD6E8FEB86659FD93) & MASK64
    h ^= h >> 32
    return h & ((1 << bits) - 1)


def text(rep, region, ref, pos_offset=0):
    """reported() -> the rows of --indel-table: POS 1-based, SEQ the inserted bases or the deleted reference bases (upper case, N beyond
    the reference)"""
    rows = []
    for col, kind, ln, bases, n, cov in rep:
        if kind == DEL:
            bases = "".join(chr(ref[t]).upper() if t < len(ref) else "N" for t in range(col, col + ln))
        rows.append("%s\t%d\t%s\t%d\t%s\t%d\t%d\t%.6f\n" % (region, col - pos_offset + 1, "INS" if kind == INS else "DEL", ln, bases, n, cov, n / cov))
    return "".join(rows)
