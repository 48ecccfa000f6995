"""The yardstick of the mate-overlap rule (--mate-overlap; tcmi_ctx_set_mate_overlap), from committed oracle functions only: the kept
records grouped by key in a Python dict, the rule applied literally — eligible, key, pair, loser, clip —, then primer_yardstick's counts
with head_end = max(head_end, p + clip).  A record is kept when it piles up (tc_oracle.read_piles_up), lies on reference 0 and passes
the read filter f = (min_mapq, require_flags, exclude_flags).  No tests in here."""
import numpy as np

from oracle import c_oracle
from oracle import tc_oracle as orc
from tests import primer_yardstick as py

NONE = (0, 0, 0)
COUNTERS = ("pairs", "clipped_reads", "clipped_columns", "ambiguous")
# why a kept record got no mate: the classes the fuzz must hold
CLASSES = ("not_paired", "not_proper", "mate_unmapped", "secondary", "supplementary", "both_or_neither_end", "other_reference", "no_next_pos",
           "single", "ambiguous", "next_pos_mismatch", "same_end")


def kept(rd, i, f=NONE):
    mapq = int(rd["mapq"][i]) if rd.get("mapq") is not None else 60
    flag = int(rd["flag"][i])
    return (orc.read_piles_up(rd, i) and int(rd["pos"][i]) >= 0 and int(rd["tid"][i]) == 0 and mapq >= f[0] and (flag & f[1]) == f[1] and
            (flag & f[2]) == 0)


def span(rd, i):
    """-> (first column, last column) of record i"""
    p = int(rd["pos"][i])
    return p, p + orc.ref_length(orc.read_cigar(rd, i)) - 1


def fields(rd, i):
    return int(rd["flag"][i]), int(rd["tid"][i]), int(rd["pos"][i]), int(rd["next_tid"][i]), int(rd["next_pos"][i])


def name(rd, i):
    return bytes(bytearray(rd["names"][int(rd["name_off"][i]):int(rd["name_off"][i + 1])]))


def why_not_eligible(flag, tid, pos, ntid, npos):
    """None: eligible"""
    if not flag & 0x1:
        return "not_paired"
    if not flag & 0x2:
        return "not_proper"
    if flag & 0x8:
        return "mate_unmapped"
    if flag & 0x100:
        return "secondary"
    if flag & 0x800:
        return "supplementary"
    if bool(flag & 0x40) == bool(flag & 0x80):
        return "both_or_neither_end"
    if ntid != tid:
        return "other_reference"
    if npos < 0:
        return "no_next_pos"
    return None


def join(rd, f=NONE):
    """-> (clip per record, {counter: n}, {record: class} of the kept records that are no member of a pair, [(loser, winner)])"""
    n = int(rd["n_reads"])
    clip = [0] * n
    groups, classes, pairs = {}, {}, []
    for i in range(n):
        if not kept(rd, i, f):
            continue
        flag, tid, pos, ntid, npos = fields(rd, i)
        why = why_not_eligible(flag, tid, pos, ntid, npos)
        if why:
            classes[i] = why
            continue
        groups.setdefault((name(rd, i), tid, min(pos, npos), max(pos, npos)), []).append(i)
    cnt = dict.fromkeys(COUNTERS, 0)
    for members in groups.values():
        if len(members) == 1:
            classes[members[0]] = "single"
            continue
        if len(members) >= 3:
            cnt["ambiguous"] += len(members)
            for i in members:
                classes[i] = "ambiguous"
            continue
        a, b = members
        fa, fb = fields(rd, a), fields(rd, b)
        if not (fa[4] == fb[2] and fb[4] == fa[2]):
            classes[a] = classes[b] = "next_pos_mismatch"
            continue
        if bool(fa[0] & 0x40) == bool(fb[0] & 0x40):
            classes[a] = classes[b] = "same_end"
            continue
        a_loses = fa[2] > fb[2] or (fa[2] == fb[2] and bool(fa[0] & 0x80))
        lo, wi = (a, b) if a_loses else (b, a)
        (pl, ql), (_, qw) = span(rd, lo), span(rd, wi)
        clip[lo] = max(0, min(qw, ql) - pl + 1)
        pairs.append((lo, wi))
        cnt["pairs"] += 1
        cnt["clipped_reads"] += clip[lo] > 0
        cnt["clipped_columns"] += clip[lo]
    return clip, cnt, classes, pairs


def tokens(rd, i, clip_i, primers=(), q=0, slack=0):
    """the tokens record i keeps: [(column, token, quality)], and whether the primer table masks it"""
    toks = list(orc.read_tokens(rd, i, with_qual=True))
    p, last = toks[0][0], toks[-1][0]
    head_end, tail_start = py.read_mask(p, last, primers, slack)
    masked = head_end > p or tail_start <= last
    head_end = max(head_end, p + clip_i)
    return [(c, t, ql) for c, t, ql in toks if head_end <= c < tail_start and ql >= q], masked


def counts(rd, L, primers=(), q=0, slack=0, f=NONE, mate=True):
    """-> {"counts": int32 [extent, 7], "n_masked", "n_piled", "max_end", "clip", "counters", "classes", "pairs", "kept_tokens"}"""
    n = int(rd["n_reads"])
    clip, cnt, classes, pairs = join(rd, f) if mate else ([0] * n, dict.fromkeys(COUNTERS, 0), {}, [])
    cols = {}
    n_masked = n_piled = max_end = n_tok = 0
    for i in range(n):
        if not kept(rd, i, f):
            continue
        n_piled += 1
        max_end = max(max_end, span(rd, i)[1] + 1)
        toks, masked = tokens(rd, i, clip[i], primers, q, slack)
        n_masked += masked
        n_tok += len(toks)
        for c, t, _ in toks:
            cols.setdefault(c, []).append(t)
    out = np.zeros((max(c_oracle.extent(rd, L), max_end, L), 7), np.int32)
    for c, t in cols.items():
        out[c] = orc.tally_tokens(t)
    return {"counts": out, "n_masked": n_masked, "n_piled": n_piled, "max_end": max_end, "clip": clip, "counters": cnt, "classes": classes,
            "pairs": pairs, "kept_tokens": n_tok}
