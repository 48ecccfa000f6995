"""The yardstick of the duplicate rule (--dedup; tcmi_ctx_set_dedup), from committed oracle functions only: the rule of include/tcmi.h
applied literally in Python dicts — examined, end, score, template, key, winner — on top of mate_overlap_yardstick.join's pairs, then
that module's tokens() with clip = max(the mate rule's clip, the span of a duplicate).  A record is kept as mate_overlap_yardstick.kept
says (reference 0 only: a file of several references is judged reference by reference, mate_overlap_cases.on_reference_0 — the key
holds the reference, and the tie-break's order is the file's within each).  No tests in here."""
import numpy as np

from oracle import c_oracle
from oracle import tc_oracle as orc
from tests import mate_overlap_yardstick as my

NONE = my.NONE
COUNTERS = ("templates", "duplicate_templates", "duplicate_records", "duplicate_sets")
MIN_QUAL = 15
SCORE_MOST = 2 ** 32 - 1


def examined(rd, i, f=NONE):
    return my.kept(rd, i, f) and not int(rd["flag"][i]) & 0x900


def end(rd, i):
    """-> (refID, u5, rev): the unclipped 5' coordinate on the record's own reference"""
    cig = orc.read_cigar(rd, i)                                 # [(op, len)]
    ops = [(int(op), int(n)) for op, n in cig]
    lead = trail = 0
    k = 0
    while k < len(ops) and ops[k][0] in (4, 5):
        lead += ops[k][1]
        k += 1
    k = len(ops)
    while k > 0 and ops[k - 1][0] in (4, 5):
        trail += ops[k - 1][1]
        k -= 1
    rev = int(bool(int(rd["flag"][i]) & 0x10))
    pos = int(rd["pos"][i])
    p, q = my.span(rd, i)
    return int(rd["tid"][i]), (pos + (q - p + 1) - 1 + trail) if rev else pos - lead, rev


def quals(rd, i):
    return [int(x) for x in rd["qual"][int(rd["qual_off"][i]):int(rd["qual_off"][i + 1])]]


def score(rd, i):
    """the sum of the QUAL bytes >= 15; a byte of 0xFF is a missing quality"""
    return min(sum(x for x in quals(rd, i) if MIN_QUAL <= x != 255), SCORE_MOST)


def key_bytes(key):
    """the twelve bytes csrc/dedup_rule.h hashes: refID << 3 | pair << 2 | rev_a << 1 | rev_b, u5_a, u5_b, little-endian"""
    kind, tid, a, b = key
    w0 = (tid << 3) | (4 if kind == "P" else 0) | (a[1] << 1) | (b[1] if kind == "P" else 0)
    return b"".join(int(v & 0xFFFFFFFF).to_bytes(4, "little") for v in (w0, a[0], b[0] if kind == "P" else 0))


def templates(rd, f=NONE):
    """-> ({key: [(score, leader, records)]}, {record: its mate} of the join's pairs): key = ("F" | "P", refID, (u5, rev), (u5, rev) | None)"""
    _, _, _, pairs = my.join(rd, f)
    mate = {}
    for lo, wi in pairs:
        mate[lo], mate[wi] = wi, lo
    out = {}
    for i in range(int(rd["n_reads"])):
        if not examined(rd, i, f):
            continue
        tid, u5, rev = end(rd, i)
        if i in mate:
            j = mate[i]
            if j < i:
                continue                                        # (its leader stands for the pair)
            ends = sorted([(u5, rev), end(rd, j)[1:]])
            key, recs, sc = ("P", tid, ends[0], ends[1]), (i, j), min(score(rd, i) + score(rd, j), SCORE_MOST)
        else:
            key, recs, sc = ("F", tid, (u5, rev), None), (i,), score(rd, i)
        out.setdefault(key, []).append((sc, i, recs))
    return out, mate


def verdicts(rd, f=NONE):
    """-> {"dup": bool [n], "counters", "templates": templates()' dict, "mate", "winner": {key: leader}}"""
    tpl, mate = templates(rd, f)
    dup = np.zeros(int(rd["n_reads"]), bool)
    cnt = dict.fromkeys(COUNTERS, 0)
    winner = {}
    for key, ts in tpl.items():
        best = max(ts, key=lambda t: (t[0], -t[1]))             # the highest score; at equal score the lowest leader
        winner[key] = best[1]
        cnt["templates"] += len(ts)
        cnt["duplicate_sets"] += len(ts) >= 2
        for t in ts:
            if t is not best:
                cnt["duplicate_templates"] += 1
                cnt["duplicate_records"] += len(t[2])
                for i in t[2]:
                    dup[i] = True
    return {"dup": dup, "counters": cnt, "templates": tpl, "mate": mate, "winner": winner}


def counts(rd, L, primers=(), q=0, slack=0, f=NONE, mate=False, dedup=True):
    """mate_overlap_yardstick.counts with the duplicate rule on top -> its dict, and "dup", "dedup_counters", "verdicts"; "counters" are
    the join's (zeros with the mate rule off)"""
    n = int(rd["n_reads"])
    clip, cnt, classes, pairs = my.join(rd, f) if mate else ([0] * n, dict.fromkeys(my.COUNTERS, 0), {}, [])
    v = verdicts(rd, f) if dedup else {"dup": np.zeros(n, bool), "counters": dict.fromkeys(COUNTERS, 0), "templates": {}, "mate": {}, "winner": {}}
    clip = list(clip)
    for i in np.flatnonzero(v["dup"]):
        p, last = my.span(rd, int(i))
        clip[i] = max(clip[i], last - p + 1)                    # clipped from end to end: piled up, adds nothing
    cols = {}
    n_masked = n_piled = max_end = 0
    for i in range(n):
        if not my.kept(rd, i, f):
            continue
        n_piled += 1
        max_end = max(max_end, my.span(rd, i)[1] + 1)
        toks, masked = my.tokens(rd, i, clip[i], primers, q, slack)
        n_masked += masked
        for c, t, _ in toks:
            cols.setdefault(c, []).append(t)
    out = np.zeros((max(c_oracle.extent(rd, L), max_end, L), 7), np.int32)
    for c, t in cols.items():
        out[c] = orc.tally_tokens(t)
    return {"counts": out, "n_masked": n_masked, "n_piled": n_piled, "max_end": max_end, "clip": clip, "counters": cnt, "classes": classes,
            "pairs": pairs, "dup": v["dup"], "dedup_counters": v["counters"], "verdicts": v}


# ---- what a set of records holds: the classes of tests/dedup_cases.py's list ---------------------------------------------------------------
def classes(rd, f=NONE):
    """-> the names of dedup_cases.CLASSES that the records show under filter f"""
    v = verdicts(rd, f)
    tpl = v["templates"]
    _, _, mate_classes, _ = my.join(rd, f)
    mclip = my.join(rd, f)[0]
    n = int(rd["n_reads"])
    seen = set()
    frag_ends, pair_ends = {}, {}
    for key, ts in tpl.items():
        if key[0] == "F":
            frag_ends.setdefault((key[1],) + key[2], []).append(key)
        else:
            for e in (key[2], key[3]):
                pair_ends.setdefault((key[1],) + e, set()).add(key)
        if len(ts) < 2:
            continue
        scores = sorted((t[0] for t in ts), reverse=True)
        recs = [i for t in ts for i in t[2]]
        if key[0] == "F" and len(ts) >= 3 and len(set(scores)) == len(scores):
            seen.add("fragment_set_of_three")
        if key[0] == "P":
            seen.add("pair_set")
        if scores[0] == scores[1]:
            seen.add("tie")
            assert v["winner"][key] == min(t[1] for t in ts if t[0] == scores[0])
        if key[0] == "F" and key[2][1] == 0 and len({int(rd["pos"][i]) for i in recs}) > 1:
            seen.add("same_u5_different_clips")
        if key[0] == "F" and any(op == 5 for i in recs for op, _ in orc.read_cigar(rd, i)):
            seen.add("hard_clip_in_set")
        if key[0] == "F" and key[2][1] == 1 and len({int(rd["pos"][i]) for i in recs}) > 1:
            seen.add("reverse_pos_differ")
        if any(quals(rd, i) and all(x == 255 for x in quals(rd, i)) for i in recs):
            seen.add("qual_ff")
        if any(14 in quals(rd, i) for i in recs) and any(15 in quals(rd, i) for i in recs):
            seen.add("threshold")
        if any(mate_classes.get(i) == "ambiguous" for i in recs):
            seen.add("ambiguous_fragments")
        if key[0] == "P" and any(v["dup"][i] and mclip[i] > 0 for i in recs):
            seen.add("dup_pair_overlaps")
        if any(e[0] < 0 for e in key[2:] if e):
            seen.add("negative_u5")
    # forward and reverse at the same pos: two fragment keys, neither record loses to the other
    at = {}
    for key in tpl:
        if key[0] == "F":
            for _, i, _ in tpl[key]:
                at.setdefault((key[1], int(rd["pos"][i])), set()).add(key[2][1])
    if any(len(s) == 2 for s in at.values()):
        seen.add("fwd_rev_same_pos")
    # two pairs that share one end and differ in the other
    if any(len(keys) >= 2 for keys in pair_ends.values()):
        seen.add("pair_one_end_differs")
    if any(e in frag_ends for e in pair_ends):
        seen.add("pair_and_fragment_same_end")
    full = {(key[1],) + key[2]: key for key, ts in tpl.items() if key[0] == "F" and len(ts) >= 2}
    for i in range(n):
        flag = int(rd["flag"][i])
        if my.kept(rd, i, f) and flag & 0x900 and end(rd, i) in full:
            seen.add("secondary_at_duplicate")
            assert not v["dup"][i]
        # a record that fails the filter at a fragment's place with a score above every template there: it is no candidate
        if f != NONE and not my.kept(rd, i, f) and my.kept(rd, i, NONE) and not flag & 0x900 and end(rd, i) in frag_ends:
            if score(rd, i) > max(t[0] for key in frag_ends[end(rd, i)] for t in tpl[key]):
                seen.add("filtered_best")
    return seen
