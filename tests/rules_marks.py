"""What the record-stream tables must give under the mate-overlap rule and the duplicate rule, from committed yardsticks only: per
record and column the class and the I mark of the token the record keeps (mate_overlap_yardstick.tokens under the clip of
mate_overlap_yardstick.counts / dedup_yardstick.counts, each column's tokens through tc_oracle.tally_tokens — links_yardstick.classes
taken under a clip, no second statement of the token rule), the indel events of the spec lists under that clip, where a record's clip
edge meets a D op or an insertion, and the per-strand and evidence tallies of the kept tokens (`walked`, which tests/test_mate_overlap.py
and tests/test_dedup.py share).  No tests in here."""
import numpy as np

from oracle import tc_oracle as orc
from tests import dedup_cases as dc
from tests import evidence_yardstick as ey
from tests import indel_yardstick as iy
from tests import links_yardstick as ly
from tests import mate_overlap_cases as mc
from tests import mate_overlap_yardstick as my
from tests import synth_small as ss

NONE = my.NONE
RULES = {"mate": (True, False), "dedup": (False, True), "both": (True, True)}       # rule -> (--mate-overlap, --dedup)
# the files both rules' tables are checked on: file -> (specs in file order, the BAM header's references, reference length, the rules
# it runs under): the hand-made cases and the fuzz seeds of tests/mate_overlap_cases.py and tests/dedup_cases.py
FILES = {"mate_cases": (lambda: mc.cases()[0], mc.REFS, mc.L, ("mate", "both")), "dedup_cases": (dc.cases, dc.REFS, dc.L, ("mate", "dedup", "both"))}
FILES.update({"mate_seed%d" % s: (lambda s=s: mc.fuzz_specs(s), mc.FUZZ_REFS, mc.FUZZ_L, ("mate", "both")) for s in mc.FUZZ_SEEDS})
FILES.update({"dedup_seed%d" % s: (lambda s=s: dc.fuzz_specs(s), dc.FUZZ_REFS, dc.FUZZ_L, ("mate", "dedup", "both")) for s in dc.FUZZ_SEEDS})


def marks(rd, y, primers=(), q=0, slack=0, f=NONE):
    """y: the dict of mate_overlap_yardstick.counts / dedup_yardstick.counts for the flat arrays rd under the same table, floor and
    filter -> (cls, ins) uint8 [records, len(y["counts"])]: the class of the record's token at the column (0 none, 1..4 counted on
    plane A, T, C, G, 5 on X, 6 on coverage and none of those) and its I mark; the rows of records that are not kept stay 0"""
    n, n_pos = int(rd["n_reads"]), len(y["counts"])
    cls, ins = np.zeros((n, n_pos), np.uint8), np.zeros((n, n_pos), np.uint8)
    for i in range(n):
        if not my.kept(rd, i, f):
            continue
        per_col = {}
        for c, t, _ in my.tokens(rd, i, y["clip"][i], primers, q, slack)[0]:
            per_col.setdefault(c, []).append(t)
        for c, t in per_col.items():
            m = orc.tally_tokens(t)
            assert max(m) <= 1 and sum(m[1:6]) <= m[0] == 1, "one record adds at most one token a column, to coverage and at most one plane of A..X"
            cls[i, c] = 1 + int(np.argmax(m[1:6])) if any(m[1:6]) else 6
            ins[i, c] = m[6]
    cols = list(range(n_pos))
    got = np.stack([(cls == k).sum(0) for k in range(7)], 1)
    assert np.array_equal(got[:, 1:], ly.classes_of_matrix(y["counts"], cols)[:, 1:]), "the classes do not add up to the yardstick's matrix"
    assert np.array_equal(ins.sum(0), y["counts"][:, 6]), "the I marks do not add up to the yardstick's I plane"
    return cls, ins


def events(specs, rd, y, primers=(), q=0, slack=0, f=NONE):
    """indel_yardstick.events of the spec list (in rd's order) under y's clips -> ({event: records}, {column: [ins_total, del_total]});
    which records are kept is mate_overlap_yardstick.kept's verdict on rd, and indel_yardstick.kept must agree on the specs"""
    assert len(specs) == int(rd["n_reads"]), (len(specs), int(rd["n_reads"]))
    keep = [my.kept(rd, i, f) for i in range(len(specs))]
    assert keep == [iy.kept(r, f) for r in specs], "the two yardsticks keep other records"
    return iy.events(specs, primers, q, slack, f, clip=y["clip"])


def clip_edges(specs, clip):
    """where the clip edges of the records with 0 < clip < span fall -> {"del_cut": D ops whose first column is clipped and whose last is
    not, "del_at_edge": D ops that start on the edge, "ins_lost": insertions anchored on column edge - 1, "ins_kept": ... on column
    edge}, counted with indel_yardstick.record_events of the unclipped record"""
    out = dict.fromkeys(("del_cut", "del_at_edge", "ins_lost", "ins_kept"), 0)
    for r, c in zip(specs, clip):
        span = sum(n for op, n in ss.parse_cigar(r["cigar"]) if op in iy.REF_OPS)
        if not iy.kept(r) or not 0 < c < span:
            continue
        edge = r["pos"] + c
        for col, kind, ln, _ in iy.record_events(r):
            if kind == iy.DEL:
                out["del_cut"] += col < edge < col + ln
                out["del_at_edge"] += col == edge
            else:
                out["ins_lost"] += col == edge - 1
                out["ins_kept"] += col == edge
    return out


def first_live_columns(rd, y, f=NONE):
    """the first live column, pos + clip, of every kept record with a clip, ascending (a duplicate's: the column behind its last)"""
    return sorted({int(rd["pos"][i]) + int(c) for i, c in enumerate(y["clip"]) if c > 0 and my.kept(rd, i, f)})


def walked(rd, y, primers=(), q=0, f=NONE):
    """the existing yardsticks' tallies fed the tokens y keeps -> (fwd, rev int32 [n_pos, 7], {"n", "qual", "mapq", "dist": int64
    [n_pos, 7]}): tc_oracle.tally_tokens per strand, evidence_yardstick.tokens' sums, on the columns the record keeps"""
    n_pos = len(y["counts"])
    fwd, rev = np.zeros((n_pos, 7), np.int32), np.zeros((n_pos, 7), np.int32)
    ev = {k: np.zeros((n_pos, 7), np.int64) for k in ("qual", "mapq", "dist", "n")}
    for i in range(int(rd["n_reads"])):
        if not my.kept(rd, i, f):
            continue
        toks, _ = my.tokens(rd, i, y["clip"][i], primers, q)
        side = rev if int(rd["flag"][i]) & 0x10 else fwd
        per_col = {}
        for c, t, _ in toks:
            per_col.setdefault(c, []).append(t)
        for c, t in per_col.items():
            side[c] += np.array(orc.tally_tokens(t), np.int32)
        keep = {c for c, _, _ in toks}
        for c, planes, ql, mq, dist in ey.tokens(rd, i):
            if c in keep:
                for pl in planes:
                    ev["qual"][c, pl] += ql
                    ev["mapq"][c, pl] += mq
                    ev["dist"][c, pl] += dist
                    ev["n"][c, pl] += 1
    assert np.array_equal(fwd + rev, y["counts"]) and np.array_equal(ev["n"], y["counts"])      # (the yardsticks add up to the matrix)
    return fwd, rev, ev
