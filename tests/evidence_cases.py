"""What the tests of --variant-evidence share (tests/test_evidence_rule.py without a GPU, tests/test_evidence_counts.py with one): the
device call between guards, the yardstick's sums of a fuzz seed (cached), the queried columns, the hand-made records of the distance
rule, the numpy restatement for tests/fixed_reads.py's records, what a workgroup's LDS counters reach on a repeated file, and the
conditions that keep a case from being vacuous.  No tests in here; importing this opens no device."""
import ctypes as C
import functools
import re

import numpy as np

from tests import device_file as dvf
from tests import evidence_yardstick as ey
from tests import fixed_reads as fx
from tests import fuzz_masked as fm
from tests import read_specs as rsp
from tests import strand_cases as stc
from trueconsense_amd import _ffi, engine
from trueconsense_amd import synthetic as syn

L = fm.L
LDS = engine.EVIDENCE_LDS
G = 64                                                                          # guard words on either side of the records
WORDS = 50                                                                      # int32 words of one tcmi_evidence_counts
NAMES = ("n", "qual", "mapq", "dist")
REF_PLANE = {"A": 1, "T": 2, "C": 3, "G": 4}


def device_counts(ctx, rs, cols):
    """tcmi_readset_evidence_counts into a host buffer between guards -> (n, qual, mapq, dist) int64 [n, 7]; pos is checked here, and
    Context.evidence_counts must give the same numbers (run after run)"""
    cols = np.ascontiguousarray(cols, np.int64)
    n = len(cols)
    buf = dvf.sentinel(2 * G + WORDS * n, np.int32, salt=11).copy()
    before = buf.copy()
    rc = _ffi.lib().tcmi_readset_evidence_counts(ctx.handle, rs.handle, n, _ffi.ptr(cols), C.c_void_p(buf.ctypes.data + 4 * G))
    _ffi.check(rc, ctx.handle)
    assert np.array_equal(buf[:G], before[:G]) and np.array_equal(buf[-G:], before[-G:]), "a guard around the records was written"
    got = buf[G:-G].view(engine.EVIDENCE_DTYPE).copy()
    assert np.array_equal(got["pos"], cols), (got["pos"][:8].tolist(), cols[:8].tolist())
    again = ctx.evidence_counts(rs, cols)
    assert all(np.array_equal(got[k], again[k]) for k in NAMES + ("pos",)), "Context.evidence_counts gave other numbers than the call before it"
    return tuple(got[k].astype(np.int64) for k in NAMES)


def differ(got, want, cols, label):
    """'' when (n, qual, mapq, dist) equal the yardstick's; else the first differing columns with both rows"""
    if all(np.array_equal(g, w) for g, w in zip(got, want)):
        return ""
    rows = []
    for name, g, w in zip(NAMES, got, want):
        if g.shape != w.shape:
            rows.append("%s: shape %r, the yardstick's %r" % (name, g.shape, w.shape))
            continue
        for k in np.unique(np.argwhere(g != w)[:, 0])[:6].tolist():
            rows.append("%s column %d: got %r want %r" % (name, cols[k], g[k].tolist(), w[k].tolist()))
    return "%r (coverage, A, T, C, G, X, I)\n%s" % (label, "\n".join(rows))


def times(sums, r):
    return tuple(r * m for m in sums)


def take(sums, idx):
    return tuple(m[idx] for m in sums)


@functools.lru_cache(maxsize=None)
def reference():
    return syn.make_reference(seed=3, L=L, cds=[])[0]


@functools.lru_cache(maxsize=None)
def fuzz_arrays(seed, window=None):
    """the arrays of every record of the seed's file, the failing ones included: a record's index is its index in the file"""
    return rsp.arrays(fm.fuzz(seed, None, window))


@functools.lru_cache(maxsize=None)
def sums_of(seed, mode, window=None):
    """-> ((n, qual, mapq, dist) on every column 0..n_pos-1, the distance marks, n_pos) of the yardstick on the seed's file under the mode"""
    tabled, slack, q, f = fm.MODES[mode]
    sums, marks = ey.whole(fuzz_arrays(seed, window), L, fm.table_of(seed) if tabled else (), q, slack, 0, f)
    n_pos = len(fm.yardstick(seed, None, window, f, tabled, q, slack)[0])
    assert n_pos <= len(sums[0]) and not sums[0][n_pos:].any()
    assert np.array_equal(sums[0][:n_pos], fm.yardstick(seed, None, window, f, tabled, q, slack)[0])
    return tuple(m[:n_pos] for m in sums), marks[:, :n_pos], n_pos


def sparse_columns(seed, n_pos):
    """strand_cases.sparse_columns (40 random columns and both sides of every mask edge of the seed's table): they fit the staging"""
    cols = stc.sparse_columns(seed, n_pos)
    assert len(cols) <= LDS, (len(cols), LDS)
    return cols


def not_vacuous(sums, marks, cols, label, ref=None, capped=False):
    """on the yardstick, before the device runs, among the queried columns: an allele other than the reference's is counted, the three
    sums differ from each other and from n, a token lies at distance 0 (and one at the cap when asked), a D token and an I mark
    contribute"""
    ref = reference() if ref is None else ref
    n, qual, mapq, dist = take(sums, cols)
    other = [(c, pl) for k, c in enumerate(cols) if c < len(ref) for pl in range(1, 7) if n[k, pl] and pl != REF_PLANE.get(ref[c].upper())]
    assert other, (label, "no allele other than the reference's")
    totals = [int(m[:, 0].sum()) for m in (n, qual, mapq, dist)]
    assert len(set(totals)) == 4 and all(totals), (label, "the sums do not differ", totals)
    assert marks[0][cols].sum() > 0, (label, "no token at distance 0")
    assert not capped or marks[1][cols].sum() > 0, (label, "no token at the cap")
    assert n[:, 5].sum() > 0 and n[:, 6].sum() > 0, (label, "no D token or no I mark", n.sum(0).tolist())


@functools.lru_cache(maxsize=None)
def _coverage_without(seed, what):
    """the yardstick's coverage per column on the seed's file under mode "all" with one of floor, mask and filter taken away (None: none)"""
    tabled, slack, q, f = fm.MODES["all"]
    args = {None: (fm.table_of(seed), q, slack, 0, f), "floor": (fm.table_of(seed), 0, slack, 0, f), "mask": ((), q, slack, 0, f),
            "filter": (fm.table_of(seed), q, slack, 0, fm.NONE)}[what]
    return ey.whole(fuzz_arrays(seed), L, *args)[0][0][:, 0]


def removed_by_each(seed, cols, label):
    """case 1's condition: on the queried columns the floor, the mask and the filter of mode "all" each remove a token"""
    have = int(ey.at((_coverage_without(seed, None)[:, None],), cols)[0].sum())
    for what in ("floor", "mask", "filter"):
        assert int(ey.at((_coverage_without(seed, what)[:, None],), cols)[0].sum()) > have, (label, what + " removes nothing")


# ---- hand-made records for the distance rule ---------------------------------------------------------------------------------------------
def hand_records():
    """-> (specs in file order, {name: spec}): every record's bases are the reference's but one, its qualities differ base by base"""
    ref = reference()
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}

    def rec(name, pos, cigar, mapq, flag=0, qual=None, clip=0):
        ops = [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
        seq, x = [], pos
        for n, op in ops:
            if op in "M=X":
                seq += list(ref[x:x + n].upper())
            elif op in "IS":
                seq += list("ACGT" * n)[:n]
            if op in "MDN=X":
                x += n
        k = clip + 3                                                           # one base other than the reference's, inside the first M op
        seq[k] = other[seq[k]]
        q = [hand_quality(j) for j in range(len(seq))] if qual is None else [qual] * len(seq)
        return {"pos": pos, "flag": flag, "cigar": cigar, "seq": "".join(seq), "qual": q, "name": name, "tid": 0, "mapq": mapq}
    specs = [rec("clipped", 100, "5S20M5S", 60, clip=5), rec("hard", 200, "3H4S10M", 0, 16, clip=4), rec("long", 300, "700M", 255),
             rec("del", 1100, "10M3D10M", 60), rec("del_at_end", 1200, "10M2D5S", 60, 16), rec("ins", 1300, "8M3I8M", 255),
             rec("noqual", 1400, "12M", 60, qual=255)]
    specs.sort(key=lambda r: r["pos"])
    return specs, {r["name"]: r for r in specs}


def hand_quality(qi):
    return (7 * qi + 3) % 41 + 1


# what include/tcmi.h's rule gives, worked out by hand: {column: (query index, MAPQ, distance)} of the one record over the column; the
# quality is hand_quality(query index), 255 for the record without QUAL
HAND = {100: (5, 60, 0), 110: (15, 60, 9), 119: (24, 60, 0),                     # 5S20M5S: [a0, a1) = [5, 25)
        200: (4, 0, 0), 204: (8, 0, 4), 209: (13, 0, 0),                         # 3H4S10M: [4, 14), H takes no part
        300: (0, 255, 0), 554: (254, 255, 254), 555: (255, 255, 255), 650: (350, 255, 255), 744: (444, 255, 255), 745: (445, 255, 254),
        999: (699, 255, 0),                                                      # 700M: capped from query index 255 to 444
        1109: (9, 60, 9), 1110: (10, 60, 9), 1112: (10, 60, 9), 1113: (10, 60, 9),      # 10M3D10M: the D columns take the next base's index
        1205: (5, 60, 4), 1209: (9, 60, 0), 1210: (10, 60, 0), 1211: (10, 60, 0),       # 10M2D5S: [0, 10), the D at index 10 = a1: -1 -> 0
        1307: (7, 255, 7), 1308: (11, 255, 7),                                   # 8M3I8M: [0, 19), the mark on index 7, the next base is index 11
        1400: (0, 60, 0), 1405: (5, 60, 5)}                                      # 12M without QUAL: the stored 0xFF


# ---- tests/fixed_reads.py's records in numpy -----------------------------------------------------------------------------------------------
def fixed_counts(rd, cols, q=0, f=(0, 0, 0), table=(), slack=0):
    """-> (n, qual, mapq, dist) int64 [len(cols), 7] for fixed_reads.generate's records (20M each): per offset into the reads one
    weighted bincount over (column, plane) of the tokens that are kept, at or above the floor and outside the read's primer mask; the
    distance of offset o is min(o, 19 - o).  Pinned to tests/evidence_yardstick.py in tests/test_evidence_rule.py."""
    keep, p = fx.kept(rd, f), rd["pos"].astype(np.int64)
    head_end, tail_start = fx.read_mask(rd, table, slack)
    out = np.zeros((4, fx.L * 8), np.int64)
    for o in range(fx.LEN):
        ok = keep & (rd["qual"][:, o] >= q) & (head_end <= p + o) & (p + o < tail_start)
        c, pl = (p + o)[ok], fx.PLANE[rd["base"][:, o]][ok].astype(np.int64)
        weights = (np.ones(len(c), np.int64), rd["qual"][ok, o].astype(np.int64), rd["mapq"][ok].astype(np.int64), np.full(len(c), min(o, fx.LEN - 1 - o), np.int64))
        for k, w in enumerate(weights):                                         # (float64 sums of integers far below 2^53: exact)
            out[k] += np.bincount(c * 8, w, minlength=fx.L * 8).astype(np.int64) + np.bincount((c * 8 + pl)[pl <= 4], w[pl <= 4], minlength=fx.L * 8).astype(np.int64)
    out = out.reshape(4, fx.L, 8)[:, :, :7]
    got = np.zeros((4, len(cols), 7), np.int64)
    inside = [k for k, c in enumerate(cols) if 0 <= c < fx.L]
    got[:, inside] = out[:, [cols[k] for k in inside]]
    return tuple(got)


# ---- what a workgroup's LDS counters reach -------------------------------------------------------------------------------------------------
def token_table(rd, cols, table=(), q=0, slack=0, f=(0, 0, 0)):
    """-> {record index: [(counter, value)]}: what every record of `rd` adds to the [len(cols)][28] counters of a query at `cols`"""
    at = {c: k for k, c in enumerate(cols)}
    per = {}
    for i, (c, planes, qual, mapq, dist) in ey.kept_tokens(rd, table, q, slack, 0, f):
        if c in at:
            per.setdefault(i, []).extend((28 * at[c] + 4 * pl + k, v) for pl in planes for k, v in enumerate((1, qual, mapq, dist)))
    return per


def lds_peak(per, n_small, n_cols, r, cap, block):
    """the largest value a staged (uint32) counter of one workgroup holds on the file that repeats each of n_small records r times in
    place, on a grid that covers `cap` records a trip: workgroup b visits the records [b * block + t * cap, ... + block) of every trip
    t; record j of the repeated file is record j // r of the small one (per: token_table's)"""
    n = r * n_small
    peak = 0
    for b in range(cap // block):
        if b * block + cap >= n and peak >= 255 * block:                        # (one trip only from here on: no counter passes 255 * block)
            break
        cnt = np.zeros(28 * n_cols, np.int64)
        for lo in range(b * block, n, cap):
            j = np.arange(lo, min(lo + block, n)) // r
            for i, m in zip(*np.unique(j, return_counts=True)):
                for k, v in per.get(int(i), ()):
                    cnt[k] += int(m) * v
        peak = max(peak, int(cnt.max()))
    return peak
