"""What the tests of the joint allele counts share (tests/test_link_counts.py, and the record-stream tests that repeat its cases at other
sizes): the device call between guards, the yardstick's class matrix of a fuzz seed, the queried columns, the conditions that keep a
case from being vacuous, and the command line's planted case.  No tests in here."""
import ctypes as C
import functools

import numpy as np

from tests import device_file as dvf
from tests import fuzz_masked as fm
from tests import links_yardstick as ly
from trueconsense_amd import _ffi, engine
from trueconsense_amd import synthetic as syn

L = fm.L
LDS = engine.LINKS_LDS
G = 64                                                                          # guard words on either side of the records
W = 52                                                                          # int32 words of a record


def device_links(ctx, rs, cols, k):
    """tcmi_readset_link_counts into a host buffer between guards -> the records (LINK_DTYPE); a, b and reserved are checked here, and
    Context.link_counts must give the same bytes (run after run)"""
    cols = np.ascontiguousarray(cols, np.int64)
    n = len(cols)
    buf = dvf.sentinel(2 * G + W * n * k, np.int32, salt=11).copy()
    before = buf.copy()
    rc = _ffi.lib().tcmi_readset_link_counts(ctx.handle, rs.handle, n, _ffi.ptr(cols), k, C.c_void_p(buf.ctypes.data + 4 * G))
    _ffi.check(rc, ctx.handle)
    assert np.array_equal(buf[:G], before[:G]) and np.array_equal(buf[-G:], before[-G:]), "a guard around the records was written"
    got = buf[G:-G].view(engine.LINK_DTYPE).copy()
    want = ly.records(cols.tolist(), k, np.zeros((n * k, 7, 7), np.int32))
    assert np.array_equal(got["a"], want["a"]) and np.array_equal(got["b"], want["b"]) and not got["reserved"].any(), \
        (got["a"][:8].tolist(), want["a"][:8].tolist(), got["b"][:8].tolist(), want["b"][:8].tolist(), int(got["reserved"].any()))
    assert not got["j"][got["b"] < 0].any() and not got["j"][:, 0, 0].any(), "counts in a record without a pair, or in the class (none, none)"
    again = ctx.link_counts(rs, cols, k)
    assert again.tobytes() == got.tobytes(), "Context.link_counts gave other bytes than the call before it"
    return got


def differ(got, want_j, label):
    """'' when the records' counts equal the yardstick's; else the first differing pairs with both matrices"""
    if np.array_equal(got["j"], want_j):
        return ""
    rows = []
    for p in np.unique(np.argwhere(got["j"] != want_j)[:, 0])[:4].tolist():
        rows.append("pair (%d, %d): got\n%r\nwant\n%r" % (got["a"][p], got["b"][p], got["j"][p], want_j[p]))
    return "%r (classes none, A, T, C, G, X, coverage only)\n%s" % (label, "\n".join(rows))


@functools.lru_cache(maxsize=None)
def classes_of(seed, mode, window=None):
    """-> (class matrix [passing records, n_pos], n_pos, the yardstick's count matrix) of a fuzz seed under a mode"""
    tabled, slack, q, f = fm.MODES[mode]
    _, rd = fm.passing(seed, None, window, f)
    whole = fm.yardstick(seed, None, window, f, tabled, q, slack)[0]
    return ly.classes(rd, L, fm.table_of(seed) if tabled else (), q, slack, n_pos=len(whole)), len(whole), whole


def sparse_columns(seed, n_pos, n=24, edges=8):
    """24 random columns and columns on both sides of mask edges of the seed's table: at most 40, staged with one and two neighbours"""
    rng = np.random.default_rng(700 + seed)
    cols = set(int(c) for c in rng.choice(n_pos, n, replace=False))
    for s, e, rev in fm.table_of(seed)[:edges]:
        edge = s if rev else e
        cols.update(c for c in (edge - 1, edge) if 0 <= c < n_pos)
    assert len(cols) * 2 <= LDS, (len(cols), LDS)
    return sorted(cols)


def window_columns(whole, width=300):
    """every column of the 300-column window with the most coverage"""
    cov = np.convolve(whole[:, 0].astype(np.int64), np.ones(width, np.int64), "valid")
    s = int(np.argmax(cov))
    return list(range(s, s + width))


def long_read_over(specs, cols, at_least=3):
    """does a long read (one the tally leaves to its per-token kernel) lie over several of the queried columns?"""
    return any(fm._piles_up(r) and fm._span(r) > fm.LONG and sum(r["pos"] <= c < r["pos"] + fm._span(r) for c in cols) >= at_least for r in specs)


def not_vacuous(j, label):
    """on the yardstick, before the device runs: a pair with an off-diagonal count among the classes 1..6, records that reach only the
    first column of a pair and records that reach only the second"""
    off = j[:, 1:, 1:].sum(0)
    assert (off - np.diag(np.diag(off))).any(), label
    assert j[:, 1:, 0].any() and j[:, 0, 1:].any(), label


# ---- the command line's case ---------------------------------------------------------------------------------------------------------------
CL = 1200
CIS, TRANS, MIXED, LOW = (300, 330), (600, 640), (800, 830), (1000, 1095)       # the planted pairs' 0-based columns


@functools.lru_cache(maxsize=None)
def cli_case():
    """-> (reference, GFF rows, records): 100-base reads at about 60x over 1 200 columns.  Of the reads over a planted pair a third
    carry another base at both columns of CIS; three in ten at the first column of TRANS only and three in ten at its second only; a
    quarter at both columns of MIXED, a quarter at its first only, a quarter at its second only; four in ten at either column of LOW,
    which only the reads that start in five columns span"""
    rng = np.random.default_rng(78)
    ref, orfs = syn.make_reference(seed=3, L=CL, cds=[(100, 900)])
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}
    specs = []
    for k in range(720):
        pos = int(rng.integers(0, CL - 100 + 1))
        seq = list(ref[pos:pos + 100])
        r = rng.random(4)
        hits = ((CIS[0], r[0] < 0.33), (CIS[1], r[0] < 0.33), (TRANS[0], r[1] < 0.3), (TRANS[1], 0.3 <= r[1] < 0.6), (MIXED[0], r[2] < 0.5),
                (MIXED[1], r[2] < 0.25 or 0.5 <= r[2] < 0.75), (LOW[0], r[3] < 0.4), (LOW[1], r[3] < 0.4))
        for col, hit in hits:
            if hit and pos <= col < pos + 100:
                seq[col - pos] = other[ref[col].upper()]
        specs.append({"pos": pos, "flag": 16 if k % 2 else 0, "cigar": "100M", "seq": "".join(seq), "name": "r%d" % k, "tid": 0, "qual": 30, "mapq": 60})
    specs.sort(key=lambda r: r["pos"])
    return ref, orfs, specs
