"""What the tests of the per-strand counts share (tests/test_strand_counts.py, and the record-stream tests that repeat its cases at
other sizes): the device call between guards, the yardstick's halves of a fuzz seed, the queried columns, the conditions that keep a
case from being vacuous.  No tests in here."""
import ctypes as C
import functools

import numpy as np

from tests import device_file as dvf
from tests import fuzz_masked as fm
from tests import strand_yardstick as sy
from trueconsense_amd import _ffi, engine

L = fm.L
LDS = engine.STRAND_LDS
G = 64                                                                          # guard words on either side of the records
assert fm.FLAGS.count(16) == 2 and len(fm.FLAGS) == 6, fm.FLAGS


def device_counts(ctx, rs, cols):
    """tcmi_readset_strand_counts into a host buffer between guards -> (fwd, rev) int32 [n, 7]; pos and reserved are checked here, and
    Context.strand_counts must give the same numbers (run after run)"""
    cols = np.ascontiguousarray(cols, np.int64)
    n = len(cols)
    buf = dvf.sentinel(2 * G + 16 * n, np.int32, salt=7).copy()
    before = buf.copy()
    rc = _ffi.lib().tcmi_readset_strand_counts(ctx.handle, rs.handle, n, _ffi.ptr(cols), C.c_void_p(buf.ctypes.data + 4 * G))
    _ffi.check(rc, ctx.handle)
    assert np.array_equal(buf[:G], before[:G]) and np.array_equal(buf[-G:], before[-G:]), "a guard around the records was written"
    got = buf[G:-G].view(engine.STRAND_DTYPE).copy()
    assert np.array_equal(got["pos"], cols) and not got["reserved"].any(), (got["pos"][:8].tolist(), cols[:8].tolist(), int(got["reserved"].any()))
    again = ctx.strand_counts(rs, cols)
    assert np.array_equal(got["fwd"], again["fwd"]) and np.array_equal(got["rev"], again["rev"]) and np.array_equal(again["pos"], cols), \
        "Context.strand_counts gave other numbers than the call before it"
    return got["fwd"], got["rev"]


def differ(got, want, cols, label):
    """'' when (fwd, rev) equal the yardstick's; else the first differing columns with both rows"""
    if all(np.array_equal(g, w) for g, w in zip(got, want)):
        return ""
    rows = []
    for name, g, w in zip(("fwd", "rev"), got, want):
        for k in np.unique(np.argwhere(g != w)[:, 0])[:6].tolist():
            rows.append("%s column %d: got %r want %r" % (name, cols[k], g[k].tolist(), w[k].tolist()))
    return "%r (coverage, A, T, C, G, X, I)\n%s" % (label, "\n".join(rows))


@functools.lru_cache(maxsize=None)
def halves(seed, mode, window=None):
    """-> (fwd, rev) of the yardstick on every column 0..n_pos-1, n_pos: the extent of the yardstick over all passing records"""
    tabled, slack, q, f = fm.MODES[mode]
    _, rd = fm.passing(seed, None, window, f)
    n_pos = len(fm.yardstick(seed, None, window, f, tabled, q, slack)[0])
    fwd, rev = sy.counts(rd, range(n_pos), L, fm.table_of(seed) if tabled else (), q, slack)
    return fwd, rev, n_pos


def sparse_columns(seed, n_pos, n=40):
    """40 random columns and the columns on both sides of every mask edge of the seed's table"""
    rng = np.random.default_rng(500 + seed)
    cols = set(int(c) for c in rng.choice(n_pos, n, replace=False))
    for s, e, rev in fm.table_of(seed):
        edge = s if rev else e
        cols.update(c for c in (edge - 1, edge) if 0 <= c < n_pos)
    assert len(cols) <= LDS, (len(cols), LDS)
    return sorted(cols)


def long_read_covers(specs, cols):
    return any(fm._piles_up(r) and fm._span(r) > fm.LONG and any(r["pos"] <= c < r["pos"] + fm._span(r) for c in cols) for r in specs)


def not_vacuous(specs, fwd, rev, cols, label):
    """on the yardstick, before the device runs: both strands have a non-zero count in every plane among the queried columns, and a
    long read covers one of them"""
    assert fwd.sum(0).all() and rev.sum(0).all(), (label, fwd.sum(0).tolist(), rev.sum(0).tolist())
    assert long_read_covers(specs, cols), label


@functools.lru_cache(maxsize=None)
def one_column_a_record():
    """-> (specs, cols): 65 kept records, 6 all-match bases each.  Record r < 64 starts at column 100 + 10 r, so no two of them share
    a column: the first wavefront holds 64 distinct counters a round, one pass of the join per lane.  Record 64 lies on record 0's
    columns, on the other strand, alone in a second, ragged wavefront.  cols: one queried column per record (also used by
    test_link_counts)"""
    def rec(r, pos, flag):
        return {"pos": pos, "flag": flag, "cigar": "6M", "seq": "ACGT"[r % 4] * 6, "name": "j%d" % r, "tid": 0, "qual": 30, "mapq": 60}
    specs = [rec(r, 100 + 10 * r, 16 if r % 3 == 0 else 0) for r in range(64)] + [rec(64, 100, 0)]
    return specs, [100 + 10 * r + r % 6 for r in range(64)]
