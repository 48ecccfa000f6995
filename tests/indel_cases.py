"""Inputs of the --indel-table tests and their non-vacuity conditions: the fuzz files' events on the yardstick (cached), the queries,
the hand-built file "one wave, many keys" with a pair of insertions whose hashes collide in 8 bits under seed 0 and under no other
seed the call gets to, and the call on the device with every host buffer between guard words.  No tests in here."""
import ctypes as C
import functools

import numpy as np

from tests import device_file as dvf
from tests import fuzz_masked as fm
from tests import indel_yardstick as iy
from tests import read_specs as rsp
from trueconsense_amd import _ffi, engine

L = fm.L
LDS = engine.INDEL_LDS
G = dvf.GUARD
EVERYTHING = dict(num=0, den=1, min_alt_depth=1, min_depth=0)                   # thresholds 0 / 1: every event is reported
TENTH = dict(num=1, den=10, min_alt_depth=1, min_depth=0)                       # --min-af 1/10


@functools.lru_cache(maxsize=None)
def fuzz_events(seed, mode):
    """-> (the yardstick's {event: records}, {column: [ins_total, del_total]}, the yardstick's matrix) of a fuzz file under a mode"""
    tabled, slack, q, f = fm.MODES[mode]
    counts, totals = iy.events(fm.fuzz(seed), fm.table_of(seed) if tabled else (), q, slack, f)
    return counts, totals, fm.yardstick(seed, None, None, f, tabled, q, slack)[0]


def sparse_columns(seed, counts, n_pos, n=200):
    """n columns, within the LDS staging: half of them columns with an event, half anywhere"""
    rng = np.random.default_rng(70 + seed)
    with_event = sorted({ev[0] for ev in counts})
    ins_cols = [ev[0] for ev in counts if ev[1] == iy.INS]
    some = set(sorted(c for c in set(ins_cols) if ins_cols.count(c) > 1)[:n // 4])       # columns with two different insertions
    some |= set(int(c) for c in rng.choice(with_event, min(n // 2, len(with_event)), replace=False))
    some |= set(int(c) for c in rng.choice(n_pos, n - len(some), replace=False))
    cols = sorted(some)
    assert len(cols) <= LDS < n_pos
    return cols


def not_vacuous(counts, cols, cov, label):
    """the query has insertions and deletions, an event of several records, two different insertions on one column, and the 1/10 rule
    both drops and keeps events"""
    cols = set(cols)
    mine = {ev: n for ev, n in counts.items() if ev[0] in cols}
    kinds = [ev[1] for ev in mine]
    assert kinds.count(iy.INS) >= 10 and kinds.count(iy.DEL) >= 10 and max(mine.values()) >= 3, (label, len(mine))
    ins_cols = [ev[0] for ev in mine if ev[1] == iy.INS]
    assert len(ins_cols) > len(set(ins_cols)), (label, "no column with two different insertions")
    all_, tenth = iy.reported(counts, sorted(cols), cov), iy.reported(counts, sorted(cols), cov, **TENTH)
    assert 0 < len(tenth) < len(all_), (label, len(tenth), len(all_))


def device_events(ctx, rs, cols, cov, num=0, den=1, min_alt_depth=1, min_depth=0):
    """tcmi_readset_indel_events through the C ABI: the sizing call, then the call with buffers of exactly that size, each between guard
    words that must be intact afterwards -> ([(column, kind, len, bases, count, cov)], totals as TOTALS_DTYPE)"""
    cols = np.ascontiguousarray(cols, np.int64)
    cov = np.ascontiguousarray(cov, np.int32)
    n, tl = C.c_int64(-1), C.c_int64(-1)
    lib = _ffi.lib()
    head = (ctx.handle, rs.handle, len(cols), _ffi.ptr(cols), _ffi.ptr(cov), num, den, min_alt_depth, min_depth)
    tot = dvf.sentinel(2 * G + 4 * len(cols), np.int32, salt=5).copy()
    p_tot = C.c_void_p(tot.ctypes.data + 4 * G)
    _ffi.check(lib.tcmi_readset_indel_events(*head, None, 0, C.byref(n), None, 0, C.byref(tl), p_tot), ctx.handle)
    sized = (n.value, tl.value, tot[G:G + 4 * len(cols)].copy())
    ev = dvf.sentinel(2 * G + 8 * n.value, np.int32, salt=6).copy()
    tx = dvf.sentinel(2 * G + tl.value, np.uint8, salt=7).copy()
    before = [a.copy() for a in (tot, ev, tx)]
    _ffi.check(lib.tcmi_readset_indel_events(*head, C.c_void_p(ev.ctypes.data + 4 * G), sized[0], C.byref(n), C.c_void_p(tx.ctypes.data + G), sized[1],
                                             C.byref(tl), p_tot), ctx.handle)
    assert (n.value, tl.value) == sized[:2] and np.array_equal(tot[G:G + 4 * len(cols)], sized[2]), "the sizing call and the call disagree"
    for a, b, lo in zip((tot, ev, tx), before, (G, G, G)):
        assert np.array_equal(a[:lo], b[:lo]) and np.array_equal(a[len(a) - G:], b[len(b) - G:]), "a guard was written"
    if n.value:                                                                 # (a short buffer: E_ARG, the sizes again, nothing written)
        n2, tl2 = C.c_int64(-1), C.c_int64(-1)
        ev2 = ev.copy()
        rc = lib.tcmi_readset_indel_events(*head, C.c_void_p(ev2.ctypes.data + 4 * G), sized[0] - 1, C.byref(n2), C.c_void_p(tx.ctypes.data + G), sized[1],
                                           C.byref(tl2), p_tot)
        assert rc == _ffi.E_ARG and (n2.value, tl2.value) == sized[:2] and np.array_equal(ev2, ev)
    events = ev[G:G + 8 * n.value].view(iy.EVENT_DTYPE)
    totals = tot[G:G + 4 * len(cols)].view(iy.TOTALS_DTYPE)
    assert not events["reserved"].any() and not totals["reserved"].any()
    return iy.unpack(events, tx[G:G + tl.value].tobytes()), totals.copy()


def differ(got, want, label):
    """'' when the lists are equal, else the label and the first events only one of them has"""
    if got == want:
        return ""
    a, b = set(got), set(want)
    return "%r: %d events, the yardstick's %d; only on the device %r; only on the yardstick %r; order %s" % (
        label, len(got), len(want), sorted(a - b)[:6], sorted(b - a)[:6], "equal" if sorted(got) == sorted(want) else "differs")


# ---- one wave, many keys -----------------------------------------------------------------------------------------------------------------
COL = 1000                                                                      # the column every event of the hand-built file is anchored on
SHARED, OTHERS, LONGER = "ACG", ("ACT", "TTT", "GGA"), "ACGT"
N_SHARED = 300                                                                  # consecutive records: five wavefronts, two workgroups


def nibbles(bases):
    return [iy.ss.NT16.index(b) for b in bases]


@functools.lru_cache(maxsize=None)
def colliding_pair():
    """two insertions of five bases whose 8-bit hashes are equal under seed 0 — and such that under seed 1 no two of the file's
    insertions share one: the call repeats exactly once.  Found with tcmi_indel_hash, checked against the restatement."""
    rng = np.random.default_rng(5)
    fixed = [SHARED, LONGER, "AC"] + list(OTHERS) + list(SINGLETONS)
    seen = {}
    for _ in range(20000):
        s = "".join("ACGT"[int(k)] for k in rng.integers(0, 4, 5))
        h0 = engine.indel_hash(0, nibbles(s), 8)
        assert h0 == iy.hash_(0, nibbles(s), 8)
        if h0 in seen and seen[h0] != s:
            every = fixed + [seen[h0], s]
            h1 = [engine.indel_hash(1, nibbles(x), 8) for x in every]
            if len(set(h1)) == len(h1):
                return seen[h0], s
        seen.setdefault(h0, s)
    raise AssertionError("no colliding pair found")


SINGLETONS = ("CAT", "GATTACA", "T", "GG", "CCCCC", "TGCATG", "AAAAAAAAAAAA", "CGCG", "NAC", "AGGA", "TTTTTTT", "CTAGCTAG")


@functools.lru_cache(maxsize=None)
def many_keys():
    """-> (records, {event: records} as the test states them by hand): ~400 records with an event on COL"""
    rng = np.random.default_rng(77)
    pair = colliding_pair()
    specs, want = [], {}

    def ins(bases, n, tag):
        for k in range(n):
            seq = "".join("ACGT"[int(t)] for t in rng.integers(0, 4, 51)) + bases + "".join("ACGT"[int(t)] for t in rng.integers(0, 4, 40))
            specs.append(rsp.mk(rng, COL - 50, [(51, "M"), (len(bases), "I"), (40, "M")], [30] * len(seq), "%s%d" % (tag, k), seq))
        want[(COL, iy.INS, len(bases), bases)] = want.get((COL, iy.INS, len(bases), bases), 0) + n

    def dele(n_del, n, tag):
        for k in range(n):
            specs.append(rsp.mk(rng, COL - 51, [(51, "M"), (n_del, "D"), (40, "M")], [30] * 91, "%s%d" % (tag, k)))
        want[(COL, iy.DEL, n_del, "")] = n

    dele(3, 12, "d3_")
    dele(9, 7, "d9_")
    ins(SHARED, N_SHARED, "shared")
    for k, (bases, n) in enumerate(zip(OTHERS, (20, 10, 5))):
        ins(bases, n, "other%d_" % k)
    ins(LONGER, 8, "longer")
    ins(pair[0], 6, "pa")
    ins(pair[1], 4, "pb")
    for k, bases in enumerate(SINGLETONS):
        ins(bases, 1, "single%d_" % k)
    # "1D" + I: a deletion of one column AND an insertion on it, from one record
    seq = "".join("ACGT"[int(t)] for t in rng.integers(0, 4, 50)) + "AC" + "".join("ACGT"[int(t)] for t in rng.integers(0, 4, 40))
    specs.append(rsp.mk(rng, COL - 50, [(50, "M"), (1, "D"), (2, "I"), (40, "M")], [30] * 92, "d1i", seq))
    want[(COL, iy.DEL, 1, "")] = 1
    want[(COL, iy.INS, 2, seq[50:52])] = want.get((COL, iy.INS, 2, seq[50:52]), 0) + 1
    for k in range(30):                                                         # plain reads over the column
        specs.append(rsp.mk(rng, COL - 45, [(91, "M")], [30] * 91, "plain%d" % k))
    return specs, want
