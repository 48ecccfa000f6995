"""Inputs for tests/test_floor_mask_fuzz.py: read sets with random CIGARs (every op of fuzz_reads.random_cigar, short and long), per-base
qualities around the floor, SEQ '*' / short SEQ / no QUAL, filterable MAPQ and FLAG bits, and insertion sites planted on the mask edges
of the primer table the test will use; random primer tables; tables of a chosen number of segments.  No tests in here."""
import numpy as np

from tests import fuzz_reads as fz
from tests import test_read_filter as rf
from trueconsense_amd import synthetic as sy

FLAGS = (0, 16, 0, 16, 4, 0x400)


def primers(seed, L=2000, n=40):
    """a random table as test_primer_mask.test_compiled_table_equals_brute_force builds one: uniform starts, lengths 1 - 33 (every
    fourth up to 119), random strand, every fifth primer on the previous one's start (an alternative primer)"""
    rng = np.random.default_rng(1000 + seed)
    out = []
    for k in range(n):
        s = int(rng.integers(0, L - 40))
        if out and k % 5 == 0:
            s = out[-1][0]
        out.append((s, s + int(rng.integers(1, 120 if k % 4 == 0 else 34)), bool(rng.integers(0, 2))))
    return out


def dense_table(n, plus_only=False):
    """n primers of three columns, six apart, '+' and '-' in turn: none overlaps another, so each is exactly one segment"""
    return [(6 * k, 6 * k + 3, bool(k & 1) and not plus_only) for k in range(n)]


def edge_columns(rng, table, L, n=4):
    """the columns on both sides of a mask edge of `n` of the table's primers: end - 1 and end of a '+', start - 1 and start of a '-'"""
    ok = [(s, e, rev) for s, e, rev in table if 35 <= (s if rev else e) <= L - 45]
    if not ok:
        return []
    out = []
    for k in rng.choice(len(ok), min(n, len(ok)), replace=False):
        s, e, rev = ok[int(k)]
        edge = s if rev else e
        out += [edge - 1, edge]
    return out


def specs(seed, n_short=1500, n_long=150, L=2000, window=None, refname_tid=0, table=None):
    """-> position-sorted read dicts for test_read_filter.arrays.  window = (a, b): every random read starts in [a, b) (depth).
    table: the primers whose mask edges the planted insertion sites sit on (without one: random columns)."""
    rng = np.random.default_rng(seed)
    ref, _ = sy.make_reference(seed=3, L=L, cds=[])
    tid = refname_tid
    out = []
    for tag, n, long_reads in (("f", n_short, False), ("g", n_long, True)):
        for k in range(n):
            cig = fz.random_cigar(rng, long_reads=long_reads)
            span = fz._span(cig)
            if span == 0 or span > L - 10:
                continue
            if window is None:
                pos = int(rng.integers(0, L - span + 1))
            else:
                pos = min(int(rng.integers(window[0], window[1])), L - span)
            r = fz._read(rng, ref, pos, cig, FLAGS[int(rng.integers(0, len(FLAGS)))], "%s%d" % (tag, k), tid)
            how = rng.random()
            if how < 0.04:
                fz._shorten(rng, r, "star")
            elif how < 0.08:
                fz._shorten(rng, r, "short")
            out.append(r)
    cols = edge_columns(rng, table, L) if table else []
    for k, shape in enumerate(fz._SHAPES):
        c = cols[k % len(cols)] if cols else int(rng.integers(35, L - 45))
        out += fz._site(rng, ref, L, c, "k%d" % k, tid, 12, shape, int(rng.integers(2, 9)), False)
    out.sort(key=lambda r: r["pos"])
    return rf.randomise(rng, out)
