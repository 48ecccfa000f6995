"""Fuzzed inputs for the base-quality floor, the primer mask and the read filter together (tests/test_floor_mask_fuzz.py and every
record-stream test after it): read sets with random CIGARs (every op of fuzz_reads.random_cigar, short and long), per-base qualities
around the floor, SEQ '*' / short SEQ / no QUAL, filterable MAPQ and FLAG bits, and insertion sites planted on the mask edges of the
primer table the test will use; random primer tables; tables of a chosen number of segments; the seeds and modes the tests run, their
records, arrays and yardsticks (cached: computed once a process), and what a failure is analysed from.  No tests in here."""
import functools

import numpy as np

from tests import fuzz_reads as fz
from tests import primer_yardstick as py
from tests import read_specs as rs
from tests import synth_small as ss
from trueconsense_amd import synthetic as sy
from trueconsense_amd.io import bamwriter

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
    """-> position-sorted read dicts for read_specs.arrays.  window = (a, b): every random read starts in [a, b) (depth).
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
    return rs.randomise(rng, out)


# ---- the seeds and modes the tests run ---------------------------------------------------------------------------------------------------
L = rs.L
SEEDS = (1, 2, 3, 4)
DEEP_SEED, DEEP_WINDOW = 5, (975, 1025)                                          # (narrowed from (900, 1100) until the depth passes 255)
F = (20, 0, 0x800)
NONE = (0, 0, 0)
LONG = 512                                                                      # a read of more columns is left to tally_stream_kernel
# mode -> (under the seed's table?, slack, floor, read filter)
MODES = {"floor": (False, 0, 13, NONE), "table": (True, 0, 0, NONE), "all": (True, 3, 13, F)}
CONTIGS = (("c0", 1500, 11), ("c1", 1200, 12))                                  # name, columns, seed


@functools.lru_cache(maxsize=None)
def table_of(key):
    """key: a seed's random table, or ("dense", n, plus_only)"""
    return tuple(dense_table(*key[1:])) if isinstance(key, tuple) else tuple(primers(key))


@functools.lru_cache(maxsize=None)
def fuzz(seed, key=None, window=None):
    """the records of a seed, their insertion sites planted on the mask edges of table_of(key) (key None: the seed's own table)"""
    return specs(seed, table=table_of(seed if key is None else key), window=window)


@functools.lru_cache(maxsize=None)
def passing(seed, key=None, window=None, f=NONE):
    """-> (the records that pass f, their arrays)"""
    every = fuzz(seed, key, window)
    b = rs.kept(every, f)[0] if f != NONE else every
    return b, rs.arrays(b)


@functools.lru_cache(maxsize=None)
def yardstick(seed, key=None, window=None, f=NONE, table=False, q=0, slack=0):
    return py.counts(passing(seed, key, window, f)[1], L, table_of(seed if key is None else key) if table else (), q, slack)


@functools.lru_cache(maxsize=None)
def contig_case():
    """-> ([(name, columns, that contig's table, its records with tid = its index)], every record in file order)"""
    parts, every = [], []
    for t, (name, ln, seed) in enumerate(CONTIGS):
        table = primers(seed, L=ln, n=30)
        part = specs(seed, n_short=800, n_long=150, L=ln, refname_tid=t, table=table)
        parts.append((name, ln, table, part))
        every += part
    return parts, every


def write(tmp_path, records, **kw):
    path = str(tmp_path / "A.bam")
    kw.setdefault("block", 4096)
    bamwriter.write_bam(path, rs.arrays(records), ref_len=L, **kw)
    return path


# ---- what the conditions on the inputs count, and what a failure is analysed from --------------------------------------------------------
def _ops(r):
    return ss.parse_cigar(r["cigar"])                                           # [(op index in "MIDNSHP=X", length)]


def _span(r):
    return sum(n for op, n in _ops(r) if op in (0, 2, 3, 7, 8))


def _piles_up(r):
    return not r["flag"] & 4 and r.get("tid", 0) >= 0 and _span(r) > 0


def covering(records, c):
    """name, POS, CIGAR and len(SEQ) of every piled-up record over 0-based column c"""
    return [(r["name"], r["pos"], r["cigar"], 0 if r["seq"] == "*" else len(r["seq"])) for r in records
            if _piles_up(r) and r["pos"] <= c < r["pos"] + _span(r)]


def differ(got, want, records, label):
    """'' when the matrices are equal; else what a failure is analysed from without another run: the label (seed, mode, packer), the
    first eight differing columns with both rows, and every passing record over the first of them"""
    if got.shape == want.shape and np.array_equal(got, want):
        return ""
    if got.shape != want.shape:
        return "%r: shape %r, the yardstick's %r" % (label, got.shape, want.shape)
    cols = np.unique(np.argwhere(got != want)[:, 0])[:8].tolist()
    rows = ["column %d: got %r want %r" % (c, got[c].tolist(), want[c].tolist()) for c in cols]
    reads = ["%s POS %d %s len(seq) %d" % t for t in covering(records, cols[0])]
    return "%r (coverage, A, T, C, G, X, I)\n%s\nrecords over column %d:\n%s" % (label, "\n".join(rows), cols[0], "\n".join(reads))


def n_long(records):
    return sum(_piles_up(r) and _span(r) > LONG for r in records)


def profile(records, table, slack):
    """what the non-vacuity conditions count, on records that all pass the filter"""
    ops, lead = set(), dict.fromkeys("DNIP", 0)
    long_ = long_masked = n_masked = crossing = star = short = noqual = 0
    for r in records:
        if not _piles_up(r):
            continue
        cig = _ops(r)
        ops.update("MIDNSHP=X"[op] for op, _ in cig)
        first = next("MIDNSHP=X"[op] for op, _ in cig if op not in (4, 5))
        if first in lead:
            lead[first] += 1
        p, span = r["pos"], _span(r)
        he, ts = py.read_mask(p, p + span - 1, table, slack)
        masked = he > p or ts <= p + span - 1
        n_masked += masked
        if span > LONG:
            long_ += 1
            long_masked += masked
        x = p
        for op, n in cig:
            if op in (2, 3):
                crossing += x < he < x + n or x < ts < x + n
            if op in (0, 2, 3, 7, 8):
                x += n
        qlen = sum(n for op, n in cig if op in (0, 1, 4, 7, 8))
        star += r["seq"] == "*"
        short += r["seq"] != "*" and len(r["seq"]) < qlen
        noqual += bool(r["qual"]) and r["qual"][0] == 255
    return dict(ops=ops, lead=lead, long=long_, long_masked=long_masked, masked=n_masked, crossing=crossing, star=star, short=short, noqual=noqual)
