"""Hand-made read pairs for the mate-overlap rule (--mate-overlap) on a 600-column reference, as record specs (read_specs.mk's dicts with
mtid / mpos), and a paired fuzz on top of fuzz_reads' CIGARs.  Every group has a name of its own; `expect` says what the rule must make of
the hand-made ones (the yardstick is checked against it in tests/test_mate_rule.py).  No tests in here."""
import functools

import numpy as np

from tests import fuzz_reads as fz
from tests import read_specs as rs
from tests import synth_small as ss

L = 600
REFS = [("ref", L), ("other", 300)]
FIRST, LAST = 99, 147                                   # 0x1 | 0x2 | 0x20 | 0x40 and 0x1 | 0x2 | 0x10 | 0x80
FILTER = (20, 0, 0)                                     # --min-mapq 20: the "winner fails the filter" pair
FLOOR = 13
# '+' primers mask a head, '-' primers a tail (start, end, reverse): the scheme the primer cases are placed on
PRIMERS = [(30, 54, False), (406, 430, True), (330, 354, False), (706, 730, True)]


def _cig(text):
    return [(n, "MIDNSHP=X"[op]) for op, n in ss.parse_cigar(text)]


def _rec(rng, name, flag, pos, cigar, mpos, mtid=0, mapq=60, qual=None):
    r = rs.mk(rng, pos, _cig(cigar), qual, name, flag=flag)
    r.update(mtid=mtid, mpos=mpos, mapq=mapq, tlen=0)
    return r


def _pair(rng, name, p1, c1, p2, c2, flags=(FIRST, LAST), **kw):
    return [_rec(rng, name, flags[0], p1, c1, p2, **kw), _rec(rng, name, flags[1], p2, c2, p1, **kw)]


@functools.lru_cache(maxsize=None)
def cases():
    """-> (specs in file order, expect): expect[name] = the clip of the group's loser (the LAST record of that name in the file unless
    the name is in `first_loses`), or None when the group is no pair"""
    rng = np.random.default_rng(77)
    out, expect = [], {}

    def add(name, recs, clip):
        out.extend(recs)
        expect[name] = clip

    # ---- geometry
    add("partial", _pair(rng, "partial", 10, "60M", 40, "60M"), 30)
    add("contained", _pair(rng, "contained", 100, "100M", 120, "30M"), 30)
    add("identical", _pair(rng, "identical", 210, "50M", 210, "50M"), 50)
    add("eq_first_then_last", _pair(rng, "eq_first_then_last", 270, "40M", 270, "30M"), 30)
    add("eq_last_then_first", _pair(rng, "eq_last_then_first", 270, "30M", 270, "40M", flags=(LAST, FIRST)), 30)      # (the 0x80 record comes first and loses)
    add("adjacent", _pair(rng, "adjacent", 320, "20M", 340, "20M"), 0)
    add("disjoint", _pair(rng, "disjoint", 370, "20M", 420, "20M"), 0)
    add("far_apart", _pair(rng, "far_apart", 0, "1M585N14M", 585, "15M"), 15)                   # (nearly every other record lies between the mates)
    # ---- not eligible / not a pair
    add("other_ref", [_rec(rng, "other_ref", FIRST, 12, "50M", 30, mtid=1), _rec(rng, "other_ref", LAST, 30, "50M", 12, mtid=1)], None)
    add("off_by_one", [_rec(rng, "off_by_one", FIRST, 30, "50M", 61), _rec(rng, "off_by_one", LAST, 60, "50M", 30)], None)
    add("mismatch", [_rec(rng, "mismatch", FIRST, 30, "50M", 60), _rec(rng, "mismatch", LAST, 30, "45M", 60)], None)
    add("not_proper", _pair(rng, "not_proper", 50, "50M", 70, "50M", flags=(FIRST & ~2, LAST)), None)
    add("mate_unmapped_bit", _pair(rng, "mate_unmapped_bit", 55, "50M", 75, "50M", flags=(FIRST | 8, LAST)), None)
    add("with_extras", _pair(rng, "with_extras", 80, "50M", 100, "50M") +
        [_rec(rng, "with_extras", FIRST | 0x100, 85, "40M", 100), _rec(rng, "with_extras", LAST | 0x800, 100, "20M", 80)], 30)
    add("twice", _pair(rng, "twice", 130, "50M", 150, "50M") + _pair(rng, "twice", 130, "48M", 150, "47M"), None)
    add("two_firsts", _pair(rng, "two_firsts", 160, "50M", 180, "50M", flags=(FIRST, FIRST | 16)), None)
    add("low_mapq_winner", [_rec(rng, "low_mapq_winner", FIRST, 190, "50M", 215, mapq=5), _rec(rng, "low_mapq_winner", LAST, 215, "50M", 190)], 25)
    add("unmapped_winner", [_rec(rng, "unmapped_winner", FIRST | 4, 220, "50M", 240), _rec(rng, "unmapped_winner", LAST, 240, "50M", 220)], None)
    # ---- CIGARs in the clipped prefix
    add("del_first_col", _pair(rng, "del_first_col", 450, "20M", 460, "9M4D10M"), 10)           # (the edge behind the deletion's first column)
    add("del_later_col", _pair(rng, "del_later_col", 450, "22M", 460, "9M4D10M"), 12)           # (... behind its third)
    add("ins_inside", _pair(rng, "ins_inside", 480, "25M", 500, "5M2I10M"), 5)                  # (the token in front of the I is the clip's last)
    add("ins_outside", _pair(rng, "ins_outside", 480, "24M", 500, "5M2I10M"), 4)                # (... the first behind it)
    add("clips_in_front", _pair(rng, "clips_in_front", 520, "30M", 530, "3H2S20M1S"), 20)
    add("skip", _pair(rng, "skip", 540, "12M", 545, "5M10N10M"), 7)
    add("long_above", _pair(rng, "long_above", 100, "50M1100N50M", 150, "30M1150N20M"), 1150)   # (the loser spans 1 200 columns: the long-read path)
    add("long_below", _pair(rng, "long_below", 120, "200M", 200, "40M1100N40M"), 120)
    # ---- names
    add("x", _pair(rng, "x", 560, "20M", 570, "20M"), 10)
    n254 = "n" * 250 + "_254"
    add(n254, _pair(rng, n254, 560, "20M", 570, "20M"), 10)
    add("last_byteA", _pair(rng, "last_byteA", 562, "20M", 572, "20M"), 10)
    add("last_byteB", _pair(rng, "last_byteB", 562, "20M", 572, "21M"), 10)
    add("pre", _pair(rng, "pre", 564, "20M", 574, "20M"), 10)
    add("prefix", _pair(rng, "prefix", 564, "20M", 574, "22M"), 10)
    # ---- with the primer table PRIMERS
    add("primer_longer", _pair(rng, "primer_longer", 30, "10M", 30, "50M"), 10)                 # (the loser's head primer masks 24 columns, the clip 10)
    add("primer_shorter", _pair(rng, "primer_shorter", 30, "40M", 30, "50M"), 40)
    add("winner_tail_masked", _pair(rng, "winner_tail_masked", 380, "50M", 400, "50M"), 30)
    # ---- with the floor FLOOR: the winner's tokens on the shared columns are below it, the columns get nothing from the pair
    add("winner_low_qual", [_rec(rng, "winner_low_qual", FIRST, 250, "40M", 270, qual=[30] * 20 + [2] * 20),
                            _rec(rng, "winner_low_qual", LAST, 270, "40M", 250, qual=[40] * 40)], 20)
    order = sorted(range(len(out)), key=lambda i: out[i]["pos"])      # (stable: records of equal pos keep the order they were made in)
    return [out[i] for i in order], expect


def arrays(specs):
    return rs.arrays(specs)


def fuzz_specs(seed, n_pairs=520, n_single=120, ref_len=2000, tid=0, ref=None, n_edge=6):
    """A paired fuzz: pairs on random CIGARs of fuzz_reads (every op) whose second mate starts inside the first, and among them every
    class of record the rule leaves alone — planted at fixed rates, so every seed holds them —, n_single records without a mate, and
    n_edge pairs (six, whatever n_pairs is, unless the caller says otherwise) whose loser carries an insertion on the last column of
    its clip (_last_clipped_column: made behind all the others, so the first n_pairs pairs and the singles do not depend on n_edge)."""
    rng = np.random.default_rng(seed)
    ref = ref or "".join("ACGT"[int(k)] for k in rng.integers(0, 4, ref_len))
    out = []
    for k in range(n_pairs):
        c1, c2 = fz.random_cigar(rng), fz.random_cigar(rng)
        s1 = fz._span(c1)
        p1 = int(rng.integers(0, max(1, ref_len - s1 - 600)))
        p2 = p1 + int(rng.integers(0, max(1, s1 + 3)))
        f1, f2 = (FIRST, LAST) if rng.random() < 0.5 else (163, 83)
        name, m1, m2, mt, n_rec = "q%d_%s" % (k, "z" * int(rng.integers(0, 40))), p2, p1, tid, 2
        kind = k % 40                                               # (0 .. 12: a class the rule leaves alone; the others are plain pairs)
        if kind == 0:
            f1 &= ~1
        elif kind == 1:
            f1 &= ~2
        elif kind == 2:
            f2 |= 8
        elif kind == 3:
            f1 |= 0x100
        elif kind == 4:
            f2 |= 0x800
        elif kind == 5:
            f1 |= 0xC0
        elif kind == 6:
            mt = 1 - tid
        elif kind == 7:
            m1 = -1
        elif kind == 8:
            n_rec = 1
        elif kind == 9:
            n_rec = 3 + k % 2
        elif kind == 10:
            m1 = p2 + 1                                             # (next_pos off by one: two keys)
        elif kind == 11:
            f2 = f1 ^ 0x30                                          # (two firsts, or two lasts, on one key)
        elif kind == 12:
            p2 = p1
            m1 = m2 = p1 + 7                                        # (one key, but neither record lies where the other says)
        recs = [fz._read(rng, ref, p1, c1, f1, name, tid, mtid=mt, mpos=m1, tlen=0), fz._read(rng, ref, p2, c2, f2, name, tid, mtid=mt, mpos=m2, tlen=0)]
        if n_rec == 1:
            recs = recs[:1]
        for extra in range(n_rec - 2):
            c3 = fz.random_cigar(rng)
            recs.append(fz._read(rng, ref, p2 if extra % 2 == 0 else p1, c3, f2 if extra % 2 == 0 else f1, name, tid, mtid=mt, mpos=m2 if extra % 2 == 0 else m1, tlen=0))
        out += recs
    for k in range(n_single):
        c = fz.random_cigar(rng)
        out.append(fz._read(rng, ref, int(rng.integers(0, ref_len - 700)), c, int(rng.choice([0, 16, 4, 1, 0x400])), "s%d" % k, tid, mtid=-1, mpos=-1, tlen=0))
    out.sort(key=lambda r: r["pos"])
    for r in out:
        r["mapq"] = int(rng.choice((0, 19, 20, 60, 60, 60, 60, 60)))
    out += _last_clipped_column(seed, ref, ref_len, tid, n_edge)
    out.sort(key=lambda r: r["pos"])
    return out


def _last_clipped_column(seed, ref, ref_len, tid, n):
    """pairs whose loser carries an insertion right behind the LAST column it shares with the winner — the insertion's token is the
    clip's last, so it goes with it (mate_overlap_cases.cases' "ins_inside") —, from a generator of their own: the random pairs put an
    insertion there in one seed of four only, and with these every record of the fuzz above stays what it was"""
    rng = np.random.default_rng(seed + 9000)
    out = []
    for k in range(n):
        s1, shared = int(rng.integers(30, 80)), int(rng.integers(1, 20))
        p1 = int(rng.integers(0, max(1, ref_len - 700)))
        p2 = p1 + s1 - shared                                       # (the winner ends on p1 + s1 - 1: clip = shared, the edge p2 + shared)
        c2 = [(shared, "M"), (int(rng.integers(1, 5)), "I"), (int(rng.integers(10, 40)), "M")]
        f1, f2 = (FIRST, LAST) if k % 2 else (163, 83)
        out += [fz._read(rng, ref, p1, [(s1, "M")], f1, "e%d" % k, tid, mtid=tid, mpos=p2, tlen=0, mapq=60),
                fz._read(rng, ref, p2, c2, f2, "e%d" % k, tid, mtid=tid, mpos=p1, tlen=0, mapq=60)]
    return out


FUZZ_SEEDS = (11, 12)
FUZZ_L = 2000
FUZZ_REFS = [("ref", FUZZ_L), ("other", 300)]


def on_reference_0(specs, tid):
    """the records of reference `tid` as a file of that reference alone would hold them: refID 0, a mate elsewhere on reference 1"""
    return [dict(r, tid=0, mtid=(0 if r["mtid"] == tid else 1 if r["mtid"] >= 0 else -1)) for r in specs if r["tid"] == tid]
