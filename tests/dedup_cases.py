"""Hand-made records for the duplicate rule (--dedup) on mate_overlap_cases' 600-column reference, as record specs with the verdict each
was made for ("dup": a duplicate without a read filter; "dup_f": under FILTER, where that differs), the same key on two references for
a contig layout, and fuzz specs: mate_overlap_cases' paired fuzz with duplicate sets planted among it.  CLASSES names what the hand-made
list holds; dedup_yardstick.classes finds them in any set of records.  No tests in here."""
import functools

import numpy as np

from tests import fuzz_reads as fz
from tests import mate_overlap_cases as mc

L = mc.L
REFS = mc.REFS
FIRST, LAST = mc.FIRST, mc.LAST
FILTER = mc.FILTER
FLOOR = mc.FLOOR
FUZZ_SEEDS = (31, 32)
FUZZ_L = mc.FUZZ_L
FUZZ_REFS = mc.FUZZ_REFS
# what the hand-made list holds (dedup_yardstick.classes); "filtered_best" shows under FILTER only, "two_references" in two_refs() only
CLASSES = ("fragment_set_of_three", "tie", "fwd_rev_same_pos", "same_u5_different_clips", "hard_clip_in_set", "reverse_pos_differ", "pair_set",
           "pair_one_end_differs", "pair_and_fragment_same_end", "secondary_at_duplicate", "qual_ff", "threshold", "ambiguous_fragments",
           "dup_pair_overlaps", "negative_u5")


def _frag(rng, name, flag, pos, cigar, q, dup, mapq=60, dup_f=None):
    n = sum(k for k, op in mc._cig(cigar) if op in "MIS=X")
    r = mc._rec(rng, name, flag, pos, cigar, -1, mtid=-1, mapq=mapq, qual=[q] * n if isinstance(q, int) else q)
    r.update(dup=dup, dup_f=dup if dup_f is None else dup_f)
    return r


def _pair(rng, name, p1, c1, p2, c2, q, dup, flags=(FIRST, LAST)):
    n1, n2 = (sum(k for k, op in mc._cig(c) if op in "MIS=X") for c in (c1, c2))
    a = mc._rec(rng, name, flags[0], p1, c1, p2, qual=[q] * n1)
    b = mc._rec(rng, name, flags[1], p2, c2, p1, qual=[q] * n2)
    for r in (a, b):
        r.update(dup=dup, dup_f=dup)
    return [a, b]


@functools.lru_cache(maxsize=None)
def cases():
    """-> specs in file order (sorted by pos, records of equal pos in the order they were made)"""
    rng = np.random.default_rng(78)
    out = []
    # a fragment set of three with distinct scores: the middle one wins
    out += [_frag(rng, "three_a", 0, 20, "30M", 30, True), _frag(rng, "three_b", 0, 20, "30M", 40, False), _frag(rng, "three_c", 0, 20, "30M", 20, True)]
    # a secondary and a supplementary record at that place: never examined
    out += [_frag(rng, "three_sec", 0x100, 20, "30M", 41, False), _frag(rng, "three_sup", 0x800, 20, "30M", 41, False)]
    # a tie: the lowest record index wins
    out += [_frag(rng, "tie_a", 0, 60, "30M", 30, False), _frag(rng, "tie_b", 0, 60, "30M", 30, True), _frag(rng, "tie_c", 0, 60, "30M", 29, True)]
    # forward and reverse at one pos: two ends
    out += [_frag(rng, "fr_fwd", 0, 100, "30M", 30, False), _frag(rng, "fr_rev", 16, 100, "30M", 20, False)]
    # the same u5 through different soft clips and a hard clip
    out += [_frag(rng, "clip_none", 0, 140, "30M", 30, True), _frag(rng, "clip_soft", 0, 145, "5S25M", 35, False),
            _frag(rng, "clip_hard", 0, 145, "3H2S25M4S", 20, True)]
    # reverse reads whose pos differ but whose unclipped ends agree (229)
    out += [_frag(rng, "rev_a", 16, 200, "20M10S", 30, True), _frag(rng, "rev_b", 16, 204, "4S26M", 31, False), _frag(rng, "rev_c", 16, 200, "30M2H", 31, False)]
    # pairs, FR: two of one key; a third whose reverse mate ends one column further; a fragment at the pairs' forward end
    out += _pair(rng, "pair_a", 250, "40M", 300, "40M", 30, False) + _pair(rng, "pair_b", 250, "40M", 300, "40M", 25, True, flags=(163, 83))
    out += _pair(rng, "pair_c", 250, "40M", 300, "41M", 20, False)
    out += [_frag(rng, "pair_frag", 0, 250, "40M", 10, False)]
    # a record that fails FILTER with the best score: no candidate under it
    out += [_frag(rng, "flt_kept", 0, 330, "30M", 30, True, dup_f=False), _frag(rng, "flt_best", 0, 330, "30M", 41, False, mapq=5)]
    # QUAL all 0xFF scores 0, whatever its place in the file
    out += [_frag(rng, "ff_none", 0, 370, "30M", 255, True), _frag(rng, "ff_low", 0, 370, "30M", 16, False)]
    # the threshold: 14 adds nothing, 15 does
    out += [_frag(rng, "q14", 0, 410, "30M", 14, True), _frag(rng, "q15", 0, 410, "30M", [15] + [14] * 29, False)]
    # an ambiguous name group: its members are fragments, and two of them share an end
    amb = [mc._rec(rng, "amb", FIRST, 450, "30M", 470, qual=[30] * 30), mc._rec(rng, "amb", LAST, 470, "30M", 450, qual=[30] * 30),
           mc._rec(rng, "amb", LAST, 470, "30M", 450, qual=[20] * 30)]
    for r, d in zip(amb, (False, False, True)):
        r.update(dup=d, dup_f=d)
    out += amb
    # a duplicate pair whose mates also overlap
    out += _pair(rng, "ovl_a", 500, "40M", 520, "40M", 30, False) + _pair(rng, "ovl_b", 500, "40M", 520, "40M", 22, True)
    # u5 < 0
    out += [_frag(rng, "neg_a", 0, 0, "3S30M", 30, False), _frag(rng, "neg_b", 0, 2, "5S28M", 25, True)]
    order = sorted(range(len(out)), key=lambda i: out[i]["pos"])
    return [out[i] for i in order]


def two_refs():
    """the same key on two references (a contig layout): a set of two on each, and neither set sees the other"""
    rng = np.random.default_rng(79)
    out = []
    for tid in (0, 1):
        for k, (q, dup) in enumerate(((20, True), (30, False))):
            r = _frag(rng, "t%d_%d" % (tid, k), 0, 50, "30M", q, dup)
            r["tid"] = tid
            out.append(r)
    return out


SHARED_AT, SHARED_CIGAR, SHARED_INS = 100, "10M2I10M3D10M", "GT"
SHARED_ELSEWHERE, SHARED_PAIRS = 200, (300, 320)


@functools.lru_cache(maxsize=None)
def shared_indel():
    """a duplicate set that shares its insertion and its deletion: five forward fragments at SHARED_AT with SHARED_CIGAR and one SEQ,
    their quality sums distinct, the best the third in the file; one fragment at SHARED_ELSEWHERE with the same inserted bases; two
    proper pairs of equal ends at SHARED_PAIRS whose second mates carry 5M1I20M (the same base) inside the overlap -> specs in file order"""
    rng = np.random.default_rng(80)
    out = []
    for k, q in enumerate((20, 25, 40, 30, 35)):
        out.append(_frag(rng, "set_%d" % k, 0, SHARED_AT, SHARED_CIGAR, q, q != 40))
    seq = out[0]["seq"][:10] + SHARED_INS + out[0]["seq"][12:]
    for r in out:
        r["seq"] = seq
    far = _frag(rng, "elsewhere", 0, SHARED_ELSEWHERE, "10M2I10M", 30, False)
    far["seq"] = far["seq"][:10] + SHARED_INS + far["seq"][12:]
    out.append(far)
    p1, p2 = SHARED_PAIRS
    pairs = _pair(rng, "eq_a", p1, "40M", p2, "5M1I20M", 30, False) + _pair(rng, "eq_b", p1, "40M", p2, "5M1I20M", 22, True)
    for r in pairs:
        if "I" in r["cigar"]:
            r["seq"] = r["seq"][:5] + "C" + r["seq"][6:]
    out += pairs
    order = sorted(range(len(out)), key=lambda i: out[i]["pos"])
    return [out[i] for i in order]


def arrays(specs):
    return mc.arrays(specs)


def _plant(rng, ref, ref_len, tid, n_sets):
    """duplicate sets among the fuzz: every class of CLASSES at a fixed rate, so every seed holds them"""
    out = []

    def rec(name, flag, pos, cig, q=None, mpos=-1, mtid=-1, mapq=60):
        r = fz._read(rng, ref, pos, cig, flag, name, tid, floor=1, mtid=mtid, mpos=mpos, tlen=0)
        if q is not None:
            r["qual"] = [q] * len(r["qual"]) if isinstance(q, int) else list(q)
        r["mapq"] = mapq
        return r

    for k in range(n_sets):
        kind = k % 12
        ln = int(rng.integers(20, 90))
        u = int(rng.integers(10, ref_len - 700))
        tag = "d%d_%d_" % (tid, k)
        if kind in (0, 1):                                      # forward fragments, clips of every sort, distinct scores (mostly)
            for m in range(int(rng.integers(2, 6))):
                c = int(rng.integers(0, 8))
                cig = ([(c, "H" if m % 3 == 2 else "S")] if c else []) + [(ln - c, "M")] + ([(2, "S")] if m % 2 else [])
                out.append(rec(tag + str(m), 0, u + c, cig))
        elif kind == 2:                                         # reverse fragments whose pos differ: all end at u + ln - 1 unclipped
            out += [rec(tag + "0", 16, u, [(ln, "M")]), rec(tag + "1", 16, u, [(ln - 3, "M"), (3, "S")]),
                    rec(tag + "2", 16, u + 4, [(4, "S"), (ln - 4, "M")]), rec(tag + "3", 16, u + 2, [(ln - 7, "M"), (5, "H")])]
        elif kind == 3:                                         # a tie, and a third below it
            q = [int(x) for x in rng.integers(2, 42, ln)]
            out += [rec(tag + "0", 0, u, [(ln, "M")], q), rec(tag + "1", 0, u, [(ln, "M")], q), rec(tag + "2", 0, u, [(ln, "M")], 3)]
        elif kind == 4:                                         # forward and reverse at one pos, a secondary record and a filtered best at a set
            out += [rec(tag + "0", 0, u, [(ln, "M")]), rec(tag + "1", 16, u, [(ln, "M")]), rec(tag + "2", 0, u, [(ln, "M")]),
                    rec(tag + "sec", 0x100, u, [(ln, "M")], 41), rec(tag + "best", 0, u, [(ln, "M")], 41, mapq=5)]
        elif kind == 5:                                         # QUAL 0xFF and the threshold
            out += [rec(tag + "0", 0, u, [(ln, "M")], 255), rec(tag + "1", 0, u, [(ln, "M")], 14), rec(tag + "2", 0, u, [(ln, "M")], [15] + [14] * (ln - 1))]
        elif kind in (6, 7, 8):                                 # pair sets, FR and RF flags; the mates overlap in some; one with another far end
            d = int(rng.integers(0, ln)) if kind == 6 else ln + int(rng.integers(0, 200))
            for m in range(int(rng.integers(2, 5))):
                c = int(rng.integers(0, 5)) if m else 0
                f1, f2 = (FIRST, LAST) if (k + m) % 2 else (163, 83)
                c1 = ([(c, "S")] if c else []) + [(ln - c, "M")]
                out += [rec(tag + str(m), f1, u + c, c1, mpos=u + d, mtid=tid), rec(tag + str(m), f2, u + d, [(ln, "M")], mpos=u + c, mtid=tid)]
            if kind == 8:
                out += [rec(tag + "far", FIRST, u, [(ln, "M")], mpos=u + d, mtid=tid), rec(tag + "far", LAST, u + d, [(ln + 1, "M")], mpos=u, mtid=tid)]
        elif kind == 9:                                         # a pair and fragments at its forward end
            d = ln + 5
            out += [rec(tag + "p", FIRST, u, [(ln, "M")], mpos=u + d, mtid=tid), rec(tag + "p", LAST, u + d, [(ln, "M")], mpos=u, mtid=tid),
                    rec(tag + "f0", 0, u, [(ln, "M")]), rec(tag + "f1", 0, u, [(ln - 3, "M"), (3, "S")])]
        elif kind == 10:                                        # an ambiguous name group whose members share ends with each other
            out += [rec(tag + "g", FIRST, u, [(ln, "M")], mpos=u + 9, mtid=tid), rec(tag + "g", LAST, u + 9, [(ln, "M")], mpos=u, mtid=tid),
                    rec(tag + "g", LAST, u + 9, [(ln, "M")], mpos=u, mtid=tid), rec(tag + "g", FIRST, u, [(ln, "M")], mpos=u + 9, mtid=tid)]
        else:                                                   # u5 < 0
            out += [rec(tag + "0", 0, 0, [(7, "S"), (ln, "M")]), rec(tag + "1", 0, 3, [(10, "S"), (ln - 3, "M")]), rec(tag + "2", 16, 0, [(ln, "M")])]
    return out


def fuzz_specs(seed, n_pairs=300, n_single=80, n_sets=96, ref_len=FUZZ_L, tid=0, ref=None):
    """mate_overlap_cases.fuzz_specs (every CIGAR op, every class of record the join leaves alone) + planted duplicate sets, in pos order"""
    rng = np.random.default_rng(seed + 5000)
    ref = ref or "".join("ACGT"[int(k)] for k in rng.integers(0, 4, ref_len))
    out = mc.fuzz_specs(seed, n_pairs=n_pairs, n_single=n_single, ref_len=ref_len, tid=tid, ref=ref) + _plant(rng, ref, ref_len, tid, n_sets)
    out.sort(key=lambda r: r["pos"])
    return out


def permuted(specs, seed):
    """the same records in another file order (the tie-break follows the file): shuffled, then sorted by pos again — records of equal
    pos, the members of most sets among them, come in another order; the file stays one the packers' chunk capacities are made for"""
    rng = np.random.default_rng(seed)
    out = [specs[int(i)] for i in rng.permutation(len(specs))]
    out.sort(key=lambda r: r["pos"])
    return out
