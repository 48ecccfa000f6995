"""What the tests of the codon counts share (tests/test_codon_counts.py, tests/test_cli_codons.py): the device call between guards, the
yardstick's records of hand-made specs and of a fuzz seed, the hand-made records around one codon of a 100-column reference, the fixed
reads' counts in numpy, and the command line's planted case.  No tests in here."""
import ctypes as C
import functools

import numpy as np

from tests import codon_yardstick as cy
from tests import device_file as dvf
from tests import fixed_reads as fx
from tests import fuzz_masked as fm
from tests import link_cases as lkc
from tests import links_yardstick as ly
from tests import primer_yardstick as py
from tests import read_specs as rsp
from trueconsense_amd import _ffi, engine

LDS = engine.CODONS_LDS
G = 64                                                                          # guard words on either side of the records
W = 346                                                                         # int32 words of a record
HL = 100                                                                        # the hand-made records' reference
C0 = 40                                                                         # ... and the codon they are made around


def device_codons(ctx, rs, c0s):
    """tcmi_readset_codon_counts into a host buffer between guards -> the records (CODON_DTYPE); pos, reserved and j[0][0][0] are checked
    here, and Context.codon_counts must give the same bytes (run after run)"""
    c0s = np.ascontiguousarray(c0s, np.int64)
    n = len(c0s)
    buf = dvf.sentinel(2 * G + W * n, np.int32, salt=13).copy()
    before = buf.copy()
    rc = _ffi.lib().tcmi_readset_codon_counts(ctx.handle, rs.handle, n, _ffi.ptr(c0s), C.c_void_p(buf.ctypes.data + 4 * G))
    _ffi.check(rc, ctx.handle)
    assert np.array_equal(buf[:G], before[:G]) and np.array_equal(buf[-G:], before[-G:]), "a guard around the records was written"
    got = buf[G:-G].view(engine.CODON_DTYPE).copy()
    assert np.array_equal(got["pos"], c0s) and not got["reserved"].any() and not got["j"][:, 0, 0, 0].any()
    assert (got["j"] >= 0).all() and (got["ins_inside"] >= 0).all() and (got["ins_inside"] <= got["j"].sum((1, 2, 3))).all()
    again = ctx.codon_counts(rs, c0s)
    assert again.tobytes() == got.tobytes(), "Context.codon_counts gave other bytes than the call before it"
    return got


def differ(got, want, label):
    """'' when the records equal the yardstick's; else the first differing codons with the differing counters of both"""
    if np.array_equal(got["j"], want["j"]) and np.array_equal(got["ins_inside"], want["ins_inside"]):
        return ""
    rows = []
    for e in range(len(got)):
        at = np.argwhere(got["j"][e] != want["j"][e])[:6].tolist()
        if at or got["ins_inside"][e] != want["ins_inside"][e]:
            rows.append("codon %d: ins_inside %d want %d; %s" % (got["pos"][e], got["ins_inside"][e], want["ins_inside"][e], ", ".join(
                "%r got %d want %d" % (tuple(t), got["j"][e][tuple(t)], want["j"][e][tuple(t)]) for t in at)))
        if len(rows) == 4:
            break
    return "%r (classes none, A, T, C, G, X, coverage only)\n%s" % (label, "\n".join(rows))


def yard(specs, n_ref, c0s, table=(), q=0, slack=0):
    """the yardstick of hand-made specs -> (the records at c0s, the count matrix, the class matrix, the I marks)"""
    rd = rsp.arrays(specs)
    whole = py.counts(rd, n_ref, table, q, slack)[0]
    cls = ly.classes(rd, n_ref, table, q, slack, n_pos=len(whole))
    ins = cy.ins_marks(rd, n_ref, table, q, slack, n_pos=len(whole))
    return cy.joint(cls, ins, c0s), whole, cls, ins


@functools.lru_cache(maxsize=None)
def marks_of(seed, mode):
    """-> (class matrix, I marks [passing records, n_pos], n_pos, the yardstick's count matrix) of a fuzz seed under a mode of fuzz_masked"""
    tabled, slack, q, f = fm.MODES[mode]
    cls, n_pos, whole = lkc.classes_of(seed, mode)
    _, rd = fm.passing(seed, None, None, f)
    return cls, cy.ins_marks(rd, fm.L, fm.table_of(seed) if tabled else (), q, slack, n_pos=n_pos), n_pos, whole


def two_frames(whole, width=150):
    """the codons at every third column of the window with the most coverage, and a second frame shifted by one: consecutive first
    columns differ by 1 and by 2"""
    s = lkc.window_columns(whole, width)[0]
    return sorted(set(range(s, s + width, 3)) | set(range(s + 1, s + width, 3)))


# ---- hand-made records around the codon at C0 ------------------------------------------------------------------------------------------------
def _rec(rng, name, pos, cigar, seq=None, qual=30, flag=0):
    cig = [(n, "MIDNSHP=X"[op]) for op, n in fm._ops({"cigar": cigar})]
    n = sum(k for k, op in cig if op in "MIS=X")
    return rsp.mk(rng, pos, cig, [qual] * (0 if seq == "*" else n), name, seq=seq, flag=flag)


def edge_specs():
    """records that begin at C0, C0 + 1, C0 + 2, that end there, one over all three columns and records over none of them"""
    rng = np.random.default_rng(40)
    out = [_rec(rng, "begins_%d" % k, C0 + k, "20M") for k in range(3)] + [_rec(rng, "ends_%d" % k, C0 + k - 19, "20M") for k in range(3)]
    out += [_rec(rng, "over", C0 - 5, "20M"), _rec(rng, "one_column", C0 + 1, "1M"), _rec(rng, "in_front", C0 - 20, "20M"), _rec(rng, "behind", C0 + 3, "20M")]
    return sorted(out, key=lambda r: r["pos"])


OVERLAP_C0 = [C0, C0 + 1, C0 + 2, C0 + 3, C0 + 13]


def overlap_specs():
    """records that start on each of the codons' first columns, in front of them and between them, of 2 to 30 columns"""
    rng = np.random.default_rng(41)
    out = []
    for k, pos in enumerate(list(range(C0 - 6, C0 + 16)) * 3):
        out.append(_rec(rng, "o%d" % k, pos, "%dM" % int(rng.integers(2, 31))))
    return sorted(out, key=lambda r: r["pos"])


def cigar_specs():
    """-> (specs, {name: ((class at C0, C0 + 1, C0 + 2), inserted bases inside?)}): every CIGAR shape over the codon"""
    rng = np.random.default_rng(42)
    A = "A" * 40
    shapes = [("del_whole", 30, "10M3D10M", (5, 5, 5), False), ("del_first_two", 30, "10M2D10M", (5, 5, 1), False),
              ("del_last_two", 30, "11M2D10M", (1, 5, 5), False), ("ins_behind_0", 30, "11M2I10M", (1, 1, 1), True),
              ("ins_behind_1", 30, "12M2I10M", (1, 1, 1), True), ("ins_behind_2", 30, "13M2I10M", (1, 1, 1), False),
              ("soft_clip", 41, "5S15M", (0, 1, 1), False), ("skip", 30, "8M6N8M", (6, 6, 6), False), ("no_seq", 35, "20M", (6, 6, 6), False),
              ("del_then_ins", 30, "10M2D2I10M", (5, 6, 1), True), ("plain", 30, "20M", (1, 1, 1), False)]
    specs, expect = [], {}
    for name, pos, cigar, cls, inside in shapes:
        qlen = sum(n for op, n in fm._ops({"cigar": cigar}) if op in (0, 1, 4, 7, 8))
        specs.append(_rec(rng, name, pos, cigar, "*" if name == "no_seq" else A[:qlen]))
        expect[name] = (cls, inside)
    return sorted(specs, key=lambda r: r["pos"]), expect


def join_specs(n=600):
    """600 records over the codon, the triplet following the record's number: at least three distinct triplets in every wavefront"""
    rng = np.random.default_rng(43)
    trip = ("AAA", "ACA", "GAT", "TTT", "AAC")
    return [_rec(rng, "j%d" % k, C0 - 4, "12M", "CCCC" + trip[k % 5] + "GGGGG") for k in range(n)]


# ---- the fixed reads of tests/fixed_reads.py ----------------------------------------------------------------------------------------------------
def fixed_codons(rd, c0s, q=0, f=(0, 0, 0)):
    """fixed_reads' 20M records -> the records (DTYPE) at c0s: no insertion anywhere, so ins_inside is 0"""
    keep, mask = fx.kept(rd, f), fx.read_mask(rd)
    n = len(rd["pos"])
    out = np.zeros(len(c0s), cy.DTYPE)
    for e, c in enumerate(c0s):
        t = np.zeros((3, n), np.int64)
        for k in range(3):
            lo, hi, cls = fx.column(rd, keep, mask, c + k, q)
            t[k, lo:hi] = cls
        j = np.bincount((t[0] * 7 + t[1]) * 7 + t[2], minlength=343)
        j[0] = 0
        out[e] = (j.reshape(7, 7, 7), 0, c, 0)
    return out


# ---- hand-written counts for the writer -------------------------------------------------------------------------------------------------------
def hand_part(shift=0):
    """-> (counts, frames, names, the [L, 7] matrix they add up to, reference): two codons of one + frame at `shift`, ATG -> ATA / TTA and
    GCA -> GCT, over a 12-column reference"""
    counts = np.zeros(2, cy.DTYPE)
    counts["pos"] = (shift, shift + 3)
    for t, v in (((1, 2, 4), 70), ((1, 2, 1), 20), ((2, 2, 1), 10), ((1, 2, 0), 5)):
        counts[0]["j"][t] = v
    for t, v in (((4, 3, 1), 60), ((4, 3, 2), 40)):
        counts[1]["j"][t] = v
    matrix = np.zeros((shift + 12, 7), np.int32)
    for r in counts:
        for k in range(3):
            s = r["j"].astype(np.int64).sum(tuple(a for a in range(3) if a != k))
            matrix[int(r["pos"]) + k, 1:6], matrix[int(r["pos"]) + k, 0] = s[1:6], s[1:].sum()
    frames = np.array([(shift, shift + 12, 1, 0)], engine.CDS_DTYPE)
    return counts, frames, ["orfA"], matrix, b"N" * shift + b"ATGGCATAAGGG"


# ---- the command line's case ------------------------------------------------------------------------------------------------------------------
CL = 300
CDS_START, CODON = 30, 96                                                        # a CDS over [30, 270); the planted codon's first column (its 23rd codon)


@functools.lru_cache(maxsize=None)
def cli_case(cis):
    """-> (reference, records): 60 reads of 100 bases over the codon GGG at CODON.  cis: a third of them carry AAG there — both changes
    on the same reads, G -> K; else a third carry AGG (R) and another third GAG (E): the same two rows in the variant table."""
    rng = np.random.default_rng(79)
    ref = list("".join("ACGT"[int(k)] for k in rng.integers(0, 4, CL)))
    ref[CODON:CODON + 3] = "GGG"
    ref[CDS_START:CDS_START + 3] = "ATG"
    ref = "".join(ref)
    specs = []
    for k in range(60):
        pos = 20 + k
        seq = list(ref[pos:pos + 100])
        if cis:
            alt = "AAG" if k % 3 == 0 else "GGG"
        else:
            alt = ("AGG", "GAG", "GGG")[k % 3]
        seq[CODON - pos:CODON - pos + 3] = alt
        specs.append({"pos": pos, "flag": 16 if k % 2 else 0, "cigar": "100M", "seq": "".join(seq), "name": "r%d" % k, "tid": 0, "qual": 30, "mapq": 60})
    return ref, specs
