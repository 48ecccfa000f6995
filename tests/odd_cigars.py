"""CIGARs no aligner writes (csrc/cigar_rule.h; DESIGN.md "CIGARs no aligner writes"): records whose CIGAR is well-formed as bytes but
not as an alignment, for tests/test_cigar_rule.py, tests/test_odd_cigars_host.py and (GPU) tests/test_odd_cigars.py.
  tolerated   nothing may be refused and every output must equal the oracle's: a seeded generator (SEEDS, about 2 000 records each on
              an axis of L columns; a record's name is "<class>|<setting>|<number>") and a hand-made list (hand_specs), with the large
              but legal query totals in a list of their own (large_specs: their token texts would take gigabytes in Python — the C
              oracle and a matrix stated by hand are their yardsticks);
  refused     LIARS: a CIGAR whose query total Yq is 2^29 or more, one of them in an otherwise good file of 40 records (refused_file)
              at each of PLACES — or in one of the three IGNORED forms, in which the file is accepted and counts what the good file
              counts.
The spec dicts are read_specs' (cigar as text: synth_small's letters, 'B' and 'a'-'f' for the reserved op codes 9-15).  No tests in here."""
import functools
import struct

import numpy as np

from tests import fuzz_masked as fm
from tests import fuzz_reads as fz
from tests import hand_bam as hb
from tests import read_specs as rs
from tests import synth_small as ss
from trueconsense_amd import synthetic as sy

L = fm.L
SEEDS = (1, 2, 3, 4)
BOUND = 1 << 29                                                                 # cigar_rule.h's TCMI_CIGAR_MAX_QUERY
MAXLEN = (1 << 28) - 1                                                          # the longest op a CIGAR word holds
LONG = fm.LONG
SETTINGS = ("plain", "edge", "long", "pair", "dup")
PER_CLASS = 40                                                                  # base records of a class in a seed; a pair adds one, a set two
REF_OPS, QUERY_OPS = (0, 2, 3, 7, 8), (0, 1, 4, 7, 8)
RESERVED = "Babcdef"


# ---- the rule, restated -------------------------------------------------------------------------------------------------------------
def sums(words):
    """CIGAR words (len << 4 | op) -> (reference span, query total Yq, malformed?) of a record that would otherwise be kept"""
    span = sum(int(w) >> 4 for w in words if int(w) & 15 in REF_OPS)
    yq = sum(int(w) >> 4 for w in words if int(w) & 15 in QUERY_OPS)
    return span, yq, int(span > 0 and yq >= BOUND)


def words_of(r):
    return [(n << 4) | op for op, n in ss.parse_cigar(r["cigar"])]


def kept(r):
    """does the record pile up when nothing filters: mapped, on the reference, with a reference span"""
    return not r["flag"] & 4 and r.get("tid", 0) >= 0 and r["pos"] >= 0 and sums(words_of(r))[0] > 0


def class_of(r):
    return r["name"].split("|")[0]


def setting_of(r):
    return r["name"].split("|")[1]


# ---- the shapes -----------------------------------------------------------------------------------------------------------------------
def _n(rng, hi=12):
    return int(rng.integers(1, hi))


def _core(rng, long=False):
    """a run of matched bases: one to three ops of M, = and X; long: with a piece of more than LONG columns (an N op now and then)"""
    ops = [(int(rng.integers(6, 25)), "MMM=X"[int(rng.integers(0, 5))]) for _ in range(int(rng.integers(1, 4)))]
    if long:
        ops.insert(int(rng.integers(0, len(ops) + 1)), (int(rng.integers(LONG + 8, LONG + 200)), "N" if rng.random() < 0.3 else "M"))
    return ops


def _zero(rng):
    return (0, "MIDNS"[int(rng.integers(0, 5))])


def _uniform(rng, long):
    ops = [(_n(rng, 30), "MIDNSHP=X"[int(rng.integers(0, 9))]) for _ in range(int(rng.integers(1, 11)))]
    if long or not any(op in "MDN=X" for _, op in ops):
        ops.insert(int(rng.integers(0, len(ops) + 1)), (int(rng.integers(LONG + 8, LONG + 200)) if long else _n(rng, 30), "M"))
    return ops


def _dn_only(rng, long):
    ops = [(_n(rng, 30), "DN"[int(rng.integers(0, 2))]) for _ in range(int(rng.integers(1, 5)))]
    if long:
        ops.append((int(rng.integers(LONG + 8, LONG + 200)), "N"))
    return ops


def _reserved(rng, long):
    r = lambda: (int(rng.integers(1, 41)), RESERVED[int(rng.integers(0, 7))])
    how = int(rng.integers(0, 4))
    mid = [[r()], [r(), (_n(rng), "I")], [(_n(rng), "I"), r()], [(_n(rng), "I"), r(), (_n(rng), "I")]][how]
    return _core(rng, long) + mid + _core(rng) + ([r()] if rng.random() < 0.3 else [])


def _with_insertion(rng, long):
    return _core(rng, long) + [(_n(rng, 9), "I")] + _core(rng) + ([(_n(rng, 9), "S")] if rng.random() < 0.5 else [])


SHAPES = {
    "lead_I": lambda g, lg: [(_n(g), "I")] + _core(g, lg), "lead_D": lambda g, lg: [(_n(g), "D")] + _core(g, lg),
    "lead_N": lambda g, lg: [(_n(g), "N")] + _core(g, lg), "lead_P": lambda g, lg: [(_n(g), "P")] + _core(g, lg),
    "trail_I": lambda g, lg: _core(g, lg) + [(_n(g), "I")], "trail_D": lambda g, lg: _core(g, lg) + [(_n(g), "D")],
    "trail_N": lambda g, lg: _core(g, lg) + [(_n(g), "N")], "trail_P": lambda g, lg: _core(g, lg) + [(_n(g), "P")],
    "mid_S": lambda g, lg: _core(g, lg) + [(_n(g), "S")] + _core(g), "mid_H": lambda g, lg: _core(g, lg) + [(_n(g), "H")] + _core(g),
    "twice": lambda g, lg: (lambda op: _core(g, lg) + [(_n(g), op), (_n(g), op)] + _core(g))("MIDNSHP=X"[int(g.integers(0, 9))]),
    "I_D": lambda g, lg: _core(g, lg) + [(_n(g), "I"), (_n(g), "D")] + _core(g),
    "D_I": lambda g, lg: _core(g, lg) + [(_n(g), "D"), (_n(g), "I")] + _core(g),
    "I_P_I": lambda g, lg: _core(g, lg) + [(_n(g), "I"), (_n(g, 4), "P"), (_n(g), "I")] + _core(g),
    "D_I_end": lambda g, lg: _core(g, lg) + [(_n(g), "D"), (_n(g), "I")],
    "DN_only": _dn_only,
    "no_span": lambda g, lg: [(_n(g, 30), "ISHP"[int(g.integers(0, 4))]) for _ in range(int(g.integers(1, 6)))],
    "uniform": _uniform,
    "zero_first": lambda g, lg: [_zero(g)] + _core(g, lg), "zero_last": lambda g, lg: _core(g, lg) + [_zero(g)],
    "zero_between_M": lambda g, lg: [(_n(g, 25), "M"), _zero(g), (int(g.integers(LONG + 8, LONG + 200)) if lg else _n(g, 25), "M")],
    "zero_before_I": lambda g, lg: _core(g, lg) + [_zero(g), (_n(g), "I")] + _core(g),
    "zero_after_I": lambda g, lg: _core(g, lg) + [(_n(g), "I"), _zero(g)] + _core(g),
    "reserved": _reserved,
    "seq_short_1": _with_insertion, "seq_short_many": _with_insertion, "seq_long_1": _with_insertion, "seq_long_many": _with_insertion,
    "seq_star": _with_insertion, "seq_odd": _with_insertion, "qual_ff": _with_insertion,
}
CLASSES = tuple(SHAPES)
NOT_KEPT = ("no_span",)                                                         # the classes defined as not kept


def _span(cig):
    return sum(n for n, op in cig if op in "MDN=X")


def _qlen(cig):
    return sum(n for n, op in cig if op in "MIS=X")


def _record(rng, ref, cls, pos, cig, flag, name, **mate):
    """the record of a class: SEQ follows the reference on matched bases, qualities lie around the floor 13; the seq_* and qual_ff
    classes then change SEQ and QUAL against the CIGAR's query total"""
    if cls == "seq_odd" and _qlen(cig) % 2 == 0:                                # an odd l_seq: the last byte's low nibble is no base
        k = max(i for i, (_, op) in enumerate(cig) if op in "M=X")
        if pos + _span(cig) < L:
            cig[k] = (cig[k][0] + 1, cig[k][1])
        else:
            cig[k] = (cig[k][0] - 1, cig[k][1])
    seq = fz._seq_for(rng, ref, pos, cig)
    bases = lambda n: "".join("ACGT"[int(k)] for k in rng.integers(0, 4, n))
    if cls == "seq_short_1":
        seq = seq[:-1]
    elif cls == "seq_short_many":
        seq = seq[:int(rng.integers(1, max(2, len(seq) - 5)))]
    elif cls == "seq_long_1":
        seq += bases(1)
    elif cls == "seq_long_many":
        seq += bases(int(rng.integers(5, 41)))
    elif cls == "seq_star":
        seq = ""
    qual = [255] * len(seq) if cls == "qual_ff" else fz._quals(rng, len(seq), floor=1)
    r = {"pos": int(pos), "flag": int(flag), "cigar": "".join("%d%s" % t for t in cig), "seq": seq or "*", "qual": qual if seq else [],
         "name": name, "tid": 0}
    r.update(mate)
    return r


def _place(rng, span, setting, table):
    """where a record of `span` columns starts: anywhere, or (edge) so that its first columns lie in a '+' primer of the table up to
    five columns in front of the mask's edge, or its last ones in a '-' primer up to five columns behind it"""
    if setting == "edge" and span > 0:
        for _ in range(20):
            s, e, rev = table[int(rng.integers(0, len(table)))]
            d = int(rng.integers(0, 6))
            pos = (s + min(d, e - 1 - s)) - span + 1 if rev else e - 1 - min(d, e - 1 - s)
            if 0 <= pos <= L - span:
                return pos
    return int(rng.integers(0, max(1, L - span + 1)))


def specs(seed):
    """-> the position-sorted records of a seed: PER_CLASS base records of every class, the k-th in setting SETTINGS[k % 5] — plain;
    at a mask edge of fuzz_masked.primers(seed); long (more than LONG columns: tally_stream_kernel's); the first of an overlapping
    mate pair whose other mate is of the same class; the first of a duplicate set of three —, strands at random, MAPQ and filterable
    FLAG bits by read_specs.randomise, one record in twenty unmapped"""
    rng = np.random.default_rng(7000 + seed)
    ref, _ = sy.make_reference(seed=3, L=L, cds=[])
    table = fm.table_of(seed)
    out = []
    for cls in CLASSES:
        for k in range(PER_CLASS):
            setting = SETTINGS[k % len(SETTINGS)]
            name = "%s|%s|%d" % (cls, setting, k)
            cig = SHAPES[cls](rng, setting == "long")
            pos = _place(rng, _span(cig), setting, table)
            flag = (16 if rng.random() < 0.5 else 0) | (4 if rng.random() < 0.05 else 0)
            if setting == "pair":
                c2 = SHAPES[cls](rng, False)
                p2 = min(pos + int(rng.integers(0, max(1, min(_span(cig), 40)))), max(0, L - _span(c2)))
                f1, f2 = (99, 147) if rng.random() < 0.5 else (163, 83)
                tlen = max(pos + _span(cig), p2 + _span(c2)) - pos
                out.append(_record(rng, ref, cls, pos, cig, f1, name, mtid=0, mpos=p2, tlen=tlen))
                out.append(_record(rng, ref, cls, p2, c2, f2, name, mtid=0, mpos=pos, tlen=-tlen))
            elif setting == "dup":
                first = _record(rng, ref, cls, pos, cig, flag, name)
                out.append(first)
                for j in (1, 2):
                    out.append(dict(first, name="%s.%d" % (name, j), qual=fz._quals(rng, len(first["qual"]), floor=1) if first["qual"] and cls != "qual_ff" else list(first["qual"])))
            else:
                out.append(_record(rng, ref, cls, pos, cig, flag, name))
    out.sort(key=lambda r: r["pos"])
    pair_flags = {id(r): r["flag"] for r in out}
    rs.randomise(rng, out)
    for r in out:                                                               # (a pair keeps its FLAG: both mates stay mapped and paired)
        if setting_of(r) == "pair":
            r["flag"] = pair_flags[id(r)]
    return out


@functools.lru_cache(maxsize=None)
def seed_case(seed):
    """-> (records, their arrays)"""
    s = specs(seed)
    return s, rs.arrays(s)


# ---- the hand-made tolerated records ----------------------------------------------------------------------------------------------------
def _hand(name, pos, cigar, seq=None, flag=0, qual=None, **kw):
    ops = ss.parse_cigar(cigar)
    qlen = sum(n for op, n in ops if op in QUERY_OPS)
    if seq is None:
        seq = ("ACGTTGCAAGCTTCGA" * (qlen // 16 + 1))[:qlen]
    q = ([12, 13, 30, 13, 12, 40, 2] * (len(seq) // 7 + 1))[:len(seq)] if qual is None else qual
    r = {"pos": pos, "flag": flag, "cigar": cigar, "seq": seq or "*", "qual": q if seq and seq != "*" else [], "name": "hand|%s|0" % name, "tid": 0, "mapq": 60}
    r.update(kw)
    return r


def hand_specs():
    """one record (two: a strand each) of every tolerated shape, stated by hand, on columns 100 - 700 of the axis"""
    texts = [("lead_I", "3I20M"), ("lead_D", "4D20M"), ("lead_N", "5N20M"), ("lead_P", "2P20M"), ("trail_I", "20M3I"), ("trail_D", "20M4D"),
             ("trail_N", "20M5N"), ("trail_P", "20M2P"), ("mid_S", "10M3S10M"), ("mid_H", "10M3H10M"), ("MM", "10M10M"), ("II", "10M2I3I10M"),
             ("DD", "10M2D3D10M"), ("I_D", "10M2I3D10M"), ("D_I", "10M3D2I10M"), ("I_P_I", "10M2I1P3I10M"), ("P_I", "10M1P2I10M"),
             ("D_I_end", "20M3D2I"), ("D_only", "12D"), ("N_only", "12N"), ("DN_only", "5D7N2D"), ("I_only", "12I"), ("S_H_P_only", "5S3H2P"),
             ("0M_first", "0M20M"), ("0I_first", "0I20M"), ("0D_first", "0D20M"), ("0N_last", "20M0N"), ("0S_last", "20M0S"),
             ("0M_between", "10M0M10M"), ("0D_between", "10M0D10M"), ("0I_between", "10M0I10M"), ("0N_before_I", "10M0N2I10M"),
             ("0D_before_I", "10M0D2I10M"), ("0M_before_I", "10M0M2I10M"), ("0S_before_I", "10M0S2I10M"), ("0I_before_I", "10M0I2I10M"),
             ("0M_after_I", "10M2I0M10M"), ("0D_after_I", "10M2I0D10M"), ("0P_I", "10M0P2I10M"), ("only_0M_and_D", "0M5D0I"),
             ("reserved_mid", "10M7B10M"), ("reserved_before_I", "10M40a2I10M"), ("reserved_after_I", "10M2I1f10M"), ("reserved_in_I", "10M2I3c2I10M"),
             ("reserved_each", "3M1B3M1a3M1b3M1c3M1d3M1e3M1f3M"), ("reserved_only", "5B5f"), ("clip_H_S", "2H3S20M3S2H"), ("S_H_lead", "3S2H20M"), ("EQ_X", "5=1X0X4=2I0=5X"), ("X_only", "12X")]
    out = []
    for k, (name, cigar) in enumerate(texts):
        for flag in (0, 16):
            out.append(_hand("%s%s" % (name, "-" if flag else "+"), 100 + 12 * k, cigar, flag=flag))
    qlen = 22
    base = "10M2I10M"
    seq = ("ACGTTGCAAGCTTCGA" * 3)
    for name, s in (("seq_short_1", seq[:qlen - 1]), ("seq_short_many", seq[:5]), ("seq_long_1", seq[:qlen + 1]), ("seq_long_many", seq[:qlen + 20]),
                    ("seq_star", ""), ("seq_ends_in_I", seq[:11])):
        out.append(_hand(name, 690 + len(s) % 7, base, seq=s))
    out.append(_hand("seq_odd", 695, "10M2I9M"))
    out.append(_hand("qual_ff", 696, base, qual=[255] * qlen))
    out.sort(key=lambda r: r["pos"])
    return out


def large_specs():
    """large but legal query totals over a small SEQ: the device carries a query index near the bound and never forms an address from
    it.  -> (records, {name: the columns it covers, every one of them an 'N' of quality 0: coverage and nothing else — and the I mark
    where one is due})"""
    def run(n, op):                                                             # (a CIGAR word holds 28 bits of length: two ops for more)
        return "%d%s%d%s" % (MAXLEN, op, n - MAXLEN, op)
    out = [_hand("S_536870000", 100, run(536870000, "S") + "12M", seq="ACGTACGTACGTACGTACGT"),
           _hand("I_to_bound_minus_1", 120, "10M" + run(BOUND - 21, "I") + "10M", seq="ACGTACGTAC", flag=99, mtid=0, mpos=125, tlen=30),
           _hand("I_to_bound_minus_1", 125, "10M" + run(BOUND - 21, "I") + "10M", seq="ACGTACGTAC", flag=147, mtid=0, mpos=120, tlen=-30),
           _hand("clip_below_2p20", 150, "%dS20M" % ((1 << 20) - 1), seq="ACGT"),
           _hand("clip_at_2p20", 175, "%dS20M" % (1 << 20), seq="ACGT"),
           _hand("clip_above_2p20", 200, "%dS20M" % ((1 << 20) + 1), seq="ACGT"),
           _hand("tail_S", 225, "20M" + run(BOUND - 21, "S"), seq="ACGTACGTACGTACGTACGT")]
    assert sums(words_of(out[1])) == (20, BOUND - 1, 0) and max(sums(words_of(r))[1] for r in out) == BOUND - 1
    return out


def large_classes(specs_, n_pos, q=0, clip=None):
    """large_specs by hand -> (cls, ins) uint8 [records, n_pos], as rules_marks.marks gives them: the class of the record's token at
    a column (0 none, 1..4 plane A, T, C, G, 6 coverage alone) and its I mark.  Every op of these records is M, I or S: a matched base
    whose query index lies in SEQ counts its plane, one beyond it is an 'N' of quality 0 (coverage alone); under a floor q > 0 a token
    counts only with a quality of at least q; the record's first clip[i] columns count nothing (its mate's, --mate-overlap); the I mark
    sits on the last column in front of an insertion, when that column's token counts"""
    cls, ins = np.zeros((len(specs_), n_pos), np.uint8), np.zeros((len(specs_), n_pos), np.uint8)
    plane = {"A": 1, "T": 2, "C": 3, "G": 4}
    for i, r in enumerate(specs_):
        x, y = r["pos"], 0
        lo = x + (int(clip[i]) if clip is not None else 0)
        ops = ss.parse_cigar(r["cigar"])
        assert all(op in (0, 1, 4) for op, _ in ops) and set(r["seq"]) <= set("ACGT")
        for k, (op, n) in enumerate(ops):
            if op == 0:
                for j in range(n):
                    qi = y + j
                    if x + j >= lo and (q == 0 or (r["qual"][qi] if qi < len(r["seq"]) else 0) >= q):
                        cls[i, x + j] = plane[r["seq"][qi]] if qi < len(r["seq"]) else 6
                if k + 1 < len(ops) and ops[k + 1][0] == 1 and cls[i, x + n - 1]:
                    ins[i, x + n - 1] = 1
                x += n
            y += n
    return cls, ins


def large_matrix(specs_, n_pos, q=0, clip=None):
    """the count matrix of large_specs from large_classes: int32 [n_pos, 7] (coverage, A, T, C, G, X, I)"""
    cls, ins = large_classes(specs_, n_pos, q, clip)
    m = np.zeros((n_pos, 7), np.int32)
    m[:, 0] = (cls > 0).sum(0)
    for k in (1, 2, 3, 4):
        m[:, k] = (cls == k).sum(0)
    m[:, 6] = ins.sum(0)
    return m


# ---- the refused records ----------------------------------------------------------------------------------------------------------------
GOOD_L = 400
SEQ20 = "ACGTACGTACGTACGTACGT"
F = fm.F                                                                        # the read filter of the "filtered" form: (20, 0, 0x800)
_M = MAXLEN
LIARS = {
    "yq_2p29": [(10, "M"), (_M, "I"), (BOUND - 20 - _M, "I"), (10, "M")],       # the partner of the tolerated 2^29 - 1
    "S_x9": [(_M, "S")] * 9 + [(20, "M")],                                      # the first signed wrap of a 32-bit query index
    "S_x17": [(_M, "S")] * 17 + [(20, "M")],                                    # ... wraps to a small index that looks valid
    "I_x9": [(10, "M")] + [(_M, "I")] * 9 + [(10, "M")],
    "I_x17": [(10, "M")] + [(_M, "I")] * 17 + [(10, "M")],
    "tail_S_x9": [(20, "M")] + [(_M, "S")] * 9,
    "tail_S_x17": [(20, "M")] + [(_M, "S")] * 17,
    "I_x4096": [(10, "M")] + [(_M, "I")] * 4096 + [(10, "M")],                  # a 16 KiB record with a sum near 2^40: it straddles blocks
}
PLACES = ("first", "middle", "last", "block_first")
IGNORED = ("unmapped", "filtered", "no_reference")
PER_BLOCK = 8


def good_records():
    """40 records, position-sorted on one reference of GOOD_L columns: -> [(pos, bytes)]"""
    out = []
    for k in range(40):
        cig = [(20, "M")] if k % 4 else [(8, "M"), (2, "I"), (6, "M"), (3, "D"), (4, "M")]
        out.append((5 + 9 * k, hb.rec(0, 5 + 9 * k, "good%d" % k, 16 if k % 3 == 0 else 0, cig, SEQ20, [30 + k % 10] * 20)))
    return out


def liar_record(kind, pos, form=None):
    flag, tid, mapq = 0, 0, 37
    if form == "unmapped":
        flag = 4
    elif form == "filtered":
        flag = F[2]
    elif form == "no_reference":
        tid, pos = -1, -1
    return hb.rec(tid, pos, "liar_" + kind, flag, LIARS[kind], SEQ20, [30] * 20, mapq=mapq)


def _write(path, records, block_cut=4096):
    """records: [bytes] in file order, PER_BLOCK of them a BGZF block (one larger than block_cut is cut into several)"""
    text = b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c\tLN:%d\n" % GOOD_L
    head = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 1) + struct.pack("<i", 2) + b"c\0" + struct.pack("<i", GOOD_L)
    with open(path, "wb") as fh:
        fh.write(hb.bgzf(head))
        for o in range(0, len(records), PER_BLOCK):
            blob = b"".join(records[o:o + PER_BLOCK])
            for a in range(0, len(blob), block_cut):
                fh.write(hb.bgzf(blob[a:a + block_cut]))
        fh.write(hb.EOF_BLOCK)


def good_file(path):
    _write(path, [b for _, b in good_records()])


def refused_file(path, kind, place, form=None):
    """the good file with one liar in it -> the liar's record index.  place: the file's first record, a middle one, the last one, the
    first of a BGZF block (record 16 of blocks of PER_BLOCK).  form: None, or one of IGNORED — the liar then is a record that is
    ignored anyway (a record without a reference goes last, as a sorted file has it)"""
    good = good_records()
    at = {"first": 0, "middle": 21, "last": len(good), "block_first": 2 * PER_BLOCK}[place]
    if form == "no_reference":
        at = len(good)
    pos = good[min(at, len(good) - 1)][0]
    recs = [b for _, b in good]
    recs.insert(at, liar_record(kind, pos, form))
    assert place != "block_first" or at % PER_BLOCK == 0
    _write(path, recs)
    return at
