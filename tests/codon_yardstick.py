"""The yardstick of --codon-table (tcmi_readset_codon_counts, tcmi_codon_aa, tcmi_codon_select, tcmi_codons_text), from committed
yardsticks only: the class of a record's token at a column is tests/links_yardstick.classes' — no second statement of the token rule —,
the I mark is read off the same single-record matrix's I plane, the joint counts are accumulated here; frames, selection, translation
and text are the rules of include/tcmi.h in Python's integers.  The genetic code is spelled as the 64-letter string in TCAG order."""
import numpy as np

from tests import primer_yardstick as py
from tests import strand_yardstick as sy

DTYPE = np.dtype([("j", np.int32, (7, 7, 7)), ("ins_inside", np.int32), ("pos", np.int32), ("reserved", np.int32)])
CDS = np.dtype([("start", np.int32), ("end", np.int32), ("strand", np.int32), ("phase", np.int32)])
HEADER = "REGION\tFEATURE\tSTRAND\tCODON\tPOS\tREF_CODON\tREF_AA\tALT_CODON\tALT_AA\tEFFECT\tSUBS\tCOUNT\tSPAN\tFREQ\tPARTIAL\tOTHER\tINS_INSIDE\n"
CODE = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"      # TTT TTC TTA TTG TCT ... GGG
LETTER = "NATCG-"                                                            # by plane: none, A, T, C, G, X
COMPLEMENT = {"A": "T", "T": "A", "C": "G", "G": "C", "N": "N", "-": "-"}


def aa(codon):
    """three letters in coding order -> the amino acid, '*' a stop, 'X' when a letter is none of A, C, G, T"""
    if any(b not in "TCAG" for b in codon) or len(codon) != 3:
        return "X"
    return CODE[16 * "TCAG".index(codon[0]) + 4 * "TCAG".index(codon[1]) + "TCAG".index(codon[2])]


def aa_of_planes(b0, b1, b2):
    return aa("".join(LETTER[b] if 1 <= b <= 4 else "?" for b in (b0, b1, b2)))


def frame_codons(f):
    """(start, end, strand, phase) -> [c0] of the frame's codons in coding direction (index + 1 is the codon's number)"""
    start, end, strand, phase = (int(x) for x in f)
    if strand > 0:
        return list(range(start + phase, end - 2, 3))
    return [hi - 2 for hi in range(end - 1 - phase, start + 1, -3)]


def select(recs, frames):
    """[(pos, allele, ...)], [(start, end, strand, phase)] -> the distinct c0, ascending, of the codons that hold a record of planes 1..5"""
    out = set()
    for f in frames:
        for c in frame_codons(f):
            if any(c <= p <= c + 2 and 1 <= a <= 5 for p, a, *_ in recs):
                out.add(c)
    return sorted(out)


def ins_marks(rd, L, table=(), q=0, slack=0, shift=0, n_pos=None):
    """-> uint8 [records, n_pos]: 1 where the record's token carries the I mark, from the matrix primer_yardstick.counts gives for that
    record alone (as links_yardstick.classes reads the classes)"""
    n = int(rd["n_reads"])
    if n_pos is None:
        n_pos = len(py.counts(rd, L, table, q, slack, shift)[0])
    out = np.zeros((n, n_pos), np.uint8)
    keep = np.zeros(n, bool)
    for i in range(n):
        keep[:] = False
        keep[i] = True
        m = py.counts(sy.subset(rd, keep), L, table, q, slack, shift)[0][:n_pos]
        out[i, :len(m)] = m[:, 6]
    return out


def joint(cls, ins, c0s):
    """class matrix and I marks [records, n_pos] (beyond n_pos: 0), the codons' first columns -> records (DTYPE)"""
    out = np.zeros(len(c0s), DTYPE)
    n_rec, n_pos = cls.shape
    none = np.zeros(n_rec, np.int64)
    for e, c in enumerate(c0s):
        t = [cls[:, c + k].astype(np.int64) if 0 <= c + k < n_pos else none for k in range(3)]
        mark = [ins[:, c + k].astype(bool) if 0 <= c + k < n_pos else none.astype(bool) for k in range(2)]
        key = (t[0] * 7 + t[1]) * 7 + t[2]
        j = np.bincount(key, minlength=343)
        j[0] = 0
        out[e] = (j.reshape(7, 7, 7), int(((key != 0) & (mark[0] | mark[1])).sum()), c, 0)
    return out


def invariant(recs, matrix):
    """'' when every codon's counts add up to the [extent, 7] count matrix at its three columns in classes 1..6, j[0][0][0] and reserved
    are 0, else the first that does not"""
    matrix = np.asarray(matrix, np.int64)
    for r in np.asarray(recs):
        j = r["j"].astype(np.int64)
        if j[0, 0, 0] or r["reserved"]:
            return "codon %d: j[0][0][0] = %d, reserved = %d" % (r["pos"], j[0, 0, 0], r["reserved"])
        for k in range(3):
            col = int(r["pos"]) + k
            m = matrix[col] if col < len(matrix) else np.zeros(7, np.int64)
            want = m[1:6].tolist() + [int(m[0] - m[1:6].sum())]
            got = j.sum(tuple(a for a in range(3) if a != k))[1:].tolist()
            if got != want:
                return "codon %d: classes 1..6 at slot %d sum to %r, the matrix says %r" % (r["pos"], k, got, want)
    return ""


def complete(t):
    return all(1 <= x <= 4 for x in t) or all(x == 5 for x in t)


def text(counts, frames, names, region, ref, num, den, min_alt_depth, min_depth, pos_offset=0):
    """counts: records (DTYPE) ascending; frames: [(start, end, strand, phase)]; ref: bytes on the axis -> the rows of --codon-table"""
    ref = bytes(ref).decode("latin-1").upper()
    rows = []
    numbered = [{c: k + 1 for k, c in enumerate(frame_codons(f))} for f in frames]
    for r in counts:
        c0 = int(r["pos"])
        j = [[[int(v) for v in row] for row in pl] for pl in r["j"]]
        cells = [((x, y, z), j[x][y][z]) for x in range(7) for y in range(7) for z in range(7)]
        total = sum(v for _, v in cells)
        span = sum(v for t, v in cells if all(t))
        done = sum(v for t, v in cells if complete(t))
        refl = "".join(ref[c0 + k] if c0 + k < len(ref) and ref[c0 + k] in "ACGT" else "N" for k in range(3))
        for f, name, num_of in zip(frames, names, numbered):
            if c0 not in num_of:
                continue
            minus = int(f[2]) < 0
            orient = (lambda s: "".join(COMPLEMENT[b] for b in reversed(s))) if minus else (lambda s: s)
            ref_codon = orient(refl)
            ref_aa = aa(ref_codon)
            shown = []
            for t, v in cells:
                alt = "".join(LETTER[x] for x in t) if complete(t) else None
                if alt is None or alt == refl:
                    continue
                if v >= min_alt_depth and v * den >= num * span and span >= min_depth:
                    shown.append((-v, (t[0] * 7 + t[1]) * 7 + t[2], alt, v))
            for _, _, alt, v in sorted(shown):
                alt_codon = orient(alt)
                if alt == "---":
                    alt_aa, effect, subs = "-", "DEL", 0
                else:
                    alt_aa = aa(alt_codon)
                    subs = sum(a != b for a, b in zip(alt, refl))
                    effect = "UNKNOWN" if ref_aa == "X" else "SYN" if alt_aa == ref_aa else "STOP_GAINED" if alt_aa == "*" else \
                        "STOP_LOST" if ref_aa == "*" else "MIS"
                rows.append("\t".join([region, name, "-" if minus else "+", str(num_of[c0]), str(c0 - pos_offset + 1), ref_codon, ref_aa, alt_codon,
                                       alt_aa, effect, str(subs), str(v), str(span), "%.6f" % (v / span), str(total - span), str(span - done),
                                       str(int(r["ins_inside"]))]) + "\n")
    return "".join(rows)
