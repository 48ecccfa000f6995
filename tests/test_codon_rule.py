"""--codon-table without a GPU: the frames, the genetic code, the selection and the row writer (csrc/codon_rule.h, csrc/codons_text.cpp) as
a program of their own (tests/codons_main.cpp), built plain and under AddressSanitizer + UBSan, against Python's integers
(tests/codon_yardstick.py), and the same functions through the ABI.  The kernel's tests are tests/test_codon_counts.py, the command
line's tests/test_cli_codons.py."""
import struct
from collections import Counter

import numpy as np
import pytest

from tests import codon_yardstick as cy
from tests import host_program
from trueconsense_amd import _ffi, engine
from trueconsense_amd.cli_tables import codon_frames

BUILDS = ("plain", "sanitized")


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("codons_main")
    src = ["tests/codons_main.cpp", "trueconsense_amd/csrc/codons_text.cpp"]
    return {"plain": host_program.build(src, d / "codons_main", sanitize=False), "sanitized": host_program.build(src, d / "codons_main_san")}


def _run(prog, mode, tmp_path, blob):
    inp, out = str(tmp_path / "c.in"), str(tmp_path / "c.out")
    with open(inp, "wb") as fh:
        fh.write(blob)
    r = host_program.run(prog, mode, inp, out)
    assert r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-4000:])
    with open(out, "rb") as fh:
        return fh.read()


# ---- the genetic code ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", BUILDS)
def test_genetic_code(programs, tmp_path, build):
    cases = [(a, b, c) for a in range(-1, 8) for b in range(-1, 8) for c in range(-1, 8)]
    got = _run(programs[build], "aa", tmp_path, struct.pack("<q", len(cases)) + np.array(cases, np.int32).tobytes()).decode()
    assert list(got) == [cy.aa_of_planes(*c) for c in cases]
    real = {c: g for c, g in zip(cases, got) if all(1 <= x <= 4 for x in c)}
    assert len(real) == 64 and all(g == "X" for c, g in zip(cases, got) if c not in real)
    hist = Counter(real.values())
    assert hist["*"] == 3 and hist["M"] == 1 and hist["W"] == 1 and hist["L"] == hist["S"] == hist["R"] == 6 and len(hist) == 21
    assert sorted(hist.values()) == sorted([1] * 2 + [2] * 9 + [3] * 2 + [4] * 5 + [6] * 3)
    A, T, C, G = 1, 2, 3, 4                                 # the planes' order, not the alphabet's
    assert real[(A, T, G)] == "M" and real[(T, G, G)] == "W" and {c for c, g in real.items() if g == "*"} == {(T, A, A), (T, A, G), (T, G, A)}
    assert [engine.codon_aa(*c) for c in cases[::7]] == list(got[::7])


# ---- frames and selection --------------------------------------------------------------------------------------------------------------
FRAMES = [(10, 40, 1, 0), (10, 40, 1, 1), (10, 40, 1, 2), (10, 40, -1, 0), (10, 40, -1, 1), (10, 40, -1, 2),
          (50, 51, 1, 0), (52, 54, 1, 0), (55, 58, 1, 0), (59, 63, 1, 0), (59, 63, -1, 0), (55, 58, -1, 1),
          (70, 77, 1, 0), (80, 88, 1, 2)]                   # the last two: one CDS in two rows, the codon (76, 80, 81) straddles them


def test_frames_of_the_yardstick():
    assert cy.frame_codons((10, 40, 1, 0))[:2] == [10, 13] and cy.frame_codons((10, 40, 1, 1))[-1] == 35 and cy.frame_codons((10, 40, 1, 2))[0] == 12
    assert cy.frame_codons((10, 40, -1, 0))[:2] == [37, 34] and cy.frame_codons((10, 40, -1, 1))[-1] == 12 and cy.frame_codons((10, 40, -1, 2))[0] == 35
    assert [len(cy.frame_codons(f)) for f in FRAMES[6:12]] == [0, 0, 1, 1, 1, 0]       # a frame of 1, 2, 3 and 4 columns
    assert cy.frame_codons((59, 63, 1, 0)) == [59] and cy.frame_codons((59, 63, -1, 0)) == [60]
    assert cy.frame_codons((70, 77, 1, 0)) == [70, 73] and cy.frame_codons((80, 88, 1, 2)) == [82, 85]


@pytest.mark.parametrize("build", BUILDS)
def test_select(programs, tmp_path, build):
    lib = _ffi.lib()
    for frames in [[f] for f in FRAMES] + [FRAMES, FRAMES[12:], []]:
        for recs in ([(p, 1 + p % 5, 3, 9) for p in range(0, 95)], [(p, 6, 3, 9) for p in range(0, 95)], [(76, 2, 3, 9), (80, 2, 3, 9), (81, 5, 1, 9)],
                     [(12, 6, 3, 9), (12, 3, 3, 9), (60, 6, 1, 9)], []):
            blob = struct.pack("<qq", len(recs), len(frames)) + np.array(recs, np.int32).reshape(-1, 4).tobytes() + \
                np.array(frames, np.int32).reshape(-1, 4).tobytes()
            got = _run(programs[build], "select", tmp_path, blob).decode().split()
            want = cy.select(recs, frames)
            assert got == ["0", str(len(want))] + [str(c) for c in want], (frames, recs[:3])
            if all(a == 6 for _, a, *_ in recs):
                assert want == []                           # '+' rows do not select
            assert engine.codon_select(np.array([tuple(r) for r in recs], engine.VARIANT_DTYPE), np.array([tuple(f) for f in frames], engine.CDS_DTYPE)).tolist() == want
    assert cy.select([(76, 2, 3, 9), (80, 2, 3, 9), (81, 5, 1, 9)], FRAMES[12:]) == []      # the straddling codon is no codon
    assert cy.select([(p, 1, 3, 9) for p in range(100)], FRAMES[12:]) == [70, 73, 82, 85]
    n = _ffi.C.c_int64(7)
    for bad in ((0, 5, 0, 0), (0, 5, 2, 0), (0, 5, 1, 3), (0, 5, 1, -1), (-1, 5, 1, 0), (5, 4, 1, 0)):
        cds = np.array([bad], engine.CDS_DTYPE)
        assert lib.tcmi_codon_select(None, 0, engine.ptr(cds), 1, None, 0, _ffi.C.byref(n)) == _ffi.E_ARG and n.value == 0, bad


def test_frames_of_gff_rows():
    def row(**kw):
        return dict(dict(seqid="c1", source="s", type="CDS", start=11, end=40, score=".", strand="+", phase="0", attributes=""), **kw)
    rows = [row(Name="N1", ID="i1", gene="g1"), row(phase=".", ID="i2", gene="g2"), row(phase="2", strand="-", gene="g3"), row(strand="-", phase="1"),
            row(type="gene"), row(strand="."), row(strand="?"), row(phase="3"), row(seqid="c2", start=1, end=9, Name=float("nan"), ID="i9")]
    cds, names = codon_frames(rows)
    assert cds.tolist() == [(10, 40, 1, 0), (10, 40, 1, 0), (10, 40, -1, 2), (10, 40, -1, 1), (0, 9, 1, 0)]
    assert names == ["N1", "i2", "g3", "CDS_11_40", "i9"]
    cds, names = codon_frames(rows, (["c0", "c2", "c1"], [0, 512, -1]))         # c1 is dropped by the layout, c2 sits at 512
    assert cds.tolist() == [(512, 521, 1, 0)] and names == ["i9"]
    cds, names = codon_frames([row(type="gene")])
    assert len(cds) == 0 and cds.dtype == engine.CDS_DTYPE and names == []


# ---- the text --------------------------------------------------------------------------------------------------------------------------
#       0         1         2         3
#       0123456789012345678901234567890123456789
REF = b"ATGGCATAAGGNTGGCGAtttACCGGGAAACCCTTTGGG"
L = 36                                                      # the matrix ends inside the last codon: columns 36.. have depth 0
F_PLUS, F_MINUS, F_SHIFT = (0, 39, 1, 0), (0, 39, -1, 0), (1, 38, 1, 0)
A, T, C, G, X, O = 1, 2, 3, 4, 5, 6


def rec(c0, cells, ins=0):
    r = np.zeros((), cy.DTYPE)
    for t, v in cells.items():
        r["j"][t] = v
    r["ins_inside"], r["pos"] = ins, c0
    return r


def matrix_of(counts, n_pos):
    """the [n_pos, 7] count matrix the (non-overlapping) codons' counts add up to"""
    m = np.zeros((n_pos, 7), np.int32)
    for r in counts:
        for k in range(3):
            col = int(r["pos"]) + k
            if col < n_pos:
                s = r["j"].astype(np.int64).sum(tuple(a for a in range(3) if a != k))
                m[col, 1:6], m[col, 0] = s[1:6], s[1:].sum()
    return m


COUNTS = [
    rec(0, {(A, T, G): 60, (A, T, A): 20, (T, T, G): 20, (C, T, G): 6, (A, T, X): 4, (A, T, 0): 7, (0, 0, G): 2, (A, O, G): 1}, ins=3),   # M: MIS twice at equal counts
    rec(3, {(G, C, A): 50, (G, C, T): 30, (X, X, X): 15, (G, A, T): 5}),          # A: SYN, DEL, MIS with SUBS 2
    rec(6, {(T, A, A): 10, (T, A, T): 9, (C, A, A): 8, (T, G, A): 7}),            # *: STOP_LOST twice, SYN (TGA)
    rec(9, {(G, G, A): 12, (G, G, G): 5, (X, X, X): 2}),                          # GGN: UNKNOWN, DEL
    rec(12, {(T, G, G): 30, (T, G, A): 11, (T, A, G): 10, (T, A, A): 9}),         # W: STOP_GAINED with SUBS 1, 1, 2
    rec(18, {(T, T, T): 40, (C, T, T): 40}),                                      # lower-case reference
    rec(33, {(T, T, T): 20, (T, T, C): 20}),
    rec(34, {(T, T, 0): 22, (T, C, 0): 18}),                # its third column is column 36 = L: nobody has a token there
]
NAMES = ["plus", "minus gene", "shifted"]


def _text_blob(counts, frames, names, matrix, n_cols, ld, num, den, mad, md, region, off, ref):
    planes = np.zeros((7, ld), np.int32)
    planes[:, :len(matrix)] = np.asarray(matrix, np.int32).T
    nm = b"".join(x.encode() + b"\0" for x in names)
    return struct.pack("<12q", len(counts), len(frames), n_cols, ld, num, den, mad, md, off, len(region), len(ref), len(nm)) + region.encode() + bytes(ref) + nm + \
        np.array(counts, cy.DTYPE).tobytes() + np.array(frames, np.int32).reshape(-1, 4).tobytes() + planes.tobytes()


def _text(prog, tmp_path, counts, frames, names, matrix, num=3, den=100, mad=1, md=10, region="chr", off=0, ref=REF, n_cols=None, ld=None):
    n_cols = len(matrix) if n_cols is None else n_cols
    got = _run(prog, "text", tmp_path, _text_blob(counts, frames, names, matrix, n_cols, n_cols + 5 if ld is None else ld, num, den, mad, md, region, off, ref))
    head, _, body = got.partition(b"\n")
    rc, ln = (int(x) for x in head.split())
    assert ln == len(body)
    return rc, body.decode()


@pytest.mark.parametrize("build", BUILDS)
def test_text_against_the_yardstick(programs, tmp_path, build):
    frames = [F_PLUS, F_MINUS, F_SHIFT]
    matrix = matrix_of(COUNTS[:-1], L)
    assert cy.invariant(np.array(COUNTS[:-1], cy.DTYPE), matrix) == ""
    m34 = matrix_of(COUNTS[:6] + COUNTS[7:], L)
    for counts, mat in ((COUNTS[:-1], matrix), (COUNTS[:6] + COUNTS[7:], m34)):
        rc, got = _text(programs[build], tmp_path, counts, frames, NAMES, mat)
        want = cy.text(np.array(counts, cy.DTYPE), frames, NAMES, "chr", REF, 3, 100, 1, 10)
        assert rc == 0 and got == want and got
        assert engine.codons_text(np.array(counts, cy.DTYPE), np.array(frames, engine.CDS_DTYPE), NAMES, mat, "chr", REF, 0, "3/100", 1, 10) == want
    rc, got = _text(programs[build], tmp_path, COUNTS[:-1], frames, NAMES, matrix)
    rows = [ln.split("\t") for ln in got.splitlines()]
    assert (cy.HEADER.rstrip("\n").split("\t").index("SUBS"), len(cy.HEADER.split("\t"))) == (10, 17) and all(len(r) == 17 for r in rows)
    assert {r[9] for r in rows} == {"SYN", "MIS", "STOP_GAINED", "STOP_LOST", "DEL", "UNKNOWN"}
    by = {(r[1], int(r[4]), r[7]): r for r in rows}
    # codon 1 of "plus": ATG -> ATA and TTG tie at 20 records, ATA with the lower class code (1, 2, 1) first; then CTG with 6
    first = [r for r in rows if r[1] == "plus" and r[4] == "1"]
    assert [r[7] for r in first] == ["ATA", "TTG", "CTG"] and [r[8] for r in first] == ["I", "L", "L"]
    assert first[0][2:7] == ["+", "1", "1", "ATG", "M"] and first[0][9:] == ["MIS", "1", "20", "111", "%.6f" % (20 / 111), "9", "5", "3"]
    # the same columns on the - strand: codon 13 of 13, CAT -> TAT / CAA / CAG, the rows in the order of the axis' class codes
    last = [r for r in rows if r[1] == "minus gene" and r[4] == "1"]
    assert [r[7] for r in last] == ["TAT", "CAA", "CAG"] and last[0][2:7] == ["-", "13", "1", "CAT", "H"] and [r[8] for r in last] == ["Y", "Q", "Q"]
    assert by[("plus", 4, "GAT")][8:11] == ["D", "MIS", "2"] and by[("plus", 4, "---")][8:11] == ["-", "DEL", "0"] and by[("plus", 4, "GCT")][9] == "SYN"
    assert by[("plus", 7, "TAT")][9] == "STOP_LOST" and by[("plus", 7, "TGA")][9] == "SYN" and by[("plus", 7, "CAA")][8] == "Q"
    assert by[("plus", 10, "GGA")][5:11] == ["GGN", "X", "GGA", "G", "UNKNOWN", "1"] and by[("plus", 10, "---")][9] == "DEL"
    assert by[("minus gene", 10, "TCC")][5:10] == ["NCC", "X", "TCC", "S", "UNKNOWN"]
    assert by[("plus", 13, "TAA")][9:11] == ["STOP_GAINED", "2"] and by[("plus", 13, "TGA")][10] == "1"
    assert by[("plus", 19, "CTT")][5:10] == ["TTT", "F", "CTT", "L", "MIS"]                 # the reference's lower case is upper case
    assert by[("minus gene", 34, "GAA")][5:10] == ["AAA", "K", "GAA", "E", "MIS"] and ("shifted", 34, "TTC") not in by
    # rows: POS ascending, then the frames in the order given, then COUNT descending
    key = [(int(r[4]), NAMES.index(r[1]), -int(r[11])) for r in rows]
    assert key == sorted(key) and {r[1] for r in rows} == {"plus", "minus gene"}
    # the codon of "shifted" whose third column is column 36 >= L
    rc, got = _text(programs[build], tmp_path, COUNTS[:6] + COUNTS[7:], frames, NAMES, m34)
    rows = [ln.split("\t") for ln in got.splitlines() if ln.split("\t")[1] == "shifted"]
    assert rc == 0 and rows == []                           # no record has three classes there: SPAN 0, nothing complete
    # an offset, a longer region, a reference that ends inside a codon (N beyond it)
    rc, got = _text(programs[build], tmp_path, COUNTS[1:3], frames, NAMES, matrix, region="contig two", off=3, ref=REF[:8])
    assert rc == 0 and got == cy.text(np.array(COUNTS[1:3], cy.DTYPE), frames, NAMES, "contig two", REF[:8], 3, 100, 1, 10, 3)
    assert "\tTAN\tX\t" in got and got.startswith("contig two\tplus\t+\t2\t1\tGCA\tA\t")
    # no frame, no codon: no rows
    assert _text(programs[build], tmp_path, COUNTS[:-1], [], [], matrix) == (0, "") and _text(programs[build], tmp_path, [], frames, NAMES, matrix) == (0, "")


@pytest.mark.parametrize("build", BUILDS)
def test_thresholds_at_equality(programs, tmp_path, build):
    counts = [rec(0, {(A, T, G): 97, (A, T, A): 3, (A, T, 0): 50})]         # COUNT 3 of SPAN 100
    matrix = matrix_of(counts, L)
    for num, den, mad, md, shown in ((3, 100, 1, 10, True), (31, 1000, 1, 10, False), (3, 100, 3, 10, True), (3, 100, 4, 10, False),
                                     (3, 100, 1, 100, True), (3, 100, 1, 101, False), (0, 1, 1, 0, True), (1, 1, 1, 0, False)):
        rc, got = _text(programs[build], tmp_path, counts, [F_PLUS], ["f"], matrix, num, den, mad, md)
        assert rc == 0 and got == cy.text(np.array(counts, cy.DTYPE), [F_PLUS], ["f"], "chr", REF, num, den, mad, md)
        assert (got != "") == shown and got.count("\n") == int(shown), (num, den, mad, md)
    for bad in ((3, 0, 1, 10), (3, 1000001, 1, 10), (11, 10, 1, 10), (-1, 10, 1, 10), (3, 100, 0, 10), (3, 100, 1, -1)):
        assert _text(programs[build], tmp_path, counts, [F_PLUS], ["f"], matrix, *bad) == (_ffi.E_ARG, "")


@pytest.mark.parametrize("build", BUILDS)
def test_broken_invariant_writes_nothing(programs, tmp_path, build):
    frames = [F_PLUS]
    good = COUNTS[:3]
    matrix = matrix_of(good, L)
    assert _text(programs[build], tmp_path, good, frames, ["f"], matrix)[0] == 0
    for cell in ((T, 0, 0), (0, C, 0), (0, 0, G), (A, T, G), (O, O, O)):    # one record more at slot 0, 1, 2 alone, and at all three
        counts = [r.copy() for r in good]
        counts[1]["j"][cell] += 1
        assert cy.invariant(np.array(counts, cy.DTYPE), matrix) != ""
        assert _text(programs[build], tmp_path, counts, frames, ["f"], matrix) == (_ffi.E_ARG, "")         # (the program checks *len = 0)
    for k in range(3):                                      # ... and the matrix one off at each slot's column, on coverage alone
        m = matrix.copy()
        m[3 + k, 0] += 1
        assert _text(programs[build], tmp_path, good, frames, ["f"], m) == (_ffi.E_ARG, "")
    counts = [r.copy() for r in good]
    counts[0]["j"][0, 0, 0] = 1
    assert _text(programs[build], tmp_path, counts, frames, ["f"], matrix) == (_ffi.E_ARG, "")
    assert _text(programs[build], tmp_path, good[::-1], frames, ["f"], matrix) == (_ffi.E_ARG, "")         # not ascending
    # a codon whose third column is >= L adds up iff nobody has a token there
    tail = [rec(34, {(T, T, 0): 22, (T, C, 0): 18})]
    assert _text(programs[build], tmp_path, tail, frames, ["f"], matrix_of(tail, L))[0] == 0
    tail[0]["j"][T, T, A] = 1
    assert _text(programs[build], tmp_path, tail, frames, ["f"], matrix_of(tail, L))[0] == _ffi.E_ARG
    with pytest.raises(_ffi.TcmiError):
        engine.codons_text(np.array(tail, cy.DTYPE), np.array(frames, engine.CDS_DTYPE), ["f"], matrix_of(tail, L), "chr", REF)
