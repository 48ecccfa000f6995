"""--variant-links without a GPU: the phase rule (csrc/links_rule.h) and the row writer (csrc/variants_links_text.cpp) as a program of
their own (tests/links_main.cpp), built plain and under AddressSanitizer + UBSan, against Python's integers
(tests/links_yardstick.py); the same writer through the ABI; the yardstick's marginals against the yardstick of the count matrix; and
the command line's argument handling.  The kernel's tests are tests/test_link_counts.py."""
import os
import struct
from fractions import Fraction

import numpy as np
import pytest

from tests import fuzz_masked as ff
from tests import host_program
from tests import links_yardstick as ly
from tests import variant_yardstick as vy
from tests.cli_run import base_args as _base
from tests.cli_run import stub_files
from trueconsense_amd import TrueConsense as cli
from trueconsense_amd import _ffi, engine

TOP = (1 << 31) - 1


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("links_main")
    src = ["tests/links_main.cpp", "trueconsense_amd/csrc/variants_links_text.cpp"]
    return {"plain": host_program.build(src, d / "links_main", sanitize=False), "sanitized": host_program.build(src, d / "links_main_san")}


def _run(prog, mode, inp, out):
    r = host_program.run(prog, mode, inp, out)
    assert r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-4000:])


# ---- the rule -----------------------------------------------------------------------------------------------------------------------
def sweep():
    """-> [(both, only_a, only_b, span, min_depth, num, den)]: a dense small sweep (ties on both inequalities arise by themselves),
    planted ties, num = den, m = 0, span below, at and above the depth, and counts at 2^31 - 1 with den = 10^6"""
    cases = []
    ratios = ((9, 10), (1, 1), (2, 3), (500001, 1000000), (999999, 1000000), (3, 4))
    for num, den in ratios:
        for both in range(0, 13):
            for oa in range(0, 13, 1 if (num, den) == (9, 10) else 3):
                for ob in (0, 1, 4, 12):
                    for span in (9, 10, 11, 40):
                        cases.append((both, oa, ob, span, 10, num, den))
    for k in (1, 7, 1000, 214748):                          # both / m = 9/10 and 1/10 exactly, one record below and above each
        for d in (-1, 0, 1):
            cases.append((9 * k + d, k - d, 5 * k, 100 * k, 10, 9, 10))
            cases.append((k + d, 9 * k - d, 20 * k, 100 * k, 10, 9, 10))
            cases.append((3 * k + d, k - d, k - d, 100 * k, 10, 3, 4))
            cases.append((k + d, 3 * k - d, 3 * k - d, 100 * k, 10, 3, 4))
    for num, den in ((9, 10), (500001, 1000000), (999999, 1000000), (1000000, 1000000), (900000, 1000000)):
        for both, oa, ob in ((TOP, 0, 0), (TOP, TOP, TOP), (0, TOP, TOP), (TOP // 10, TOP - TOP // 10, TOP), (TOP - TOP // 10, TOP // 10, 0), (0, 0, TOP), (0, 0, 0),
                             (TOP - 1, 1, 1), (1, TOP - 1, TOP - 1), (TOP // 2, TOP // 2, TOP // 2), (TOP // 2 + 1, TOP // 2, TOP // 2)):
            cases.append((both, oa, ob, TOP, 10, num, den))
            cases.append((both, oa, ob, TOP, TOP, num, den))
            cases.append((both, oa, ob, TOP - 1, TOP, num, den))       # one record below the depth: LOW
    rng = np.random.default_rng(5)
    for _ in range(2000):
        num, den = ratios[int(rng.integers(0, len(ratios)))]
        both, oa, ob = (int(x) for x in rng.integers(0, 1 << 29, 3))
        cases.append((both, oa, ob, both + oa + ob + int(rng.integers(0, 1 << 29)), int(rng.integers(1, 1 << 20)), num, den))
    return cases


@pytest.mark.parametrize("build", ("plain", "sanitized"))
def test_phase_program_against_python_integers(programs, tmp_path, build):
    cases = sweep()
    want = [ly.phase(*c) for c in cases]
    m = [min(c[0] + c[1], c[0] + c[2]) for c in cases]
    # what the sweep holds
    cis_ties = [i for i, c in enumerate(cases) if want[i] != 4 and m[i] and c[0] * c[6] == c[5] * m[i]]
    trans_ties = [i for i, c in enumerate(cases) if want[i] != 4 and m[i] and c[0] * c[6] == (c[6] - c[5]) * m[i]]
    assert len(cis_ties) >= 50 and all(want[i] == 0 for i in cis_ties)                      # an exact tie is in, on both sides
    assert len(trans_ties) >= 50 and all(want[i] == 1 for i in trans_ties)
    same = [i for i, c in enumerate(cases) if c[5] == c[6]]
    assert {want[i] for i in same} >= {0, 1, 2, 3, 4}                                       # num = den: CIS only with no record off, TRANS only at both = 0
    assert all((want[i] == 0) == (cases[i][0] == m[i]) and (want[i] == 1) == (cases[i][0] == 0) for i in same if want[i] in (0, 1, 2))
    assert any(w == 3 for w in want) and all((w == 3) == (mm == 0) for w, mm in zip(want, m) if w != 4)
    assert {(c[3] > c[4]) - (c[3] < c[4]) for c in cases} == {-1, 0, 1}
    assert any(c[0] == TOP and c[6] == 1000000 for c in cases) and {0, 1, 2, 3, 4} == set(want)
    inp, out = str(tmp_path / "v.in"), str(tmp_path / "v.out")
    with open(inp, "wb") as fh:
        fh.write(struct.pack("<q", len(cases)) + np.array(cases, np.int64).tobytes())
    _run(programs[build], "phase", inp, out)
    got = np.fromfile(out, np.int32).tolist()
    bad = [(cases[i], got[i], want[i]) for i in range(len(cases)) if got[i] != want[i]]
    assert not bad, bad[:8]
    pick = cis_ties[:5] + trans_ties[:5] + same[:5]
    assert [engine.link_phase(*cases[i][:5], Fraction(cases[i][5], cases[i][6])) for i in pick] == [want[i] for i in pick]


def test_phase_argument_errors():
    lib = _ffi.lib()
    for bad in ((1, 1, 1, 5, 0, 9, 10), (1, 1, 1, 5, 1, 9, 0), (1, 1, 1, 5, 1, 999999, 1000001), (1, 1, 1, 5, 1, 11, 10), (1, 1, 1, 5, 1, 5, 10), (1, 1, 1, 5, 1, 1, 3),
                (1, 1, 1, 5, 1, -9, -10), (-1, 1, 1, 5, 1, 9, 10), (1, -1, 1, 5, 1, 9, 10), (1, 1, -1, 5, 1, 9, 10), (1, 1, 1, -5, 1, 9, 10)):
        assert lib.tcmi_link_phase(*bad) == _ffi.E_ARG, bad
    assert lib.tcmi_link_phase(1, 0, 0, 5, 1, 1000000, 1000000) == 0 and lib.tcmi_link_phase(1, 0, 0, 5, 1, 500001, 1000000) == 0


# ---- the text -----------------------------------------------------------------------------------------------------------------------
REF = b"AAcNGTTGARtA"
RECS = [(0, 2, 5, 20), (2, 4, 10, 40), (2, 5, 4, 40), (7, 1, 30, 100), (7, 6, 30, 100), (10, 5, 3, 12)]
# (first column, second column) -> {(class at the first, class at the second): records}.  The classes at a column add up to RECS:
# column 0: A 15, T 5; column 2: C 26, G 10, X 4; column 7: A 30, G 65, coverage only 5; column 10: T 9, X 3
PAIRS = {(0, 2): {(2, 4): 5, (1, 3): 10, (1, 5): 2, (1, 0): 3, (0, 4): 5, (0, 5): 2, (0, 3): 16},
         (0, 7): {(1, 0): 15, (2, 0): 5, (0, 1): 30, (0, 4): 65, (0, 6): 5},
         (0, 10): {(1, 0): 15, (2, 0): 5, (0, 2): 9, (0, 5): 3},
         (2, 7): {(4, 1): 6, (4, 4): 4, (5, 1): 1, (5, 4): 1, (5, 0): 2, (3, 1): 3, (3, 4): 20, (3, 6): 1, (3, 0): 2, (0, 1): 20, (0, 4): 40, (0, 6): 4},
         (2, 10): {(3, 2): 6, (3, 0): 20, (4, 0): 10, (5, 0): 4, (0, 2): 3, (0, 5): 3},
         (7, 10): {(1, 5): 3, (1, 2): 1, (1, 0): 26, (4, 2): 8, (4, 0): 57, (6, 0): 5}}
ROWS = {(0, 2, 4): "ctg\t1\tA\tT\t3\tC\tG\t17\t5\t0\t0\t12\tCIS\n",            # every T read carries the G
        (0, 2, 5): "ctg\t1\tA\tT\t3\tC\t*\t17\t0\t5\t2\t10\tTRANS\n",          # no read carries T and the deletion
        (0, 7, 1): "ctg\t1\tA\tT\t8\tG\tA\t0\t0\t0\t0\t0\tLOW\n",              # no record spans both
        (2, 7, 41): "ctg\t3\tC\tG\t8\tG\tA\t36\t6\t4\t4\t22\tMIXED\n",
        (2, 10, 45): "ctg\t3\tC\tG\t11\tT\t*\t6\t0\t0\t0\t6\tNONE\n",          # six records span, neither allele among them
        (2, 7, 51): "ctg\t3\tC\t*\t8\tG\tA\t36\t1\t1\t9\t25\tMIXED\n",
        (2, 10, 55): "ctg\t3\tC\t*\t11\tT\t*\t6\t0\t0\t0\t6\tNONE\n",
        (7, 10, 15): "ctg\t8\tG\tA\t11\tT\t*\t12\t3\t1\t0\t8\tCIS\n",
        (0, 10, 25): "ctg\t1\tA\tT\t11\tT\t*\t0\t0\t0\t0\t0\tLOW\n"}
WANT2 = "".join(ROWS[k] for k in ((0, 2, 4), (0, 2, 5), (0, 7, 1), (2, 7, 41), (2, 10, 45), (2, 7, 51), (2, 10, 55), (7, 10, 15)))
WANT1 = "".join(ROWS[k] for k in ((0, 2, 4), (0, 2, 5), (2, 7, 41), (2, 7, 51), (7, 10, 15)))
WANT7 = "".join(ROWS[k] for k in ((0, 2, 4), (0, 2, 5), (0, 7, 1), (0, 10, 25), (2, 7, 41), (2, 10, 45), (2, 7, 51), (2, 10, 55), (7, 10, 15)))


def matrix_of(entries):
    j = np.zeros((7, 7), np.int32)
    for (x, y), v in entries.items():
        j[x][y] = v
    return j


def links_dict(pairs=PAIRS):
    return {k: matrix_of(v) for k, v in pairs.items()}


def link_array(k, cols=(0, 2, 7, 10), pairs=PAIRS):
    """the link records of `cols` with k neighbours: the pairs' counts, b = -1 and zeros where there is no such column"""
    cols = list(cols)
    j = np.zeros((len(cols) * k, 7, 7), np.int32)
    for i, a in enumerate(cols):
        for d in range(1, k + 1):
            if i + d < len(cols):
                j[i * k + d - 1] = matrix_of(pairs[(a, cols[i + d])])
    return ly.records(cols, k, j)


def run_text(prog, tmp_path, tag, recs, links, k, rule, region, ref, pos_offset=0, n_cols=None):
    inp, out = str(tmp_path / (tag + ".in")), str(tmp_path / (tag + ".out"))
    links = np.ascontiguousarray(links, ly.DTYPE)
    n_cols = len(links) // k if n_cols is None else n_cols
    assert n_cols * k == len(links)
    with open(inp, "wb") as fh:
        fh.write(struct.pack("<9q", len(recs), n_cols, k, *rule, pos_offset, len(region.encode()), len(ref)))
        fh.write(region.encode() + ref + vy.as_array(recs).tobytes() + links.tobytes())
    _run(prog, "text", inp, out)
    raw = open(out, "rb").read()
    head, _, body = raw.partition(b"\n")
    rc, ln = (int(x) for x in head.split())
    assert len(body) == ln
    return rc, body.decode("latin-1")


def test_yardstick_text_on_the_hand_written_rows():
    for k, want in ((1, WANT1), (2, WANT2), (7, WANT7)):
        assert ly.text(RECS, links_dict(), k, "ctg", REF, 5, 9, 10) == want
    assert {ln.split("\t")[-1] for ln in WANT7.splitlines()} == set(ly.PHASES)
    assert not any(ln.split("\t")[3] == "+" or ln.split("\t")[6] == "+" for ln in WANT7.splitlines())         # '+' rows are not linked
    arr = link_array(2)
    assert arr["a"].tolist() == [0, 0, 2, 2, 7, 7, 10, 10] and arr["b"].tolist() == [2, 7, 7, 10, 10, -1, -1, -1] and not arr["j"][5:].any()


@pytest.mark.parametrize("build", ("plain", "sanitized"))
def test_text_program(programs, tmp_path, build):
    """the rows at K = 1, 2 and 7, an offset, two regions, counts at 2^31 - 1, the refusals; the program itself checks the sizing call, a
    buffer one byte short and a buffer with room to spare"""
    prog = programs[build]
    for k, want in ((1, WANT1), (2, WANT2), (7, WANT7)):
        rc, text = run_text(prog, tmp_path, "hand%d" % k, RECS, link_array(k), k, (5, 9, 10), "ctg", REF)
        assert rc == 0 and text == want, k
    spelled = {tuple(ln.split("\t")[:4]) for ln in engine.variants_text(vy.as_array(RECS), "ctg", REF).splitlines()}
    for ln in WANT7.splitlines():                                                            # the alleles as tcmi_variants_text spells them
        f = ln.split("\t")
        assert tuple(f[:4]) in spelled and (f[0],) + tuple(f[4:7]) in spelled
    assert run_text(prog, tmp_path, "none", [], link_array(2, ()), 2, (5, 9, 10), "ctg", REF) == (0, "")
    rc, text = run_text(prog, tmp_path, "one", RECS[:1], link_array(2, (0,)), 2, (5, 9, 10), "ctg", REF)
    assert (rc, text) == (0, "")
    # other thresholds: depth 13 makes the 12-record pair LOW
    rc, text = run_text(prog, tmp_path, "thr", RECS, link_array(2), 2, (13, 1, 1), "ctg", REF)
    assert rc == 0 and text == ly.text(RECS, links_dict(), 2, "ctg", REF, 13, 1, 1) and text.endswith("\t12\t3\t1\t0\t8\tLOW\n") and text != WANT2
    rc, text = run_text(prog, tmp_path, "thr1", RECS, link_array(2), 2, (5, 3, 5), "ctg", REF)
    assert rc == 0 and "\t36\t6\t4\t4\t22\tCIS\n" in text and text.startswith(ROWS[(0, 2, 4)])      # 6 of 10 at ratio 3/5: the tie is CIS
    # two regions cut out of one call over both regions' columns: a region's last pairs name columns beyond it and give no row
    whole = link_array(2)
    first, second = whole[:4], whole[4:]
    assert first["b"].tolist() == [2, 7, 7, 10] and second["b"].tolist() == [10, -1, -1, -1]
    rc, text = run_text(prog, tmp_path, "reg1", RECS[:3], first, 2, (5, 9, 10), "ctg", REF)
    assert rc == 0 and text == ROWS[(0, 2, 4)] + ROWS[(0, 2, 5)]
    rc, text = run_text(prog, tmp_path, "reg2", RECS[3:], second, 2, (5, 9, 10), "seg 2", REF, 6)
    assert rc == 0 and text == "seg 2\t2\tG\tA\t5\tT\t*\t12\t3\t1\t0\t8\tCIS\n" == ly.text(RECS[3:], links_dict(), 2, "seg 2", REF, 5, 9, 10, 6)
    # counts at 2^31 - 1
    recs = [(0, 2, TOP - 10, TOP), (1, 3, 10, TOP), (1, 4, TOP - 10, TOP)]
    pairs = {(0, 1): {(2, 4): TOP - 10, (1, 3): 10}}
    rc, text = run_text(prog, tmp_path, "top", recs, link_array(1, (0, 1), pairs), 1, (TOP, 999999, 1000000), "r", b"AA")
    assert rc == 0 and text == ly.text(recs, links_dict(pairs), 1, "r", b"AA", TOP, 999999, 1000000)
    assert [ln.split("\t")[-1] for ln in text.splitlines()] == ["TRANS", "CIS"] and str(TOP) in text
    # the refusals: TCMI_E_ARG and no text
    def changed(k=2, **kw):
        arr = link_array(k)
        for name, (idx, value) in kw.items():
            arr[name][idx] = value
        return arr
    moved_a, moved_b, tail_b, tail_ok = changed(a=(2, 3)), changed(b=(1, 8)), changed(b=(5, 10)), changed(b=(5, 11))
    tail_ok["j"][5] = matrix_of({(1, 0): 30, (4, 0): 65, (6, 0): 5})                        # (such a pair has counts: they add up at column 7)
    assert run_text(prog, tmp_path, "tail_ok", RECS, tail_ok, 2, (5, 9, 10), "ctg", REF) == (0, WANT2)                # (a column beyond the last: the next region's)
    row = link_array(2)
    row["j"][0][2][4] += 1                                                                  # T at column 0: 6 records, the table says 5
    cov = link_array(2)
    cov["j"][3][3][0] -= 1                                                                  # coverage at column 2 in pair (2, 10): 39 of 40
    col = link_array(2)
    col["j"][2][0][1] += 1                                                                  # A at column 7 in pair (2, 7): 31 of 30
    plus = link_array(2)
    plus["j"][4][6][0] += 1                                                                 # coverage at column 7 in pair (7, 10): 101; only the '+' row's cov differs too
    neg = link_array(2)
    neg["j"][0][1][0] -= 16
    neg["j"][0][1][3] += 16                                                                 # (one count is negative)
    assert neg["j"][0][1][0] < 0
    for tag, links, k, rule, n_cols in (("a", moved_a, 2, (5, 9, 10), None), ("b", moved_b, 2, (5, 9, 10), None), ("tail", tail_b, 2, (5, 9, 10), None),
                                        ("row", row, 2, (5, 9, 10), None), ("cov", cov, 2, (5, 9, 10), None), ("col", col, 2, (5, 9, 10), None),
                                        ("plus", plus, 2, (5, 9, 10), None), ("neg", neg, 2, (5, 9, 10), None),
                                        ("short", link_array(2)[:-2], 2, (5, 9, 10), None), ("extra", link_array(2, (0, 2, 7, 10, 11), {**PAIRS, (2, 11): {}, (7, 11): {}, (10, 11): {}}), 2, (5, 9, 10), None),
                                        ("k", link_array(1), 2, (5, 9, 10), None), ("k0", link_array(1)[:0], 0, (5, 9, 10), 4), ("k8", link_array(8, pairs={**PAIRS}), 8, (5, 9, 10), None),
                                        ("depth", link_array(2), 2, (0, 9, 10), None), ("den", link_array(2), 2, (5, 999999, 1000001), None),
                                        ("num", link_array(2), 2, (5, 11, 10), None), ("half", link_array(2), 2, (5, 1, 2), None)):
        assert run_text(prog, tmp_path, tag, RECS, links, k, rule, "ctg", REF, n_cols=n_cols) == (_ffi.E_ARG, ""), tag
    unsorted = [RECS[1], RECS[0]] + RECS[2:]
    assert run_text(prog, tmp_path, "order", unsorted, link_array(2), 2, (5, 9, 10), "ctg", REF) == (_ffi.E_ARG, "")


def test_text_writer_through_the_abi():
    assert engine.variants_links_text(vy.as_array(RECS), link_array(2), 2, "ctg", REF, min_depth=5) == WANT2
    assert engine.variants_links_text(vy.as_array(RECS), link_array(7), 7, "ctg", REF, 0, 5, "0.9") == WANT7
    assert engine.variants_links_text(vy.as_array([]), link_array(2, ()), 2, "ctg", REF) == ""
    assert engine.VARIANTS_LINKS_HEADER == ly.HEADER and engine.VARIANTS_LINKS_HEADER.count("\t") == WANT2.splitlines()[0].count("\t") == 12
    assert engine.LINK_DTYPE.itemsize == 208 and engine.LINK_DTYPE == ly.DTYPE and engine.LINKS_LDS == 80 and engine.LINK_PHASES == ly.PHASES
    assert _ffi.K_LINK_COUNTS == 14
    bad = link_array(2)
    bad["j"][0][2][4] += 1
    for links, k in ((bad, 2), (link_array(2)[2:], 2), (link_array(2), 1), (link_array(2)[:-1], 2)):
        with pytest.raises(_ffi.TcmiError) as e:
            engine.variants_links_text(vy.as_array(RECS), links, k, "ctg", REF, min_depth=5)
        assert e.value.code == _ffi.E_ARG
    assert [engine.link_phase(*c) for c in ((9, 1, 1, 20), (1, 9, 9, 20), (5, 5, 5, 20), (0, 0, 0, 20), (9, 1, 1, 9))] == [0, 1, 2, 3, 4]
    assert engine.link_phase(9, 1, 1, 9, min_depth=9) == 0 and engine.link_phase(3, 1, 1, 20, ratio="3/4") == 0 and engine.link_phase(3, 1, 1, 20) == 2
    for kw in (dict(min_depth=0), dict(ratio="1/2"), dict(ratio="0.4")):
        with pytest.raises(_ffi.TcmiError):
            engine.link_phase(1, 1, 1, 5, **kw)


# ---- the yardstick itself -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ff.SEEDS)
def test_the_marginals_are_the_yardstick_of_the_count_matrix(seed):
    """under floor 13 and the seed's primer table: for every pair of links_yardstick.joint the classes at its first and at its second
    column add up to primer_yardstick.counts of all records — the invariant of include/tcmi.h —, on every column and three beyond"""
    _, rd = ff.passing(seed)
    table = ff.table_of(seed)
    whole = ff.yardstick(seed, table=True, q=13)[0]
    cls = ly.classes(rd, ff.L, table, 13, 0, n_pos=len(whole))
    assert cls.shape == (rd["n_reads"], len(whole)) and set(np.unique(cls).tolist()) == set(range(7))
    cols = list(range(len(whole) + 3))
    for k in (1, 3):
        j = ly.joint(cls, cols, k)
        recs = ly.records(cols, k, j)
        assert not ly.invariant(recs, k, whole), ly.invariant(recs, k, whole)
        assert not j[:, 0, 0].any() and j[:, 1:, 0].any() and j[:, 0, 1:].any() and (recs["b"] == -1).sum() == k * (k + 1) // 2
        first, second = ly.marginals(j, cols, k)
        want = ly.classes_of_matrix(whole, cols)
        for i in range(len(cols) - k):
            assert first[i * k:i * k + k, 1:].tolist() == [want[i, 1:].tolist()] * k
            assert [second[i * k + d - 1, 1:].tolist() for d in range(1, k + 1)] == [want[i + d, 1:].tolist() for d in range(1, k + 1)]
    broken = ly.records(cols, 1, ly.joint(cls, cols, 1))
    at = int(np.argmax(whole[:, 0]))
    broken["j"][at][1][1] += 1
    assert "pair (%d, %d)" % (at, at + 1) in ly.invariant(broken, 1, whole)


# ---- command line -------------------------------------------------------------------------------------------------------------------


def test_flags_defaults_and_children(tmp_path):
    f = stub_files(tmp_path, ("x.bam", "r.fa", "f.gff", "o.csv.gz"))
    a = cli.GetArgs(_base(f) + ["--variant-table", "t.tsv", "--variant-links", "l.tsv"])
    assert (a.variant_links, a.link_neighbours, a.link_min_depth, a.link_ratio) == ("l.tsv", 2, 10, Fraction(9, 10))
    assert cli.links_of(a) == ("l.tsv", 2, dict(min_depth=10, ratio=Fraction(9, 10)))
    b = cli.GetArgs(_base(f) + ["--variant-table", "t.tsv"])
    assert b.variant_links is None and cli.links_of(b) is None and not any(x.startswith("--link") or x == "--variant-links" for x in cli._child_argv(b, True))
    got = [cli.GetArgs(_base(f) + ["--variant-table", "t.tsv", "--variant-links", "l.tsv", "--link-ratio", s, "--link-min-depth", "3", "--link-neighbours", "7"])
           for s in ("0.8", "8e-1", "4/5")]
    assert [(x.link_ratio, x.link_min_depth, x.link_neighbours) for x in got] == [(Fraction(4, 5), 3, 7)] * 3
    argv = cli._child_argv(got[0], True)                                                    # a --gpus child parses what the parent understood
    back = cli.GetArgs(argv)
    assert cli.links_of(back) == cli.links_of(got[0]) == ("l.tsv", 7, dict(min_depth=3, ratio=Fraction(4, 5))) and back.variant_table == "t.tsv"
    both = cli.GetArgs(_base(f) + ["--variant-table", "t.tsv", "--variant-links", "l.tsv", "--variant-strand", "--link-ratio", "1"])
    assert cli.strand_of(both) is not None and cli.links_of(both)[2]["ratio"] == 1
    back = cli.GetArgs(cli._child_argv(both, True))
    assert cli.strand_of(back) == cli.strand_of(both) and cli.links_of(back) == cli.links_of(both)
    assert cli.link_stats() == dict(variant_link_rows=0, variant_links_cis=0, variant_links_trans=0, variant_links_mixed=0, variant_links_none=0, variant_links_low=0)
    assert cli.link_stats(WANT7) == dict(variant_link_rows=9, variant_links_cis=2, variant_links_trans=1, variant_links_mixed=2, variant_links_none=2, variant_links_low=2)


@pytest.mark.parametrize("extra", (["--link-min-depth", "0"], ["--link-min-depth", "x"], ["--link-ratio", "1.5"], ["--link-ratio", "1/2"], ["--link-ratio", "0.3"],
                                   ["--link-ratio", "2000001/3000001"], ["--link-neighbours", "0"], ["--link-neighbours", "8"], ["--link-neighbours", "x"]))
def test_bad_link_thresholds_are_refused(tmp_path, capsys, extra):
    f = stub_files(tmp_path, ("x.bam", "r.fa", "f.gff", "o.csv.gz"))
    with pytest.raises(SystemExit) as e:
        cli.GetArgs(_base(f) + ["--variant-table", "t.tsv", "--variant-links", "l.tsv"] + extra)
    assert e.value.code == 2 and extra[0] in capsys.readouterr().err


def test_refusals_exit_1_with_one_line_and_write_nothing(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    f = stub_files(tmp_path, ("x.bam", "r.fa", "f.gff", "o.csv.gz"))
    man = tmp_path / "m.tsv"
    man.write_text("%s\tS0\to0.fa\t-\t-\t-\tt0.tsv\n" % f["x.bam"])
    batch = ["--batch", str(man), "-ref", f["r.fa"], "-gff", f["f.gff"], "-cov", "30"]
    before = sorted(os.listdir(tmp_path))
    for argv, word in ((_base(f) + ["--variant-links", "l.tsv"], "--variant-links needs --variant-table"),
                       (_base(f) + ["--variant-table", "t.tsv", "--link-min-depth", "5"], "need --variant-links"),
                       (_base(f) + ["--variant-table", "t.tsv", "--link-ratio", "4/5"], "need --variant-links"),
                       (_base(f) + ["--variant-table", "t.tsv", "--link-neighbours", "3"], "need --variant-links"),
                       (_base(f) + ["--link-neighbours", "3"], "need --variant-links"),
                       (batch + ["--variant-links", "l.tsv"], "--batch is refused"),
                       (batch + ["--variant-links", "l.tsv", "--gpus", "2"], "--batch is refused"),
                       (_base(f) + ["--variant-table", "t.tsv", "--variant-links", "l.tsv", "--index-override", f["o.csv.gz"]], "--index-override"),
                       (_base(f) + ["--variant-table", "t.tsv", "--variant-links", "l.tsv", "--index-override", f["o.csv.gz"], "--gpus", "2"], "--index-override")):
        for call in (cli.GetArgs, cli.main):
            with pytest.raises(SystemExit) as e:
                call(argv)
            out = capsys.readouterr().out
            assert e.value.code == 1 and word in out and "--variant-links" in out and out.count("\n") == 1 and out.endswith("Exiting...\n"), (argv, out)
    assert sorted(os.listdir(tmp_path)) == before
