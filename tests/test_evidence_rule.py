"""--variant-evidence without a GPU: the evidence verdict and the LDS bound (csrc/evidence_rule.h) and the row writer
(csrc/variants_evidence_text.cpp) as a program of their own (tests/evidence_main.cpp), built plain and under AddressSanitizer + UBSan,
against Python's integers (tests/evidence_yardstick.py); the same writer through the ABI; the yardstick's walk on hand-made records and
against the committed oracles; the numpy restatement for tests/fixed_reads.py's records; and the command line's argument handling.  The
kernel's tests are tests/test_evidence_counts.py."""
import os
import struct

import numpy as np
import pytest

from tests import evidence_cases as ec
from tests import evidence_yardstick as ey
from tests import fixed_reads as fx
from tests import fuzz_masked as fm
from tests import host_program
from tests import read_specs as rsp
from tests import schemes as sch
from tests import variant_yardstick as vy
from tests.cli_run import base_args as _base
from tests.cli_run import stub_files
from trueconsense_amd import TrueConsense as cli
from trueconsense_amd import _ffi, engine

TOP = (1 << 31) - 1


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("evidence_main")
    src = ["tests/evidence_main.cpp", "trueconsense_amd/csrc/variants_evidence_text.cpp"]
    return {"plain": host_program.build(src, d / "evidence_main", sanitize=False), "sanitized": host_program.build(src, d / "evidence_main_san")}


def _run(prog, mode, inp, out):
    r = host_program.run(prog, mode, inp, out)
    assert r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-4000:])


# ---- the verdict ------------------------------------------------------------------------------------------------------------------
def sweep():
    """-> [(n, qual, mapq, dist, min_qual, min_mapq, min_dist)]: n from 0 to 2^31 - 1 and each sum at, one below and one above
    threshold * n, thresholds 0, 1, 20, 255; sums of 255 * n at n = 2^31 - 1; random cases"""
    cases = []
    for n in (0, 1, 2, 7, 1000, 65536, TOP // 255, TOP // 255 + 1, TOP):
        for t in (0, 1, 5, 20, 255):
            for d in (-1, 0, 1):
                edge = max(t * n + d, 0)
                cases += [(n, edge, 255 * n, 255 * n, t, 20, 5), (n, 255 * n, edge, 255 * n, 20, t, 5), (n, 255 * n, 255 * n, edge, 20, 20, t),
                          (n, edge, edge, edge, t, t, t)]
    cases += [(TOP, 255 * TOP, 255 * TOP, 255 * TOP, 255, 255, 255), (TOP, 255 * TOP - 1, 255 * TOP, 255 * TOP - 1, 255, 255, 255), (TOP, 0, 0, 0, 255, 255, 255),
              (TOP, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 255, 255, 255)]
    rng = np.random.default_rng(6)
    for _ in range(2000):
        n = int(rng.integers(0, 1 << 31))
        cases.append((n,) + tuple(int(rng.integers(0, 255 * n + 1)) for _ in range(3)) + tuple(int(x) for x in rng.integers(0, 256, 3)))
    return cases


@pytest.mark.parametrize("build", ("plain", "sanitized"))
def test_verdict_program_against_python_integers(programs, tmp_path, build):
    cases = sweep()
    want = [ey.verdict(*c) for c in cases]
    # what the sweep holds
    assert set(want) == set(range(8))
    assert all(w == 0 for w, c in zip(want, cases) if c[0] == 0) and any(c[0] == 0 and max(c[4:]) == 255 for c in cases)      # n = 0 gives 0
    for k in range(3):                                                                      # a threshold of 0 switches its bit off
        assert any(c[4 + k] == 0 and c[0] for c in cases) and not any(w >> k & 1 for w, c in zip(want, cases) if c[4 + k] == 0)
        ties = [i for i, c in enumerate(cases) if c[0] and c[4 + k] and c[1 + k] == c[4 + k] * c[0]]
        assert len(ties) >= 20 and not any(want[i] >> k & 1 for i in ties)                  # a mean at the threshold passes
        assert any(want[i] >> k & 1 for i, c in enumerate(cases) if c[0] and c[1 + k] == c[4 + k] * c[0] - 1)
    wide = [i for i, c in enumerate(cases) if c[0] == TOP and ey.verdict_in_32_bits(*c) != want[i]]
    assert len(wide) >= 5, "no case of the sweep needs products of more than 32 bits"
    inp, out = str(tmp_path / "v.in"), str(tmp_path / "v.out")
    with open(inp, "wb") as fh:
        fh.write(struct.pack("<q", len(cases)) + np.array(cases, np.int64).tobytes())
    _run(programs[build], "verdict", inp, out)
    got = np.fromfile(out, np.int32).tolist()
    bad = [(cases[i], got[i], want[i]) for i in range(len(cases)) if got[i] != want[i]]
    assert not bad, bad[:8]
    assert [engine.evidence_verdict(*cases[i]) for i in wide[:5]] == [want[i] for i in wide[:5]]


def test_verdict_argument_errors():
    lib = _ffi.lib()
    for bad in ((1, 1, 1, 1, 256, 0, 0), (1, 1, 1, 1, 0, 256, 0), (1, 1, 1, 1, 0, 0, 256), (1, 1, 1, 1, -1, 0, 0), (1, 1, 1, 1, 0, -1, 0), (1, 1, 1, 1, 0, 0, -1),
                (-1, 1, 1, 1, 20, 20, 5), (1, -1, 1, 1, 20, 20, 5), (1, 1, -1, 1, 20, 20, 5), (1, 1, 1, -1, 20, 20, 5)):
        assert lib.tcmi_evidence_verdict(*bad) == _ffi.E_ARG, bad
    assert lib.tcmi_evidence_verdict(1, 255, 255, 255, 255, 255, 255) == 0 and lib.tcmi_evidence_verdict(1, 254, 254, 254, 255, 255, 255) == 7
    with pytest.raises(_ffi.TcmiError):
        engine.evidence_verdict(1, 1, 1, 1, min_qual=256)


# ---- the LDS bound ----------------------------------------------------------------------------------------------------------------
def lds_ok(n_cols, n_records, grid, block):
    if not 1 <= n_cols <= 128 or n_records < 0 or grid < 1 or block < 1:
        return 0
    blocks = -(-n_records // block)
    return int(255 * (-(-blocks // grid)) * block <= (1 << 32) - 1)


@pytest.mark.parametrize("build", ("plain", "sanitized"))
def test_the_lds_bound_at_its_edge(programs, tmp_path, build):
    """a workgroup of 256 lanes may visit 65 793 trips' worth of records (255 * 65 793 * 256 = 2^32 - 256) and not one trip more"""
    trips = ((1 << 32) - 1) // (255 * 256)
    assert trips == 65793 and 255 * trips * 256 <= (1 << 32) - 1 < 255 * (trips + 1) * 256
    cases = []
    for grid in (1, 7, 2048):
        full = trips * grid * 256
        cases += [(128, full, grid, 256), (128, full + 1, grid, 256), (128, full - 255, grid, 256), (1, full, grid, 256), (129, 1000, grid, 256), (0, 1000, grid, 256),
                  (128, 0, grid, 256), (128, 1, grid, 256), (128, -1, grid, 256)]
    cases += [(128, 1000, 0, 256), (128, 1000, 8, 0), (128, (1 << 62), 1, 256), (128, (1 << 62), 1 << 40, 256), (64, 16843009, 1, 1), (64, 16843010, 1, 1)]
    want = [lds_ok(*c) for c in cases]
    assert want[:4] == [1, 0, 1, 1] and want.count(1) >= 10 and want.count(0) >= 10 and want[-2:] == [1, 0]
    inp, out = str(tmp_path / "l.in"), str(tmp_path / "l.out")
    with open(inp, "wb") as fh:
        fh.write(struct.pack("<q", len(cases)) + np.array(cases, np.int64).tobytes())
    _run(programs[build], "lds", inp, out)
    got = np.fromfile(out, np.int32).tolist()
    assert got == want, [(c, g, w) for c, g, w in zip(cases, got, want) if g != w]


# ---- the text ---------------------------------------------------------------------------------------------------------------------
REF = b"AAcNGTTGARtA"
RECS = [(0, 2, 5, 20), (2, 4, 10, 40), (2, 5, 4, 40), (6, 3, 9, 10), (7, 1, 30, 100), (7, 6, 30, 100), (10, 5, 3, 12), (11, 5, 30, 30)]
#        position -> (n, qual, mapq, dist) in plane order (coverage, A, T, C, G, X, I)
EV = {0: ((20, 15, 5, 0, 0, 0, 0), (700, 600, 99, 0, 0, 0, 0), (1200, 900, 300, 0, 0, 0, 0), (200, 150, 25, 0, 0, 0, 0)),          # T: mean quality 19.8: LOWQ
      2: ((40, 0, 0, 26, 10, 4, 0), (1400, 0, 0, 1000, 200, 160, 0), (2400, 0, 0, 1560, 199, 240, 0), (400, 0, 0, 300, 49, 8, 0)),  # G: LOWMQ, END; X: END
      6: ((10, 0, 0, 9, 0, 0, 1), (300, 0, 0, 270, 0, 0, 30), (600, 0, 0, 540, 0, 0, 60), (100, 0, 0, 90, 0, 0, 10)),              # reference T: nobody has it
      7: ((100, 30, 15, 15, 5, 15, 30), (3000, 599, 15, 15, 101, 15, 600), (6000, 600, 15, 15, 301, 15, 599), (1000, 150, 15, 15, 26, 15, 149)),
      10: ((12, 0, 9, 0, 0, 3, 0), (400, 0, 300, 0, 0, 0, 0), (700, 0, 500, 0, 0, 0, 0), (100, 0, 80, 0, 0, 0, 0)),                # X with all sums 0: every name
      11: ((30, 0, 0, 0, 0, 30, 0), (7650, 0, 0, 0, 0, 7650, 0), (7650, 0, 0, 0, 0, 7650, 0), (7650, 0, 0, 0, 0, 7650, 0))}        # 255 everywhere
WANT = ("ctg\t1\tA\tT\t5\t20\t0.250000\t40.0\t19.8\t60.0\t60.0\t10.0\t5.0\tLOWQ\n"
        "ctg\t3\tC\tG\t10\t40\t0.250000\t38.4\t20.0\t60.0\t19.9\t11.5\t4.9\tLOWMQ,END\n"
        "ctg\t3\tC\t*\t4\t40\t0.100000\t38.4\t40.0\t60.0\t60.0\t11.5\t2.0\tEND\n"
        "ctg\t7\tT\tC\t9\t10\t0.900000\t0.0\t30.0\t0.0\t60.0\t0.0\t10.0\tPASS\n"
        "ctg\t8\tG\tA\t30\t100\t0.300000\t20.2\t19.9\t60.2\t20.0\t5.2\t5.0\tLOWQ\n"
        "ctg\t8\tG\t+\t30\t100\t0.300000\t20.2\t20.0\t60.2\t19.9\t5.2\t4.9\tLOWMQ,END\n"
        "ctg\t11\tT\t*\t3\t12\t0.250000\t33.3\t0.0\t55.5\t0.0\t8.8\t0.0\tLOWQ,LOWMQ,END\n"
        "ctg\t12\tA\t*\t30\t30\t1.000000\t0.0\t255.0\t0.0\t255.0\t0.0\t255.0\tPASS\n")
RULE = (20, 20, 5)


def ev_array(ev=EV):
    cols = sorted(ev)
    return ey.records(cols, [np.array([ev[c][k] for c in cols], np.int64).reshape(len(cols), 7) for k in range(4)])


def run_text(prog, tmp_path, tag, recs, ev, rule, region, ref, pos_offset=0):
    inp, out = str(tmp_path / (tag + ".in")), str(tmp_path / (tag + ".out"))
    with open(inp, "wb") as fh:
        fh.write(struct.pack("<8q", len(recs), len(ev), *rule, pos_offset, len(region.encode()), len(ref)))
        fh.write(region.encode() + ref + vy.as_array(recs).tobytes() + np.ascontiguousarray(ev, ey.DTYPE).tobytes())
    _run(prog, "text", inp, out)
    raw = open(out, "rb").read()
    head, _, body = raw.partition(b"\n")
    rc, ln = (int(x) for x in head.split())
    assert len(body) == ln
    return rc, body.decode("latin-1")


def test_yardstick_text_on_the_hand_written_rows():
    """every allele kind (a base, '*', '+'), n = 0 for the reference's plane and for the allele's sums, names alone and all three"""
    assert ey.text(RECS, EV, "ctg", REF, *RULE) == WANT
    assert {ln.split("\t")[-1] for ln in WANT.splitlines()} == {"PASS", "LOWQ", "END", "LOWMQ,END", "LOWQ,LOWMQ,END"}


@pytest.mark.parametrize("build", ("plain", "sanitized"))
def test_text_program(programs, tmp_path, build):
    """the rows, the first seven fields against tcmi_variants_text, the refusals; the program itself checks the sizing call, a buffer
    one byte short, a buffer with room to spare and that a refusal writes nothing"""
    prog = programs[build]
    rc, text = run_text(prog, tmp_path, "hand", RECS, ev_array(), RULE, "ctg", REF)
    assert rc == 0 and text == WANT
    plain = engine.variants_text(vy.as_array(RECS), "ctg", REF).splitlines()
    assert [ln.split("\t")[:7] for ln in text.splitlines()] == [ln.split("\t") for ln in plain]
    assert run_text(prog, tmp_path, "none", [], ev_array({}), RULE, "ctg", REF) == (0, "")
    # a position offset, all thresholds off
    rc, text = run_text(prog, tmp_path, "off", RECS[3:], ev_array({k: v for k, v in EV.items() if k >= 6}), (0, 0, 0), "seg 2", REF, 6)
    assert rc == 0 and text == ey.text(RECS[3:], EV, "seg 2", REF, 0, 0, 0, 6) and text.startswith("seg 2\t1\tT\tC") and {ln.split("\t")[-1] for ln in text.splitlines()} == {"PASS"}
    # a reference base that is none of A, T, C, G: zeros in the REF columns (the rule of the table skips such a position; the writer takes it)
    n_ref = [(3, 1, 15, 20)]
    ev_n = {3: EV[0]}
    rc, text = run_text(prog, tmp_path, "n", n_ref, ev_array(ev_n), RULE, "ctg", REF)
    assert rc == 0 and text == ey.text(n_ref, ev_n, "ctg", REF, *RULE) == "ctg\t4\tN\tA\t15\t20\t0.750000\t0.0\t40.0\t0.0\t60.0\t0.0\t10.0\tPASS\n"
    # random rows with counts up to 2^31 - 1 and sums up to 255 times as much
    rng = np.random.default_rng(3)
    ref = bytes(rng.choice(np.frombuffer(b"ACGTacgtN", np.uint8), 400))
    recs, ev = [], {}
    for p in sorted(rng.choice(400, 150, replace=False).tolist()):
        n = rng.integers(0, 1 << 31, 7) // (1 if p % 3 else 1 << 24)
        n[1 + p % 6] *= p % 4 != 0                                                          # (a plane nobody has: its mean is 0.0)
        ev[p] = (n.tolist(),) + tuple([int(rng.integers(0, (60 if p % 2 else 255) * int(x) + 1)) for x in n] for _ in range(3))
        for a in sorted(rng.choice(np.arange(1, 7), int(rng.integers(1, 4)), replace=False).tolist()):
            if n[0]:
                recs.append((p, a, int(n[a]), int(n[0])))
    ev = {p: v for p, v in ev.items() if any(r[0] == p for r in recs)}
    rc, text = run_text(prog, tmp_path, "big", recs, ev_array(ev), (30, 30, 30), "MN908947.3", ref)
    assert rc == 0 and text == ey.text(recs, ev, "MN908947.3", ref, 30, 30, 30)
    assert len({ln.split("\t")[-1] for ln in text.splitlines()}) >= 6 and "\t0.0\t" in text
    # the refusals: TCMI_E_ARG and no text
    moved = ev_array()
    moved["pos"][2] += 1
    alt = ev_array()
    alt["n"][1][4] += 1                                                                     # n[G] = count + 1 at position 2
    tot = ev_array()
    tot["n"][4][0] -= 1                                                                     # n[coverage] = cov - 1 at position 10
    neg = ev_array()
    neg["dist"][0][3] = -1
    over = ev_array()
    over["qual"][5][5] = 255 * 30 + 1                                                       # more than 255 a token
    for tag, ev_, rule in (("pos", moved, RULE), ("alt", alt, RULE), ("tot", tot, RULE), ("short", ev_array()[:-1], RULE), ("neg", neg, RULE), ("over", over, RULE),
                           ("extra", ev_array({**EV, 12: EV[0]}), RULE), ("qual", ev_array(), (256, 20, 5)), ("mapq", ev_array(), (20, -1, 5)),
                           ("dist", ev_array(), (20, 20, 256))):
        assert run_text(prog, tmp_path, tag, RECS, ev_, rule, "ctg", REF) == (_ffi.E_ARG, ""), tag


def test_text_writer_through_the_abi():
    assert engine.variants_evidence_text(vy.as_array(RECS), ev_array(), "ctg", REF) == WANT
    assert engine.variants_evidence_text(vy.as_array(RECS), ev_array(), "ctg", REF, 0, 20, 20, 5) == WANT
    assert engine.variants_evidence_text(vy.as_array([]), ev_array({}), "ctg", REF) == ""
    assert engine.VARIANTS_EVIDENCE_HEADER.startswith(engine.VARIANTS_HEADER[:-1] + "\t") and engine.VARIANTS_EVIDENCE_HEADER.endswith("\tALT_ENDDIST\tEVIDENCE\n")
    assert engine.VARIANTS_EVIDENCE_HEADER.count("\t") == WANT.splitlines()[0].count("\t") == 13
    assert engine.EVIDENCE_DTYPE.itemsize == 200 and engine.EVIDENCE_DTYPE == ey.DTYPE and engine.EVIDENCE_LDS == 128
    assert _ffi.K_EVIDENCE_COUNTS == 16 and _ffi.lib().tcmi_abi_version() == 5
    bad = ev_array()
    bad["n"][0][2] += 1
    for ev in (bad, ev_array()[1:]):
        with pytest.raises(_ffi.TcmiError) as e:
            engine.variants_evidence_text(vy.as_array(RECS), ev, "ctg", REF)
        assert e.value.code == _ffi.E_ARG and "do not add up" in str(e.value)
    assert engine.evidence_verdict(10, 199, 200, 50) == 1 and engine.evidence_verdict(10, 200, 199, 50) == 2 and engine.evidence_verdict(10, 200, 200, 49) == 4
    assert engine.evidence_verdict(10, 0, 0, 0, 0, 0, 0) == 0 and engine.evidence_verdict(0, 0, 0, 0) == 0
    assert cli.evidence_stats(WANT) == dict(variant_evidence_lowq=3, variant_evidence_lowmq=3, variant_evidence_end=4)
    assert cli.evidence_stats() == dict(variant_evidence_lowq=0, variant_evidence_lowmq=0, variant_evidence_end=0)


# ---- the yardstick's walk -----------------------------------------------------------------------------------------------------------
def test_the_walk_on_the_hand_made_records_gives_what_the_rule_says():
    """tests/evidence_cases.HAND, worked out by hand from include/tcmi.h: soft and hard clips, the cap on a 700-base read, the D columns,
    a D that starts at a1, the insertion mark, MAPQ 0 / 60 / 255, no QUAL"""
    specs, by = ec.hand_records()
    assert {r["mapq"] for r in specs} == {0, 60, 255} and by["noqual"]["qual"] == [255] * 12 and by["long"]["cigar"] == "700M"
    sums, marks = ey.whole(rsp.arrays(specs), ec.L)
    for c, (qi, mapq, dist) in ec.HAND.items():
        quality = 255 if c >= 1400 else ec.hand_quality(qi)
        assert tuple(int(m[c, 0]) for m in sums) == (1, quality, mapq, dist), c
    assert sums[0][1307].tolist()[5:] == [0, 1] and sums[0][1110].tolist()[5:] == [1, 0] and sums[0][1210].tolist()[5:] == [1, 0]
    assert marks[1][300:1000].sum() == 444 - 255 + 1 and marks[1].sum() == 190 and sums[3][555:745, 0].min() == 255
    ec.not_vacuous(sums, marks, sorted(ec.HAND), "hand", capped=True)


@pytest.mark.parametrize("mode", sorted(fm.MODES))
@pytest.mark.parametrize("seed", fm.SEEDS)
def test_the_walk_on_the_fuzz_files(seed, mode):
    """every record's (column, quality) sequence is tc_oracle.read_tokens', the token counts are primer_yardstick.counts (both asserted
    inside the walk), the queries the GPU tests make are not vacuous, and the floor, the mask and the filter each remove a token"""
    sums, marks, n_pos = ec.sums_of(seed, mode)
    for cols in (ec.sparse_columns(seed, n_pos), list(range(n_pos))):
        ec.not_vacuous(sums, marks, cols, (seed, mode, len(cols)))
        if mode == "all":
            ec.removed_by_each(seed, cols, (seed, len(cols)))
    n, qual, mapq, dist = sums
    assert (qual <= 255 * n).all() and (mapq <= 255 * n).all() and (dist <= 255 * n).all() and marks[1].sum() > 0
    assert (n[:, 0] >= n[:, 1:6].sum(1)).all()


# ---- tests/fixed_reads.py's records ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", (0, 13))
def test_the_numpy_restatement_equals_the_yardstick(q):
    from oracle import c_oracle
    rd = fx.generate(2000, 7)
    flat = {"n_reads": 2000, "pos": rd["pos"], "flag": rd["flag"], "l_qseq": np.full(2000, fx.LEN, np.int32), "tid": np.zeros(2000, np.int32),
            "mapq": rd["mapq"], "cigar_off": np.arange(2001, dtype=np.uint64), "cigar": np.full(2000, fx.LEN << 4, np.uint32),
            "seq_off": np.arange(2001, dtype=np.uint64) * (fx.LEN // 2), "seq": ((rd["base"][:, 0::2] << 4) | rd["base"][:, 1::2]).reshape(-1).astype(np.uint8),
            "qual_off": np.arange(2001, dtype=np.uint64) * fx.LEN, "qual": rd["qual"].reshape(-1)}
    assert c_oracle.extent(flat, fx.L) == fx.L
    cols = list(range(fx.L)) + [fx.L + 5]
    for f, table, slack in ((fm.NONE, (), 0), (fx.MQ, (), 0), (fx.MQ, tuple(sch.PRIMER_SCHEME), 3)):
        want = ey.counts(flat, cols, fx.L, table, q, slack, 0, f)
        got = ec.fixed_counts(rd, cols, q, f, table, slack)
        assert not ec.differ(got, want, cols, (q, f, bool(table))), ec.differ(got, want, cols, (q, f, bool(table)))
        assert want[0][:, 1:5].sum(0).all() and len({int(m[:, 0].sum()) for m in want}) == 4 and not want[0][-1].any()
        fwd, rev = fx.strand(rd, cols, q, f, table, slack)
        assert np.array_equal(got[0], (fwd + rev).astype(np.int64))


# ---- command line -----------------------------------------------------------------------------------------------------------------
def test_flags_and_defaults(tmp_path):
    f = stub_files(tmp_path, ("x.bam", "r.fa", "f.gff", "o.csv.gz"))
    a = cli.GetArgs(_base(f) + ["--variant-table", "t.tsv", "--variant-evidence", "e.tsv"])
    assert (a.variant_evidence, a.evidence_min_qual, a.evidence_min_mapq, a.evidence_min_enddist) == ("e.tsv", 20, 20, 5)
    assert cli.evidence_of(a) == ("e.tsv", dict(min_qual=20, min_mapq=20, min_enddist=5))
    want = cli.StreamCounts(a)
    assert want and want.need == "--variant-evidence" and want.lists_records and want.evidence == cli.evidence_of(a) and "variant_evidence" not in want.KEYS
    assert "variant_evidence" not in want.split_kwargs("ACGT")
    b = cli.GetArgs(_base(f) + ["--variant-table", "t.tsv"])
    assert b.variant_evidence is None and cli.evidence_of(b) is None and not cli.StreamCounts(b)
    c = cli.GetArgs(_base(f) + ["--variant-table", "t.tsv", "--variant-evidence", "e.tsv", "--evidence-min-qual", "0", "--evidence-min-mapq", "0x10",
                                "--evidence-min-enddist", "255"])
    assert cli.evidence_of(c)[1] == dict(min_qual=0, min_mapq=16, min_enddist=255)
    d = cli.GetArgs(_base(f) + ["--variant-table", "t.tsv", "--variant-evidence", "e.tsv", "--variant-strand", "--variant-links", "l.tsv", "--indel-table", "i.tsv"])
    assert cli.StreamCounts(d).need == "--variant-strand" and cli.StreamCounts(d).evidence


@pytest.mark.parametrize("extra", (["--evidence-min-qual", "256"], ["--evidence-min-qual", "-1"], ["--evidence-min-mapq", "x"], ["--evidence-min-mapq", "300"],
                                   ["--evidence-min-enddist", "256"], ["--evidence-min-enddist=-3"]))
def test_bad_evidence_thresholds_are_refused(tmp_path, capsys, extra):
    f = stub_files(tmp_path, ("x.bam", "r.fa", "f.gff", "o.csv.gz"))
    with pytest.raises(SystemExit) as e:
        cli.GetArgs(_base(f) + ["--variant-table", "t.tsv", "--variant-evidence", "e.tsv"] + extra)
    assert e.value.code == 2 and extra[0].split("=")[0] in capsys.readouterr().err


def test_refusals_exit_1_with_one_line_and_write_nothing(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    f = stub_files(tmp_path, ("x.bam", "r.fa", "f.gff", "o.csv.gz"))
    man = tmp_path / "m.tsv"
    man.write_text("%s\tS0\to0.fa\t-\t-\t-\tt0.tsv\n" % f["x.bam"])
    batch = ["--batch", str(man), "-ref", f["r.fa"], "-gff", f["f.gff"], "-cov", "30"]
    ev = ["--variant-evidence", "e.tsv"]
    before = sorted(os.listdir(tmp_path))
    for argv, word in ((_base(f) + ev, "--variant-evidence needs --variant-table"),
                       (_base(f) + ["--variant-table", "t.tsv", "--evidence-min-qual", "5"], "need --variant-evidence"),
                       (_base(f) + ["--variant-table", "t.tsv", "--evidence-min-mapq", "5"], "need --variant-evidence"),
                       (_base(f) + ["--variant-table", "t.tsv", "--evidence-min-enddist", "0"], "need --variant-evidence"),
                       (_base(f) + ["--evidence-min-enddist", "5"], "need --variant-evidence"),
                       (batch + ev, "--batch is refused"),
                       (batch + ev + ["--gpus", "2"], "--batch is refused"),
                       (_base(f) + ["--variant-table", "t.tsv"] + ev + ["--index-override", f["o.csv.gz"]], "--index-override"),
                       (_base(f) + ["--variant-table", "t.tsv"] + ev + ["--gpus", "2"], "--variant-evidence does not go with -i --gpus N"),
                       (_base(f) + ["--variant-table", "t.tsv", "--variant-strand"] + ev + ["--gpus", "2"], "--variant-evidence does not go with -i --gpus N")):
        for call in (cli.GetArgs, cli.main):
            with pytest.raises(SystemExit) as e:
                call(argv)
            out = capsys.readouterr().out
            assert e.value.code == 1 and word in out and out.count("\n") == 1 and out.endswith("Exiting...\n"), (argv, out)
    assert sorted(os.listdir(tmp_path)) == before
