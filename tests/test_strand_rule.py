"""--variant-strand without a GPU: the strand verdict (csrc/strand_rule.h) and the row writer (csrc/variants_strand_text.cpp) as a
program of their own (tests/strand_main.cpp), built plain and under AddressSanitizer + UBSan, against Python's integers
(tests/strand_yardstick.py); the same writer through the ABI; the yardstick's two halves against the yardstick over all records; and
the command line's argument handling.  The kernel's tests are tests/test_strand_counts.py."""
import os
import struct
from fractions import Fraction

import numpy as np
import pytest

from tests import fuzz_masked as ff
from tests import host_program
from tests import strand_yardstick as sy
from tests import variant_yardstick as vy
from tests.cli_run import base_args as _base
from tests.cli_run import stub_files
from trueconsense_amd import TrueConsense as cli
from trueconsense_amd import _ffi, engine

TOP = (1 << 31) - 1


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("strand_main")
    src = ["tests/strand_main.cpp", "trueconsense_amd/csrc/variants_strand_text.cpp"]
    return {"plain": host_program.build(src, d / "strand_main", sanitize=False), "sanitized": host_program.build(src, d / "strand_main_san")}


def _run(prog, mode, inp, out):
    r = host_program.run(prog, mode, inp, out)
    assert r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-4000:])


def sweep():
    """-> [(alt_fwd, alt_rev, tot_fwd, tot_rev, min_strand_depth, num, den)]: a dense small sweep (ties arise by themselves, each side
    below, at and above the depth), planted ties, num = 0 and num = den, and counts at 2^31 - 1 with den = 10^6"""
    cases = []
    ratios = ((0, 1), (1, 1), (1, 10), (1, 2), (333333, 1000000), (999999, 1000000), (1, 1000000))
    for num, den in ratios:
        for tf in (9, 10, 11, 20):
            for tr in (9, 10, 11, 30):
                for af in range(0, 13, 1 if (num, den) == (1, 10) else 3):
                    for ar in range(0, 13):
                        cases.append((af, ar, tf, tr, 10, num, den))
    for k in (1, 7, 1000, 214748):                          # alt_rev / alt_fwd = 10 at equal depths: the tie, one read below it, one above
        for d in (-1, 0, 1):
            cases.append((k, 10 * k + d, 3000000, 3000000, 10, 1, 10))
            cases.append((10 * k + d, k, 3000000, 3000000, 10, 1, 10))
    for num, den in ((1, 10), (100001, 1000000), (999999, 1000000), (500000, 1000000), (1000000 - 1, 1000000), (1, 1), (0, 1)):
        for af, ar in ((TOP, TOP), (TOP, TOP // 10), (TOP // 10, TOP), (TOP, TOP - 1), (TOP, 214748365), (TOP, 214748364), (TOP, 0), (0, 0), (12345, TOP)):
            cases.append((af, ar, TOP, TOP, 10, num, den))
            cases.append((af, ar, TOP, TOP - 1, TOP - 1, num, den))
            cases.append((af, ar, TOP, TOP - 1, TOP, num, den))        # the reverse strand one read below the depth: LOW
    rng = np.random.default_rng(5)
    for _ in range(2000):
        tf, tr = (int(x) for x in rng.integers(1, 1 << 31, 2))
        num, den = ratios[int(rng.integers(0, len(ratios)))]
        cases.append((int(rng.integers(0, tf + 1)), int(rng.integers(0, tr + 1)), tf, tr, int(rng.integers(1, 1 << 20)), num, den))
    return cases


@pytest.mark.parametrize("build", ("plain", "sanitized"))
def test_verdict_program_against_python_integers(programs, tmp_path, build):
    cases = sweep()
    want = [sy.verdict(*c) for c in cases]
    # what the sweep holds
    x = [(c[0] * c[3], c[1] * c[2]) for c in cases]
    ties = [i for i, c in enumerate(cases) if want[i] != 2 and max(x[i]) > 0 and min(x[i]) * c[6] == max(x[i]) * c[5]]
    assert len(ties) >= 100 and all(want[i] == 0 for i in ties)                             # an exact tie is PASS
    assert any(c[5] == 0 for c in cases) and not any(w == 1 for w, c in zip(want, cases) if c[5] == 0)      # num = 0 never gives BIAS
    assert any(w == 1 for w, c in zip(want, cases) if c[5] == c[6]) and any(w == 0 for w, c in zip(want, cases) if c[5] == c[6] and c[0])
    for side in (2, 3):                                                                     # each side below, at and above the depth
        assert {(c[side] > c[4]) - (c[side] < c[4]) for c in cases} == {-1, 0, 1}
    assert {0, 1, 2} == set(want)
    narrow = [i for i, c in enumerate(cases) if c[2] >= TOP - 1 and c[6] == 1000000 and sy.verdict_in_64_bits(*c) != want[i]]
    assert len(narrow) >= 5, "no case of the sweep needs more than 64 bits"
    inp, out = str(tmp_path / "v.in"), str(tmp_path / "v.out")
    with open(inp, "wb") as fh:
        fh.write(struct.pack("<q", len(cases)) + np.array(cases, np.int64).tobytes())
    _run(programs[build], "verdict", inp, out)
    got = np.fromfile(out, np.int32).tolist()
    bad = [(cases[i], got[i], want[i]) for i in range(len(cases)) if got[i] != want[i]]
    assert not bad, bad[:8]
    assert [engine.strand_verdict(*cases[i][:5], Fraction(cases[i][5], cases[i][6])) for i in narrow[:5] + ties[:5]] == [want[i] for i in narrow[:5] + ties[:5]]


def test_verdict_argument_errors():
    lib = _ffi.lib()
    for bad in ((1, 1, 5, 5, 0, 1, 10), (1, 1, 5, 5, 1, 1, 0), (1, 1, 5, 5, 1, 1, 1000001), (1, 1, 5, 5, 1, 11, 10), (1, 1, 5, 5, 1, -1, 10), (-1, 1, 5, 5, 1, 1, 10),
                (1, 1, 5, -5, 1, 1, 10)):
        assert lib.tcmi_strand_verdict(*bad) == _ffi.E_ARG, bad
    assert lib.tcmi_strand_verdict(1, 1, 5, 5, 1, 1, 1000000) == 0


# ---- the text ---------------------------------------------------------------------------------------------------------------------
REF = b"AAcNGTTGARtA"
RECS = [(0, 2, 5, 20), (2, 4, 10, 40), (2, 5, 4, 40), (6, 3, 9, 10), (7, 1, 30, 100), (7, 6, 30, 100), (10, 5, 3, 12), (11, 5, 30, 30)]
#        position -> (fwd, rev) in plane order (coverage, A, T, C, G, X, I)
STRAND = {0: ((10, 8, 2, 0, 0, 0, 0), (10, 7, 3, 0, 0, 0, 0)),              # T on both strands: PASS
          2: ((30, 0, 0, 20, 10, 0, 0), (10, 0, 0, 6, 0, 4, 0)),            # G on the forward strand only, X on the reverse only: BIAS twice
          6: ((10, 0, 0, 9, 0, 0, 1), (0, 0, 0, 0, 0, 0, 0)),               # nobody on the reverse strand: LOW
          7: ((50, 15, 15, 15, 5, 15, 15), (50, 15, 15, 15, 0, 15, 15)),
          10: ((6, 0, 6, 0, 0, 3, 3), (6, 0, 6, 0, 0, 0, 0)),               # 6 reads a strand under min_strand_depth 5; X one-sided: BIAS
          11: ((26, 0, 0, 0, 0, 26, 0), (4, 0, 0, 0, 0, 4, 0))}             # the reverse strand below the depth: LOW
WANT = ("ctg\t1\tA\tT\t5\t20\t0.250000\t8\t7\t2\t3\t10\t10\tPASS\n" "ctg\t3\tC\tG\t10\t40\t0.250000\t20\t6\t10\t0\t30\t10\tBIAS\n"
        "ctg\t3\tC\t*\t4\t40\t0.100000\t20\t6\t0\t4\t30\t10\tBIAS\n" "ctg\t7\tT\tC\t9\t10\t0.900000\t0\t0\t9\t0\t10\t0\tLOW\n"
        "ctg\t8\tG\tA\t30\t100\t0.300000\t5\t0\t15\t15\t50\t50\tPASS\n" "ctg\t8\tG\t+\t30\t100\t0.300000\t5\t0\t15\t15\t50\t50\tPASS\n"
        "ctg\t11\tT\t*\t3\t12\t0.250000\t6\t6\t3\t0\t6\t6\tBIAS\n" "ctg\t12\tA\t*\t30\t30\t1.000000\t0\t0\t26\t4\t26\t4\tLOW\n")


def strand_array(strand=STRAND):
    cols = sorted(strand)
    return sy.records(cols, [strand[c][0] for c in cols], [strand[c][1] for c in cols])


def run_text(prog, tmp_path, tag, recs, strand, rule, region, ref, pos_offset=0):
    inp, out = str(tmp_path / (tag + ".in")), str(tmp_path / (tag + ".out"))
    with open(inp, "wb") as fh:
        fh.write(struct.pack("<8q", len(recs), len(strand), *rule, pos_offset, len(region.encode()), len(ref)))
        fh.write(region.encode() + ref + vy.as_array(recs).tobytes() + np.ascontiguousarray(strand, sy.DTYPE).tobytes())
    _run(prog, "text", inp, out)
    raw = open(out, "rb").read()
    head, _, body = raw.partition(b"\n")
    rc, ln = (int(x) for x in head.split())
    assert len(body) == ln
    return rc, body.decode("latin-1")


def test_yardstick_text_on_the_hand_written_rows():
    assert sy.text(RECS, STRAND, "ctg", REF, 5, 1, 10) == WANT
    assert {ln.split("\t")[-1] for ln in WANT.splitlines()} == {"PASS", "BIAS", "LOW"}


@pytest.mark.parametrize("build", ("plain", "sanitized"))
def test_text_program(programs, tmp_path, build):
    """the rows, the first seven fields against tcmi_variants_text, the refusals; the program itself checks the sizing call, a buffer
    one byte short and a buffer with room to spare"""
    prog = programs[build]
    rc, text = run_text(prog, tmp_path, "hand", RECS, strand_array(), (5, 1, 10), "ctg", REF)
    assert rc == 0 and text == WANT
    plain = engine.variants_text(vy.as_array(RECS), "ctg", REF).splitlines()
    assert [ln.split("\t")[:7] for ln in text.splitlines()] == [ln.split("\t") for ln in plain]
    assert run_text(prog, tmp_path, "none", [], strand_array({}), (5, 1, 10), "ctg", REF) == (0, "")
    rc, text = run_text(prog, tmp_path, "off", RECS[3:], strand_array({k: v for k, v in STRAND.items() if k >= 6}), (10, 0, 1), "seg 2", REF, 6)
    assert rc == 0 and text == sy.text(RECS[3:], STRAND, "seg 2", REF, 10, 0, 1, 6) and "BIAS" not in text and text.startswith("seg 2\t1\tT\tC")
    # random rows with counts up to 2^31 - 1
    rng = np.random.default_rng(3)
    ref = bytes(rng.choice(np.frombuffer(b"ACGTacgt", np.uint8), 400))
    recs, strand = [], {}
    for p in sorted(rng.choice(400, 150, replace=False).tolist()):
        fwd = rng.integers(0, 1 << 30, 7)
        rev = rng.integers(0, 1 << 30, 7) // (1 if p % 3 else 1 << 20)
        strand[p] = (fwd.tolist(), rev.tolist())
        for a in sorted(rng.choice(np.arange(1, 7), int(rng.integers(1, 4)), replace=False).tolist()):
            recs.append((p, a, int(fwd[a] + rev[a]), int(fwd[0] + rev[0])))
    rc, text = run_text(prog, tmp_path, "big", recs, strand_array(strand), (1000, 333333, 1000000), "MN908947.3", ref)
    assert rc == 0 and text == sy.text(recs, strand, "MN908947.3", ref, 1000, 333333, 1000000)
    assert {ln.split("\t")[-1] for ln in text.splitlines()} == {"PASS", "BIAS", "LOW"}
    # the refusals: TCMI_E_ARG and no text
    moved = strand_array()
    moved["pos"][2] += 1
    alt = strand_array()
    alt["fwd"][1][4] += 1                                                                   # alt_fwd + alt_rev = count + 1 at position 2
    tot = strand_array()
    tot["rev"][4][0] -= 1                                                                   # tot_fwd + tot_rev = cov - 1 at position 10
    for tag, strand_, rule in (("pos", moved, (5, 1, 10)), ("alt", alt, (5, 1, 10)), ("tot", tot, (5, 1, 10)), ("short", strand_array()[:-1], (5, 1, 10)),
                               ("extra", strand_array({**STRAND, 12: STRAND[0]}), (5, 1, 10)), ("depth", strand_array(), (0, 1, 10)), ("den", strand_array(), (5, 1, 1000001)),
                               ("num", strand_array(), (5, 11, 10))):
        assert run_text(prog, tmp_path, tag, RECS, strand_, rule, "ctg", REF) == (_ffi.E_ARG, ""), tag


def test_text_writer_through_the_abi():
    assert engine.variants_strand_text(vy.as_array(RECS), strand_array(), "ctg", REF, min_strand_depth=5) == WANT
    assert engine.variants_strand_text(vy.as_array(RECS), strand_array(), "ctg", REF, 0, 5, "0.1") == WANT
    assert engine.variants_strand_text(vy.as_array([]), strand_array({}), "ctg", REF) == ""
    assert engine.VARIANTS_STRAND_HEADER.startswith(engine.VARIANTS_HEADER[:-1] + "\t") and engine.VARIANTS_STRAND_HEADER.endswith("\tTOTAL_REV\tSTRAND\n")
    assert engine.STRAND_DTYPE.itemsize == 64 and engine.STRAND_DTYPE == sy.DTYPE and engine.STRAND_LDS == 256
    bad = strand_array()
    bad["fwd"][0][2] += 1
    for strand in (bad, strand_array()[1:]):
        with pytest.raises(_ffi.TcmiError) as e:
            engine.variants_strand_text(vy.as_array(RECS), strand, "ctg", REF, min_strand_depth=5)
        assert e.value.code == _ffi.E_ARG and "do not add up" in str(e.value)
    assert engine.strand_verdict(5, 5, 50, 50) == 0 and engine.strand_verdict(5, 0, 50, 50) == 1 and engine.strand_verdict(5, 5, 50, 9) == 2
    assert engine.strand_verdict(5, 5, 50, 9, min_strand_depth=9) == 0 and engine.strand_verdict(1, 9, 50, 50, strand_ratio="1/8") == 1
    with pytest.raises(_ffi.TcmiError):
        engine.strand_verdict(1, 1, 5, 5, min_strand_depth=0)


# ---- the yardstick's halves -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ff.SEEDS)
def test_the_two_strands_add_up_to_the_yardstick_over_all_records(seed):
    """under floor 13 and the seed's primer table: strand_yardstick.counts' halves sum to primer_yardstick.counts on every column, both
    halves hold something on every plane, and neither is the whole"""
    _, rd = ff.passing(seed)
    table = ff.table_of(seed)
    whole = ff.yardstick(seed, table=True, q=13)[0]
    cols = list(range(len(whole) + 3))                                                      # (... and three columns beyond every read)
    fwd, rev = sy.counts(rd, cols, ff.L, table, 13, 0)
    assert np.array_equal(fwd + rev, sy.at(whole, cols))
    assert fwd.sum(0).all() and rev.sum(0).all() and not fwd[-3:].any() and not rev[-3:].any()
    n_rev = int(((rd["flag"] & 0x10) != 0).sum())
    assert 0.2 < n_rev / rd["n_reads"] < 0.5
    half = sy.subset(rd, (rd["flag"] & 0x10) != 0)
    assert half["n_reads"] == n_rev and not ((half["flag"] & 0x10) == 0).any() and len(half["cigar_off"]) == n_rev + 1


# ---- command line -----------------------------------------------------------------------------------------------------------------


def test_flags_defaults_and_children(tmp_path):
    f = stub_files(tmp_path, ("x.bam", "r.fa", "f.gff", "o.csv.gz"))
    a = cli.GetArgs(_base(f) + ["--variant-table", "t.tsv", "--variant-strand"])
    assert (a.variant_strand, a.strand_min_depth, a.strand_ratio) == (True, 10, Fraction(1, 10))
    assert cli.strand_of(a) == dict(min_strand_depth=10, strand_ratio=Fraction(1, 10))
    b = cli.GetArgs(_base(f) + ["--variant-table", "t.tsv"])
    assert b.variant_strand is False and cli.strand_of(b) is None and "--variant-strand" not in cli._child_argv(b, True)
    got = [cli.GetArgs(_base(f) + ["--variant-table", "t.tsv", "--variant-strand", "--strand-ratio", s, "--strand-min-depth", "3"]) for s in ("0.2", "2e-1", "1/5")]
    assert [(x.strand_ratio, x.strand_min_depth) for x in got] == [(Fraction(1, 5), 3)] * 3
    argv = cli._child_argv(got[0], True)                                                    # a --gpus child parses what the parent understood
    back = cli.GetArgs(argv)
    assert cli.strand_of(back) == cli.strand_of(got[0]) == dict(min_strand_depth=3, strand_ratio=Fraction(1, 5)) and back.variant_table == "t.tsv"


@pytest.mark.parametrize("extra", (["--strand-min-depth", "0"], ["--strand-min-depth", "x"], ["--strand-ratio", "1.5"], ["--strand-ratio", "1/3000001"], ["--strand-ratio=-1"]))
def test_bad_strand_thresholds_are_refused(tmp_path, capsys, extra):
    f = stub_files(tmp_path, ("x.bam", "r.fa", "f.gff", "o.csv.gz"))
    with pytest.raises(SystemExit) as e:
        cli.GetArgs(_base(f) + ["--variant-table", "t.tsv", "--variant-strand"] + extra)
    assert e.value.code == 2 and extra[0].split("=")[0] in capsys.readouterr().err


def test_refusals_exit_1_with_one_line_and_write_nothing(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    f = stub_files(tmp_path, ("x.bam", "r.fa", "f.gff", "o.csv.gz"))
    man = tmp_path / "m.tsv"
    man.write_text("%s\tS0\to0.fa\t-\t-\t-\tt0.tsv\n" % f["x.bam"])
    batch = ["--batch", str(man), "-ref", f["r.fa"], "-gff", f["f.gff"], "-cov", "30"]
    before = sorted(os.listdir(tmp_path))
    for argv, word in ((_base(f) + ["--variant-strand"], "--variant-strand needs --variant-table"),
                       (_base(f) + ["--variant-table", "t.tsv", "--strand-min-depth", "5"], "need --variant-strand"),
                       (_base(f) + ["--variant-table", "t.tsv", "--strand-ratio", "1/5"], "need --variant-strand"),
                       (_base(f) + ["--strand-ratio", "1/5"], "need --variant-strand"),
                       (batch + ["--variant-strand"], "--batch is refused"),
                       (batch + ["--variant-strand", "--gpus", "2"], "--batch is refused"),
                       (_base(f) + ["--variant-table", "t.tsv", "--variant-strand", "--index-override", f["o.csv.gz"]], "--index-override"),
                       (_base(f) + ["--variant-table", "t.tsv", "--variant-strand", "--index-override", f["o.csv.gz"], "--gpus", "2"], "--index-override")):
        for call in (cli.GetArgs, cli.main):
            with pytest.raises(SystemExit) as e:
                call(argv)
            out = capsys.readouterr().out
            assert e.value.code == 1 and word in out and out.count("\n") == 1 and out.endswith("Exiting...\n"), (argv, out)
    assert sorted(os.listdir(tmp_path)) == before
