"""The amplicon table without a GPU: the yardstick (tests/amplicon_yardstick.py) pinned against hand-written cases, the scheme rule
(io/primers.py: read_scheme, amplicons) against it and against every error with its line, the product's argument checks
(csrc/intervals_rule.h) and row writer (csrc/amplicons_text.cpp) as a program of their own under AddressSanitizer + UBSan, and
the command line's argument handling with the part-file join of --batch --gpus.  The kernel's tests are tests/test_amplicon_table.py."""
import os
import struct

import numpy as np
import pytest

from tests import amplicon_yardstick as ay
from tests import host_program
from tests.cli_run import base_args as _base
from tests.schemes import AMPLICON_SCHEME as SCHEME
from tests.schemes import AMPLICON_WANT as WANT
from tests.schemes import scheme_files as _files
from tests.schemes import write_scheme_bed as write_bed
from trueconsense_amd import TrueConsense as cli
from trueconsense_amd import _ffi, engine
from trueconsense_amd.io import primers as pb


#            0  1  2  3  4  5  6  7  8  9
HAND_COV = [5, 3, 9, 3, 7, 0, 0, 8, 2, 2]
HAND = [((0, 5), 4, (27, 5, 3, 1, 5, 2, 0)),            # odd n: the middle; the minimum twice, its first position
        ((0, 4), 4, (20, 4, 3, 1, 3, 2, 0)),            # even n: the LOWER median (3, 3, 5, 9 -> 3)
        ((4, 8), 1, (15, 4, 0, 5, 0, 2, 0)),
        ((8, 12), 3, (4, 4, 0, 10, 0, 4, 0)),           # crosses L = 10: the columns behind it have depth 0
        ((12, 15), 0, (0, 3, 0, 12, 0, 0, 0)),          # wholly beyond L; min_depth 0: nothing is below
        ((12, 15), 1, (0, 3, 0, 12, 0, 3, 0)),
        ((7, 7), 9, ay.EMPTY), ((9, 10), 2, (2, 1, 2, 9, 2, 0, 0))]


def test_yardstick_on_hand_written_intervals():
    for (s, e), md, want in HAND:
        assert ay.record(HAND_COV, s, e, md) == want, (s, e, md)
    assert ay.record([-4, 7, -9, 2], 0, 4, 0) == (-4, 4, -9, 2, -4, 2, 0)                   # signed depths
    assert ay.record([-4, 7, -9, 2], 0, 6, 0)[4] == 0                                       # -9 -4 [0] 0 2 7
    rng = np.random.default_rng(2)
    for trial in range(300):            # the columns behind L counted, not listed: the same records as listing them
        cov = rng.integers(-3, 4, int(rng.integers(1, 12))).tolist()
        s = int(rng.integers(0, 14))
        e = s + int(rng.integers(0, 12))
        for md in (0, 1, 5):
            assert ay.record(cov, s, e, md) == ay.record_listed(cov, s, e, md), (cov, s, e, md)
    assert ay.record([4, 2], 1, 1 << 29, 3) == (2, (1 << 29) - 1, 0, 2, 0, (1 << 29) - 1, 0)
    recs = [HAND[0][2], ay.EMPTY, (1, 8, 0, 21, 0, 8, 0)]
    assert ay.text(recs, "S1", "ctg", ["a_1", "a_2", "b"], ["1", "2", "p"], [0, 7, 20]) == (
        "S1\tctg\ta_1\t1\t1\t5\t5\t5.40\t5\t3\t2\t2\n" "S1\tctg\ta_2\t2\t8\t7\t0\tNA\tNA\tNA\tNA\t0\n" "S1\tctg\tb\tp\t21\t28\t8\t0.12\t0\t0\t22\t8\n")
    assert ay.text(recs[2:], "S", "c", ["b"], ["p"], [20], pos_offset=15) == "S\tc\tb\tp\t6\t13\t8\t0.12\t0\t0\t7\t8\n"
    assert ay.HEADER == engine.AMPLICONS_HEADER


# ------------------------------------------------------------------------------------------------------------- the scheme rule


@pytest.mark.parametrize("region", ("insert", "unique", "full"))
def test_scheme_to_amplicons(tmp_path, region):
    bed = write_bed(tmp_path / "s.bed", SCHEME)
    rows = pb.read_scheme(bed)
    assert [(r.chrom, r.start, r.end, r.name, r.pool, "-" if r.reverse else "+") for r in rows] == SCHEME
    assert [(r.chrom, r.start, r.end, r.reverse) for r in rows] == pb.read_bed(bed)        # the same lines as read_bed
    assert rows[0].where == bed + ":4"
    got = [tuple(a) for a in pb.amplicons(rows, region)]
    assert got == WANT[region]
    assert got == ay.scheme(SCHEME, region)
    if region == "insert":
        assert [tuple(a) for a in pb.amplicons(rows)] == got                               # the default
        assert [tuple(a) for a in pb.amplicons(pb.read_scheme(write_bed(tmp_path / "b.bed", SCHEME, " ")))] == got


def test_unique_region_first_of_equal_longest():
    rows = [("c", 0, 10, "a_LEFT", "1", "+"), ("c", 100, 110, "a_RIGHT", "1", "-"),
            ("c", 40, 45, "b_LEFT", "2", "+"), ("c", 65, 70, "b_RIGHT", "2", "-")]         # a's insert [10, 100) minus [40, 70): 30 and 30
    srows = [pb.SchemeRow(c, s, e, n, p, st == "-", "f:%d" % (k + 1)) for k, (c, s, e, n, p, st) in enumerate(rows)]
    got = [tuple(a) for a in pb.amplicons(srows, "unique")]
    assert got == [("c", "a", "1", 10, 40), ("c", "b", "2", 45, 45)] == ay.scheme(rows, "unique")
    with pytest.raises(ValueError):
        pb.amplicons(srows, "inner")


@pytest.mark.parametrize("case", (
    (0, ("chrA", 10, 30, "nCoV-2019_1", "1", "+"), "no _LEFT or _RIGHT"),
    (0, ("chrA", 10, 30, "nCoV-2019_1_LEFT", "1", "-"), "LEFT primer on the '-' strand"),
    (1, ("chrA", 400, 420, "nCoV-2019_1_RIGHT", "1", "+"), "RIGHT primer on the '+' strand"),
    (1, ("chrZ", 400, 420, "nCoV-2019_1_RIGHT", "1", "-"), "lies on 'chrZ'"),
    (3, None, "has no RIGHT primer"),
    (2, None, "has no LEFT primer"),
))
def test_scheme_errors_name_file_and_line(tmp_path, case):
    at, row, words = case
    rows = list(SCHEME[:6])
    if row is None:                     # drop a side of amplicon 2: the error names the line of the amplicon's first row
        rows = rows[:at] + rows[at + 1:]
        rows = [r for r in rows if not r[3].lower().endswith("_alt")]
        line = 4 + next(k for k, r in enumerate(rows) if "_2_" in r[3])
    else:
        rows[at] = row
        line = 4 + at
    bed = write_bed(tmp_path / "e.bed", rows)
    with pytest.raises(pb.PrimerBedError) as e:
        pb.amplicons(pb.read_scheme(bed))
    assert str(e.value).startswith("%s:%d: " % (bed, line)) and words in str(e.value), str(e.value)


def test_layout_shifts_and_ignores(tmp_path):
    amps = pb.amplicons(pb.read_scheme(write_bed(tmp_path / "s.bed", SCHEME)))
    got = pb.amplicons_for_layout(amps, ["chrB", "other", "chrA"], [0, 5000, -1])           # chrA has no slot: ignored
    assert [(a.name, sh) for a, sh in got] == [("seg_LEFT_b", 0), ("ov", 0), ("in", 0)]
    got = pb.amplicons_for_layout(amps, ["chrB", "chrA"], [2000, 0])
    assert [a.chrom for a, _ in got] == ["chrA"] * 3 + ["chrB"] * 3 and [sh for _, sh in got] == [0] * 3 + [2000] * 3
    assert cli.amplicon_intervals(got)[3] == (2025, 2300)
    assert pb.amplicons_for_layout(amps, ["x"], [0]) == []


# ------------------------------------------------------------------------------------------------------------- the program


def run_program(prog, tmp_path, tag, cov, intervals, min_depth, sample, region, names, pools, pos_offset=0):
    inp, rec, txt = (str(tmp_path / (tag + ext)) for ext in (".in", ".rec", ".txt"))
    nm = b"".join(x.encode() + b"\0" for x in names)
    pl = b"".join(x.encode() + b"\0" for x in pools)
    with open(inp, "wb") as fh:
        fh.write(struct.pack("<8q", len(cov), len(intervals), min_depth, pos_offset, len(sample.encode()), len(region.encode()), len(nm), len(pl)))
        fh.write(sample.encode() + region.encode() + nm + pl)
        fh.write(np.array([s for s, _ in intervals], np.int64).tobytes() + np.array([e for _, e in intervals], np.int64).tobytes())
        fh.write(np.ascontiguousarray(cov, np.int32).tobytes())
    r = host_program.run(prog, inp, rec, txt)
    assert r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-4000:])
    return np.fromfile(rec, ay.DTYPE), open(txt).read()


def test_checks_rule_and_text_program_under_sanitizers(tmp_path):
    """tests/amplicons_main.cpp + csrc/intervals_rule.h + csrc/amplicons_text.cpp and nothing else, with AddressSanitizer + UBSan, run
    as a program: the argument checks' refusals (inside the program), its records equal the yardstick's, its text the yardstick's"""
    prog = host_program.build(["tests/amplicons_main.cpp", "trueconsense_amd/csrc/amplicons_text.cpp"], tmp_path / "amplicons_main")
    iv = [x[0] for x in HAND if x[1] == 1] + [(7, 7), (0, 10), (3, 5000)]
    names = ["amp_%d" % k for k in range(len(iv))]
    pools = [str(1 + k % 2) for k in range(len(iv))]
    got, text = run_program(prog, tmp_path, "hand", HAND_COV, iv, 1, "S", "ctg", names, pools)
    want = ay.records(HAND_COV, iv, 1)
    assert want[-1] == (sum(HAND_COV[3:]), 4997, 0, 5, 0, 4997 - 5, 0)
    assert got.tolist() == [tuple(w) for w in want]
    assert text == ay.text(want, "S", "ctg", names, pools, [s for s, _ in iv])
    assert "\t8\t7\t0\tNA\tNA\tNA\tNA\t0\n" in text                                          # the empty interval's row
    # %.2f ties (sums of n = 8: .125 -> .12, .375 -> .38 as the exact binary values round), large and negative depths, an offset
    rng = np.random.default_rng(5)
    cov = rng.integers(-50, 1 << 31, 3000, dtype=np.int64).astype(np.int32)
    cov[100:108] = [1, 0, 0, 0, 0, 0, 0, 0]
    cov[108:116] = [3, 0, 0, 0, 0, 0, 0, 0]
    cov[200:1400] = (1 << 31) - 1
    cov[2000:2100] &= 0xFF
    cov[2100:2200] &= ~0xFFFFFF
    iv = [(100, 108), (108, 116), (200, 1400), (150, 1500), (2000, 2100), (2100, 2200), (2999, 3001), (3000, 3000), (1000, 2999), (1000, 3000)]
    names = ["x%d" % k for k in range(len(iv))]
    for md in (0, 1, (1 << 31) - 1):
        got, text = run_program(prog, tmp_path, "big%d" % (md % 7), cov, iv, md, "sample 1", "MN908947.3", names, names, pos_offset=100)
        want = ay.records(cov, iv, md)
        assert np.array_equal(got, ay.as_array(want)), md
        assert text == ay.text(want, "sample 1", "MN908947.3", names, names, [s for s, _ in iv], 100), md
    assert want[2][0] == 1200 * ((1 << 31) - 1) > 1 << 32 and "\t0.12\t" in text and "\t0.38\t" in text


def test_text_writer_through_the_abi():
    """tcmi_amplicons_text as Python calls it (no GPU): rows, an offset, the empty table and its refusals"""
    recs = [x[2] for x in HAND if x[1] in (1, 9)]
    starts = [x[0][0] for x in HAND if x[1] in (1, 9)]
    names, pools = ["a", "b", "c"], ["1", "2", "1"]
    assert engine.amplicons_text(ay.as_array(recs), "S", "ctg", names, pools, starts) == ay.text(recs, "S", "ctg", names, pools, starts)
    assert engine.amplicons_text(ay.as_array(recs), "S", "ctg", names, pools, starts, 4) == ay.text(recs, "S", "ctg", names, pools, starts, 4)
    assert engine.amplicons_text(ay.as_array([]), "S", "ctg", [], [], []) == ""
    with pytest.raises(_ffi.TcmiError) as e:
        engine.amplicons_text(ay.as_array(recs), "S", "ctg", names, pools, starts, 5)      # a start in front of the offset
    assert e.value.code == _ffi.E_ARG
    with pytest.raises(_ffi.TcmiError):
        engine.amplicons_text(ay.as_array([(3, 3, 1, 99, 1, 0, 0)]), "S", "ctg", ["a"], ["1"], [0])
    with pytest.raises(ValueError):
        engine.amplicons_text(ay.as_array(recs), "S", "ctg", names[:2], pools, starts)
    assert (_ffi.K_INTERVALS, engine.INTERVAL_DTYPE.itemsize, engine.INTERVAL_DTYPE) == (11, 32, ay.DTYPE)


# ------------------------------------------------------------------------------------------------------------- command line


def test_the_four_flags(tmp_path, capsys):
    f = _files(tmp_path)
    a = cli.GetArgs(_base(f))
    assert (a.amplicon_table, a.amplicon_scheme, a.amplicon_region) == (None, None, "insert") and cli.amplicons_of(a) is None
    a = cli.GetArgs(_base(f) + ["--amplicon-table", "t.tsv", "--amplicon-scheme", f["s.bed"]])
    assert (a.amplicon_table, a.amplicon_scheme, a.amplicon_region, a.primers) == ("t.tsv", f["s.bed"], "insert", None)
    a = cli.GetArgs(_base(f) + ["--amplicon-table", "t.tsv", "--primers", f["p.bed"], "--amplicon-region", "unique"])
    assert (a.amplicon_scheme, a.amplicon_region) == (f["p.bed"], "unique")                 # the scheme defaults to the file of --primers
    a = cli.GetArgs(_base(f) + ["--amplicon-table", "t.tsv", "--primers", f["p.bed"], "--amplicon-scheme", f["s.bed"], "--amplicon-region", "full"])
    assert (a.amplicon_scheme, a.primers, a.amplicon_region) == (f["s.bed"], f["p.bed"], "full")
    for extra, word in ((["--amplicon-table", "t.tsv"], "--amplicon-scheme"), (["--amplicon-scheme", f["s.bed"]], "--amplicon-table"),
                        (["--amplicon-region", "full"], "--amplicon-table"),
                        (["--amplicon-table", "t.tsv", "--amplicon-scheme", f["s.bed"], "--amplicon-region", "inner"], "--amplicon-region")):
        with pytest.raises(SystemExit) as e:
            cli.GetArgs(_base(f) + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err, extra
    neg = [x if x != "30" else "-1" for x in _base(f)]
    with pytest.raises(SystemExit) as e:
        cli.GetArgs(neg + ["--amplicon-table", "t.tsv", "--amplicon-scheme", f["s.bed"]])
    assert e.value.code == 2 and "-cov" in capsys.readouterr().err
    assert cli.GetArgs(neg).coverage_level == -1                                            # without the table: as before


def test_amplicons_of_the_reference_and_children(tmp_path, capsys):
    f = _files(tmp_path)
    man = tmp_path / "m.tsv"
    man.write_text("".join("%s\tS%d\to%d.fa\n" % (f["x.bam"], k, k) for k in range(5)))
    batch = ["--batch", str(man), "-ref", f["r.fa"], "-gff", f["f.gff"], "-cov", "12"]
    a = cli.GetArgs(batch + ["--amplicon-table", "t.tsv", "--amplicon-scheme", f["s.bed"], "--amplicon-region", "full"])
    amps = cli.amplicons_of(a)                          # --batch: the amplicons on the reference -ref names
    assert [(m.name, sh) for m, sh in amps] == [("nCoV-2019_%d" % k, 0) for k in (1, 2, 3)]
    assert cli.amplicon_intervals(amps) == [(10, 420), (320, 720), (640, 1020)]
    argv = cli._child_argv(a, False)
    assert "--amplicon-table" not in argv and argv[argv.index("--amplicon-scheme") + 1] == f["s.bed"] and argv[argv.index("--amplicon-region") + 1] == "full"
    single = cli.GetArgs(_base(f) + ["--amplicon-table", "t.tsv", "--primers", f["s.bed"]])
    argv = cli._child_argv(single, True)
    back = cli.GetArgs(argv)
    assert (back.amplicon_table, back.amplicon_scheme, back.amplicon_region, back.primers) == ("t.tsv", f["s.bed"], "insert", f["s.bed"])
    assert not any(x.startswith("--amplicon") for x in cli._child_argv(cli.GetArgs(_base(f)), True))
    (tmp_path / "o.fa").write_text(">elsewhere\nACGT\n")
    b = cli.GetArgs(["--batch", str(man), "-ref", str(tmp_path / "o.fa"), "-gff", f["f.gff"], "-cov", "30", "--amplicon-table", "t.tsv", "--amplicon-scheme", f["s.bed"]])
    with pytest.raises(SystemExit) as e:
        cli.amplicons_of(b)
    assert e.value.code == 1 and 'no amplicon' in capsys.readouterr().out
    bad = write_bed(tmp_path / "bad.bed", [SCHEME[0]])
    c = cli.GetArgs(batch + ["--amplicon-table", "t.tsv", "--amplicon-scheme", bad])
    with pytest.raises(SystemExit) as e:
        cli.amplicons_of(c)
    assert e.value.code == 1 and bad + ":4" in capsys.readouterr().out


def test_batch_over_gpus_joins_the_parts_in_manifest_order(tmp_path, monkeypatch):
    """`--batch m.tsv --gpus 2 --amplicon-table FILE`: every child writes FILE.partK (its samples k, k + 2, ...); once all have exited
    with status 0 the parent writes FILE in manifest order and removes the parts; a failed child: no FILE, the parts stay"""
    f = _files(tmp_path)
    man = tmp_path / "m.tsv"
    man.write_text("".join("%s\tS%d\to%d.fa\n" % (f["x.bam"], k, k) for k in range(5)))
    table = str(tmp_path / "amp.tsv")
    status = [0]
    seen = []

    def fake_spawn(cmds, envs):
        for cmd in cmds:
            child = cli.GetArgs(cmd[3:])
            rows = cli.read_manifest(child)
            amps = cli.amplicons_of(child)
            seen.append((child.amplicon_table, [r[1] for r in rows]))
            recs = [(100 * int(r[1][1:]) + k, 1, 0, m.start, 0, 0, 0) for r in rows for k, (m, _) in enumerate(amps)]
            cli.write_amplicon_table(child.amplicon_table, [(r[1], ay.as_array(recs[i * len(amps):(i + 1) * len(amps)])) for i, r in enumerate(rows)], amps)
        return status[0]
    monkeypatch.setattr("trueconsense_amd.launch._spawn", fake_spawn)
    argv = ["--batch", str(man), "--gpus", "2", "-ref", f["r.fa"], "-gff", f["f.gff"], "-cov", "30", "--amplicon-table", table, "--amplicon-scheme", f["s.bed"]]
    cli.main(argv)
    assert seen == [(table + ".part0", ["S0", "S2", "S4"]), (table + ".part1", ["S1", "S3"])]
    lines = open(table).read().split("\n")
    assert lines[0] + "\n" == ay.HEADER and lines[-1] == "" and len(lines) == 1 + 5 * 3 + 1
    assert [ln.split("\t")[0] for ln in lines[1:-1]] == [s for k in range(5) for s in ["S%d" % k] * 3]
    assert [ln.split("\t")[7] for ln in lines[1:-1]] == ["%d.00" % (100 * k + j) for k in range(5) for j in range(3)]      # MEAN = sum / 1
    assert not os.path.exists(table + ".part0") and not os.path.exists(table + ".part1")
    os.remove(table)
    status[0] = 3
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 3 and not os.path.exists(table) and os.path.exists(table + ".part0")
