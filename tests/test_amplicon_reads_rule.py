"""--amplicon-reads without a GPU: the yardstick (tests/amplicon_reads_yardstick.py) pinned on hand-written cases; the compiled table
and its lookup (csrc/amplicon_reads_rule.h + amplicon_reads_table.cpp) as a program of their own (tests/amplicon_reads_main.cpp), plain
and under AddressSanitizer + UBSan, and through tcmi_amplicon_reads_compile against the yardstick on seeded random schemes; the
scheme's zones (io/primers.amplicon_zones); the writer's text; the command line's argument handling, the --batch refusal included.
The kernel's tests are tests/test_amplicon_reads.py."""
import os

import numpy as np
import pytest

from tests import amplicon_reads_yardstick as ry
from tests import host_program
from tests import schemes as sch
from tests.cli_run import ROOT, base_args
from trueconsense_amd import TrueConsense as cli
from trueconsense_amd import _ffi, engine, indexing
from trueconsense_amd.io import primers as pb

NONE = -(1 << 31)


def lookup(table, p, q):
    """the header's lookup over the exported int32 [6, n] table, written out in Python -> (index or -1 none / -2 ambiguous, full)"""
    a, bmax, idx, b2, le, rs = table
    k = int(np.searchsorted(a, p, side="right"))
    if k == 0 or bmax[k - 1] <= q:
        return -1, False
    if k >= 2 and b2[k - 1] > q:
        return -2, False
    i = int(idx[k - 1])
    return i, bool(p < le[i] and q >= rs[i])


def test_yardstick_on_hand_written_cases():
    amps = [(100, 120, 180, 200), (150, 170, 230, 250), (100, 120, 180, 200), (400, 450, 430, 480)]    # 0 and 2 identical; 3: primers overlap
    for (p, q), want in (((100, 199), (-2, False)),         # inside the twins: ambiguous, never full
                         ((210, 249), (1, False)), ((150, 249), (1, True)), ((201, 249), (1, False)),   # q >= 200: behind the twins, amplicon 1 alone
                         ((160, 240), (1, True)), ((169, 230), (1, True)), ((170, 230), (1, False)), ((169, 229), (1, False)),
                         ((150, 250), (-1, False)), ((149, 200), (-1, False)),
                         ((400, 479), (3, True)), ((449, 449), (3, True)), ((450, 479), (3, False)), ((400, 429), (3, False)), ((480, 480), (-1, False))):
        assert ry.classify(p, q, amps, 0) == want, (p, q)
    assert ry.classify(95, 204, amps[:1], 5) == (0, True) and ry.classify(94, 204, amps[:1], 5) == (-1, False) and ry.classify(95, 205, amps[:1], 5) == (-1, False)
    assert ry.classify(-3, 10, [(0, 5, 8, 12)], 5) == (0, True)                             # a = -5: no clamp at 0
    rd = {"n_reads": 6, "flag": [0, 4, 16, 0, 0x400, 0], "pos": [10, 10, -1, 20, 30, 40], "tid": [0, 0, 0, 1, 0, 0],
          "cigar_off": [0, 3, 4, 5, 6, 7, 8], "cigar": [(5 << 4) | 4, (10 << 4) | 0, (2 << 4) | 2, 10 << 4, 10 << 4, 10 << 4, 10 << 4, (7 << 4) | 1]}
    assert ry.kept_columns(rd) == [(10, 21), (30, 39)]                                      # unmapped, pos < 0, another reference, span 0 are out
    assert ry.kept_columns(rd, shift=[100, 1000]) == [(110, 121), (1020, 1029), (130, 139)]
    assert ry.kept_columns(rd, read_filter=(0, 0, 0x400)) == [(10, 21)]
    assert ry.kept_columns(rd, read_filter=(30, 0, 0), mapq=[40, 40, 40, 40, 29, 40]) == [(10, 21)]
    got = ry.counts([(100, 199), (160, 240), (210, 249), (0, 5)], amps, 0)
    assert got.tolist() == [[0, 0], [2, 1], [0, 0], [0, 0], [1, 0], [1, 0]]
    assert ry.text("S", got[[1, 4, 5]], ["c"], ["a_1"], ["2"]) == ry.HEADER + "S\tc\ta_1\t2\t2\t1\nS\t*\t*ambiguous\t*\t1\t0\nS\t*\t*unassigned\t*\t1\t0\n"
    assert ry.HEADER == engine.AMPLICON_READS_HEADER


@pytest.mark.parametrize("sanitize", (False, True))
def test_rule_program(tmp_path, sanitize):
    """tests/amplicon_reads_main.cpp + csrc/amplicon_reads_table.cpp and nothing else, plain and with AddressSanitizer + UBSan, run as a
    program: every (p, q) of a small axis against its own brute force, every argument error"""
    out = host_program.build(["tests/amplicon_reads_main.cpp", "trueconsense_amd/csrc/amplicon_reads_table.cpp"], tmp_path / "amplicon_reads_main", sanitize)
    r = host_program.run(out)
    assert r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-4000:])
    assert int(r.stdout.split()[2]) > 1000000


def random_scheme(rng, n, axis):
    amps = []
    for i in range(n):
        fs = int(rng.integers(0, axis - 4))
        fe = fs + 2 + int(rng.integers(0, 150 if i % 4 == 0 else 60))
        if amps and i % 5 == 0:
            fs, fe = amps[-1][0], max(fe, amps[-1][0] + 2)                                  # the same start
        if amps and i % 7 == 0:
            fs, fe = amps[-1][0], amps[-1][3]                                               # identical extents
        amps.append((fs, fs + 1 + int(rng.integers(0, fe - fs)), fs + int(rng.integers(0, fe - fs)), fe))
    return amps


@pytest.mark.parametrize("slack", (0, 1, 5, 1000))
def test_compiled_table_equals_the_yardstick(slack):
    """tcmi_amplicon_reads_compile + the lookup on seeded random schemes: every p of an axis that starts in front of the widened starts,
    with near and far q"""
    rng = np.random.default_rng(7 + slack)
    for trial in range(10):
        n = (1, 2, 3, 30)[trial % 4] if trial < 8 else int(rng.integers(4, 60))
        amps = random_scheme(rng, n, 400)
        t = engine.amplicon_reads_compile(amps, slack)
        assert t.shape == (6, n) and t.dtype == np.int32 and (np.diff(t[0]) >= 0).all() and t[3, 0] == NONE
        assert sorted(t[0].tolist()) == sorted(fs - slack for fs, _, _, _ in amps) and t[4].tolist() == [a[1] for a in amps] and t[5].tolist() == [a[2] for a in amps]
        lo, hi = -slack - 3, 560 + slack
        for p in range(lo, hi, 1 if slack < 1000 else 7):
            for q in list(range(p, min(p + 12, hi))) + [p + 40, p + 100, p + 170, p + 2 * slack + 60]:
                assert lookup(t, p, q) == ry.classify(p, q, amps, slack), (trial, slack, p, q, amps)


def test_compile_argument_errors():
    ok = [(10, 20, 80, 100), (50, 90, 60, 170)]             # (the second: overlapping primers, legal)
    assert engine.amplicon_reads_compile(ok, 0).shape == (6, 2) and engine.amplicon_reads_compile(ok, 1000)[0].tolist() == [-990, -950]
    T = 1 << 29
    assert engine.amplicon_reads_compile([(T - 9, T - 5, T - 3, T)], 1000)[1].tolist() == [T + 1000]
    many = [(k, k + 5, k + 7, k + 9) for k in range(65537)]
    assert engine.amplicon_reads_compile(many[:65536], 0).shape == (6, 65536)
    for amps, slack, word in (([], 0, "1..65536"), (many, 0, "1..65536"), (ok, -1, "slack"), (ok, 1001, "slack"), ([(-1, 20, 80, 100)], 0, "2^29"),
                              ([(10, 20, 80, T + 1)], 0, "2^29"), ([(10, 20, -2, 100)], 0, "2^29"), ([(10, T + 5, 80, 100)], 0, "2^29"),
                              ([(10, 10, 80, 100)], 0, "fs < le"), ([(10, 20, 100, 100)], 0, "rs < fe"), ([(50, 60, 20, 30)], 0, "fs < fe"),
                              (ok + [(10, 5, 80, 100)], 0, "amplicon 2")):
        with pytest.raises(_ffi.TcmiError) as e:
            engine.amplicon_reads_compile(amps, slack)
        assert e.value.code == _ffi.E_ARG and word in str(e.value), (amps[:2], slack, str(e.value))
    fs, le, rs, fe = (np.array([v], np.int64) for v in ok[0])
    small = np.zeros(5, np.int32)
    msg = _ffi.C.create_string_buffer(200)
    assert _ffi.lib().tcmi_amplicon_reads_compile(1, _ffi.ptr(fs), _ffi.ptr(le), _ffi.ptr(rs), _ffi.ptr(fe), 0, _ffi.ptr(small), 5, msg, 200) == _ffi.E_ARG
    assert b"room" in msg.value and not small.any()
    assert _ffi.lib().tcmi_amplicon_reads_compile(1, _ffi.ptr(fs), None, _ffi.ptr(rs), _ffi.ptr(fe), 0, _ffi.ptr(small), 5, None, 0) == _ffi.E_ARG


def test_the_capacity_and_the_slot_are_the_headers():
    text = open(os.path.join(ROOT, "include", "tcmi.h")).read()
    assert "#define TCMI_AMPLICON_READS_LDS %d\n" % engine.AMPLICON_READS_LDS in text and "TCMI_K_AMPLICON_READS = %d " % _ffi.K_AMPLICON_READS in text
    assert engine.AMPLICON_READS_DTYPE.itemsize == 16 and '#define TCMI_AMPLICONS_HEADER' in text
    # eight workgroups' tables and counters fit the compute unit's 160 KiB of LDS
    assert 8 * (6 * 4 + 2 * 4) * (engine.AMPLICON_READS_LDS + 2) <= 160 * 1024


# ------------------------------------------------------------------------------------------------------------- the scheme's zones
def test_scheme_zones(tmp_path):
    rows = pb.read_scheme(sch.write_scheme_bed(tmp_path / "s.bed", sch.AMPLICON_SCHEME))
    zones = pb.amplicon_zones(rows)
    full = pb.amplicons(rows, "full")
    assert zones == [(10, 34, 400, 420), (320, 342, 690, 720), (640, 660, 1000, 1020), (5, 25, 300, 320), (50, 80, 70, 90), (100, 110, 150, 160)]
    assert [(z[0], z[3]) for z in zones] == [(m.start, m.end) for m in full]               # the same order as amplicons(), whatever the region
    assert [(z[1], max(z[1], z[2])) for z in zones] == [(m.start, m.end) for m in pb.amplicons(rows, "insert")]
    assert zones[4][1] > zones[4][2]                                                        # overlapping primers: legal for this rule
    assert engine.amplicon_reads_compile(zones[:3], 5).shape == (6, 3)
    assert [tuple(a) for a in pb.amplicons(rows, "insert")] == sch.AMPLICON_WANT["insert"]           # amplicons() is what it was
    with pytest.raises(pb.PrimerBedError):
        pb.amplicon_zones(rows[:1])                                                         # an amplicon without its RIGHT side: amplicons()' error


# ------------------------------------------------------------------------------------------------------------- the writer
def test_writer_text(tmp_path):
    rows = pb.read_scheme(sch.write_scheme_bed(tmp_path / "s.bed", sch.AMPLICON_SCHEME))
    amps = pb.amplicons(rows, "full")
    cnt = np.arange(16, dtype=np.int64).reshape(8, 2) * 3
    want = ry.text("S 1", cnt, [m.chrom for m in amps], [m.name for m in amps], [m.pool for m in amps])
    path = str(tmp_path / "r.tsv")
    cli.write_amplicon_reads(path, "S 1", cnt, amps)
    assert open(path).read() == want
    assert want.split("\n")[1] == "S 1\tchrA\tnCoV-2019_1\t1\t0\t3" and want.split("\n")[4] == "S 1\tchrB\tseg_LEFT_b\t1\t18\t21"
    assert want.endswith("S 1\t*\t*ambiguous\t*\t36\t0\nS 1\t*\t*unassigned\t*\t42\t0\n")
    rec = np.zeros(8, engine.AMPLICON_READS_DTYPE)          # Context.amplicon_reads' structured rows print alike
    rec["reads"], rec["full"] = cnt[:, 0], cnt[:, 1]
    assert cli.amplicon_reads_text("S 1", rec, amps) == want[len(ry.HEADER):]
    with pytest.raises(ValueError):
        cli.amplicon_reads_text("S", cnt[:7], amps)


# ------------------------------------------------------------------------------------------------------------- command line
def test_flags_and_their_errors(tmp_path, capsys):
    f = sch.scheme_files(tmp_path)
    base = base_args(f)
    a = cli.GetArgs(base)
    assert (a.amplicon_reads, a.amplicon_reads_slack) == (None, 5) and cli.amplicon_reads_of(a) is None
    a = cli.GetArgs(base + ["--amplicon-reads", "r.tsv", "--amplicon-scheme", f["s.bed"]])                 # the scheme alone now goes with --amplicon-reads
    assert (a.amplicon_reads, a.amplicon_reads_slack, a.amplicon_scheme, a.amplicon_table) == ("r.tsv", 5, f["s.bed"], None)
    a = cli.GetArgs(base + ["--amplicon-reads", "r.tsv", "--primers", f["p.bed"], "--amplicon-reads-slack", "0"])
    assert (a.amplicon_scheme, a.amplicon_reads_slack) == (f["p.bed"], 0)                                  # the scheme defaults to the file of --primers
    a = cli.GetArgs(base + ["--amplicon-reads", "r.tsv", "--amplicon-table", "t.tsv", "--amplicon-scheme", f["s.bed"], "--amplicon-reads-slack", "1000"])
    assert (a.amplicon_reads, a.amplicon_table, a.amplicon_reads_slack, a.amplicon_region) == ("r.tsv", "t.tsv", 1000, "insert")
    for extra, word in ((["--amplicon-reads", "r.tsv"], "--amplicon-reads needs the scheme's BED: --amplicon-scheme, or --primers."),
                        (["--amplicon-reads-slack", "3"], "--amplicon-reads-slack needs --amplicon-reads"),
                        (["--amplicon-reads", "r.tsv", "--amplicon-scheme", f["s.bed"], "--amplicon-reads-slack", "1001"], "0 to 1000"),
                        (["--amplicon-reads", "r.tsv", "--amplicon-scheme", f["s.bed"], "--amplicon-reads-slack", "-1"], "0 to 1000"),
                        (["--amplicon-reads", "r.tsv", "--amplicon-scheme", f["s.bed"], "--amplicon-region", "full"], "--amplicon-table"),
                        (["--amplicon-scheme", f["s.bed"]], "--amplicon-table")):
        with pytest.raises(SystemExit) as e:
            cli.GetArgs(base + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err, extra
    # the table's own error is worded as before
    with pytest.raises(SystemExit):
        cli.GetArgs(base + ["--amplicon-table", "t.tsv"])
    assert "--amplicon-table needs the scheme's BED: --amplicon-scheme, or --primers." in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.GetArgs(["-h"])
    text = capsys.readouterr().out
    assert text.index("--amplicon-region") < text.index("--amplicon-reads File") < text.index("--amplicon-reads-slack N")


def test_batch_is_refused(tmp_path, capsys):
    f = sch.scheme_files(tmp_path)
    man = tmp_path / "m.tsv"
    man.write_text("%s\tS0\to0.fa\n" % f["x.bam"])
    batch = ["--batch", str(man), "-ref", f["r.fa"], "-gff", f["f.gff"], "-cov", "12"]
    for gpus in ([], ["--gpus", "2"]):
        with pytest.raises(SystemExit) as e:
            cli.main(batch + gpus + ["--amplicon-reads", "r.tsv", "--amplicon-scheme", f["s.bed"]])
        err = capsys.readouterr().err
        assert e.value.code == 2 and "--amplicon-reads" in err and "--batch is refused" in err, err
    assert cli.GetArgs(batch + ["--amplicon-table", "t.tsv", "--amplicon-scheme", f["s.bed"]]).amplicon_reads is None     # the table goes on as before


def test_amplicons_of_the_reference_and_children(tmp_path, capsys):
    f = sch.scheme_files(tmp_path)
    base = base_args(f)
    (tmp_path / "r.fa").write_text(">chrA\nACGT\n")
    a = cli.GetArgs(base + ["--amplicon-reads", "r.tsv", "--amplicon-scheme", f["s.bed"], "--amplicon-reads-slack", "7"])
    a.input = None                                          # (x.bam is no BAM: the reference's name comes from -ref, as for --batch)
    amps, amps4, slack = cli.amplicon_reads_of(a)
    assert [m.name for m in amps] == ["nCoV-2019_%d" % k for k in (1, 2, 3)] and slack == 7
    assert amps4 == [(10, 34, 400, 420), (320, 342, 690, 720), (640, 660, 1000, 1020)]
    assert [(m.start, m.end) for m in amps] == [(z[0], z[3]) for z in amps4]
    # under a layout: every amplicon shifted by its contig's slot, in amplicons_of's order
    amps, amps4, _ = cli.amplicon_reads_of(a, (["chrB", "other", "chrA"], [0, -1, 5000]))
    assert [m.name for m in amps] == ["nCoV-2019_1", "nCoV-2019_2", "nCoV-2019_3", "seg_LEFT_b", "ov", "in"]
    assert amps4[0] == (5010, 5034, 5400, 5420) and amps4[4] == (50, 80, 70, 90)
    a.amplicon_table, a.amplicon_region = "t.tsv", "unique"
    assert [m.name for m, _ in cli.amplicons_of(a, (["chrB", "other", "chrA"], [0, -1, 5000]))] == [m.name for m in amps]
    a.amplicon_table = None
    with pytest.raises(SystemExit) as e:
        cli.amplicon_reads_of(a, (["x"], [0]))
    assert e.value.code == 1 and "--amplicon-reads: no amplicon" in capsys.readouterr().out
    # the children of --gpus N get both flags, and only when they are set
    a = cli.GetArgs(base + ["--amplicon-reads", "r.tsv", "--primers", f["s.bed"], "--amplicon-reads-slack", "7"])
    back = cli.GetArgs(cli._child_argv(a, True))
    assert (back.amplicon_reads, back.amplicon_reads_slack, back.amplicon_scheme, back.amplicon_table, back.primers) == ("r.tsv", 7, f["s.bed"], None, f["s.bed"])
    both = cli.GetArgs(base + ["--amplicon-reads", "r.tsv", "--amplicon-table", "t.tsv", "--amplicon-scheme", f["s.bed"], "--amplicon-region", "full"])
    back = cli.GetArgs(cli._child_argv(both, True))
    assert (back.amplicon_reads, back.amplicon_reads_slack, back.amplicon_table, back.amplicon_region) == ("r.tsv", 5, "t.tsv", "full")
    assert not any(x.startswith("--amplicon") for x in cli._child_argv(cli.GetArgs(base), True))


def test_files_that_leave_the_device_path_are_refused(monkeypatch):
    """a file the device decoder declines is refused on behalf of --amplicon-reads, as --primers refuses it: never counted another way"""
    class Ctx:
        read_rules = engine.ReadRules()

        def upload_bamfile(self, d, blocks):
            raise _ffi.TcmiError(_ffi.E_UNSUPPORTED, "the device packer declined")

    class Dev:
        def __init__(self, path):
            pass

        def close(self):
            pass
    monkeypatch.setattr(indexing, "DeviceBam", Dev)
    assert indexing.device_readset(Ctx(), "x.bam") is None                                  # without the flag: the host reader may take it
    with pytest.raises(_ffi.TcmiError) as e:
        indexing.device_readset(Ctx(), "x.bam", need="--amplicon-reads")
    assert e.value.code == _ffi.E_UNSUPPORTED and "--amplicon-reads needs the device path" in str(e.value) and "x.bam" in str(e.value)
