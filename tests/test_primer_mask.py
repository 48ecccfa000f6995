"""The amplicon primer mask (--primers; tcmi_ctx_set_primers): a kept read's tokens on columns in front of head_end (the largest end
over the '+' primers that hold its first column) or from tail_start on (the smallest start over the '-' primers that hold its last
column) are skipped exactly as tokens below the base-quality floor are; nothing else about the read changes.  The yardstick is
tests/primer_yardstick.py (committed oracle functions only).  Both device packers (one-sync, several-kernel), the drop variant of
the plane tally kernel and the stream-walking kernel of long reads are driven (on fuzzed inputs: tests/test_floor_mask_fuzz.py); the
flat-array entry points refuse."""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest

from oracle import c_oracle
from oracle import tc_oracle as orc
from tests import cli_run as cr
from tests import fuzz_reads as fz
from tests import host_program
from tests import primer_yardstick as py
from tests import read_specs as rsp
from tests.device_file import PACKERS, through
from tests.read_specs import L
from tests.schemes import PRIMER_SCHEME as SCHEME
from tests.schemes import compile_primers, write_primer_bed
from trueconsense_amd import TrueConsense as cli
from trueconsense_amd import _ffi, contigs, distributed, engine
from trueconsense_amd import synthetic as sy
from trueconsense_amd.io import bamwriter
from trueconsense_amd.io import primers as pbed


@functools.lru_cache(maxsize=None)
def mixed_yardstick(primed=True, q=0):
    """read_specs.mixed() under the scheme (or no table) and floor q -> (counts, masked reads, tokens kept, tokens)"""
    return py.counts(rsp.arrays(rsp.mixed()[2]), L, SCHEME if primed else (), q)


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_yardstick_without_primers_is_the_committed_oracle():
    rd = rsp.arrays(rsp.mixed()[2])
    got = mixed_yardstick(False)
    assert np.array_equal(got[0], c_oracle.tally(rd, c_oracle.extent(rd, L))) and got[1] == 0 and got[2] == got[3]
    assert np.array_equal(mixed_yardstick(False, 13)[0], rsp.oracle_counts(rd, 13, len(got[0])))      # pileup_columns(min_base_quality=13)


def test_yardstick_on_the_mixed_fixture():
    rd = rsp.arrays(rsp.mixed()[2])
    base, (want, n_masked, kept, total) = mixed_yardstick(False)[0], mixed_yardstick()
    assert len(SCHEME) == 12 and sum(orc.read_piles_up(rd, i) for i in range(int(rd["n_reads"]))) == 2960 and n_masked == 625
    assert round(100.0 * kept / total, 1) == 96.5
    assert (int(base[:, 5].sum()), int(want[:, 5].sum())) == (719, 716) and (int(base[:, 6].sum()), int(want[:, 6].sum())) == (825, 818)


def _find(seg, x, none):
    k = int(np.searchsorted(seg[:, 0], x, side="right")) - 1 if len(seg) else -1
    return int(seg[k, 2]) if k >= 0 and x < seg[k, 1] else none


@pytest.mark.parametrize("slack", (0, 5))
def test_compiled_table_equals_brute_force(slack):
    """random tables with overlapping, nested and alternative primers on a 600-column axis: every (p, q)"""
    rng = np.random.default_rng(100 + slack)
    for trial in range(12):
        prim = []
        for k in range(int(rng.integers(1, 30))):
            s = int(rng.integers(0, 560))
            if prim and k % 5 == 0:
                s = prim[-1][0]                                                 # an alternative primer: the same start
            prim.append((s, s + int(rng.integers(1, 120 if k % 4 == 0 else 30)), bool(rng.integers(0, 2))))
        rc, head, tail, msg = compile_primers(prim, slack)
        assert rc == 0, msg
        for seg in (head, tail):
            assert (seg[:, 0] < seg[:, 1]).all() and (seg[1:, 0] >= seg[:-1, 1]).all()
        for p in range(600):
            he = _find(head, p, p)
            for q in range(p, min(p + 40, 600)) if p % 7 else range(p, 600):
                assert (he, _find(tail, q, q + 1)) == py.read_mask(p, q, prim, slack), (trial, p, q)


def test_compile_argument_errors():
    ok = [(10, 34, False), (300, 324, True)]
    assert compile_primers(ok, 0)[0] == 0 and compile_primers([], 0)[0] == 0 and compile_primers(ok, 1000)[0] == 0
    for prim, slack, word in (([(-1, 5, False)], 0, "interval"), ([(10, 10, True)], 0, "interval"), ([(10, 9, False)], 0, "interval"),
                              ([(1 << 29, (1 << 29) + 5, False)], 0, "2^29"), ([(10, 1 << 29, True)], 0, "2^29"), ([(10, 34, 2)], 0, "strand"),
                              (ok, -1, "slack"), (ok, 1001, "slack"), ([(k, k + 5, False) for k in range(65537)], 0, "65536")):
        rc, _, _, msg = compile_primers(prim, slack, cap=4)
        assert rc == _ffi.E_ARG and word in msg, (prim[:2], slack, msg)
    assert compile_primers([(k * 10, k * 10 + 5, False) for k in range(8)], 0, cap=4)[0] == _ffi.E_ARG       # no room


def test_primer_table_program_under_sanitizers(tmp_path):
    """tests/primer_table_main.cpp + csrc/primer_table.cpp and nothing else, with AddressSanitizer + UBSan, run as a program"""
    out = host_program.build(["tests/primer_table_main.cpp", "trueconsense_amd/csrc/primer_table.cpp"], tmp_path / "primer_table_main")
    r = host_program.run(out)
    assert r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-4000:])


def test_bed_reader(tmp_path):
    path = write_primer_bed(str(tmp_path / "p.bed"), SCHEME, extra=["browser position ref:1-100", "other 5 29 x 1 +", "ref\t7\t9\tshort\t2\t-\tACGT"])
    rows = pbed.read_bed(path)
    assert len(rows) == 14 and rows[:2] == [("ref", 30, 54, False), ("ref", 406, 430, True)] and rows[12] == ("other", 5, 29, False)
    assert pbed.rows_for_reference(rows, "ref") == list(SCHEME) + [(7, 9, True)] and pbed.rows_for_reference(rows, "nope") == []
    assert pbed.rows_for_layout(rows, ["x", "other", "ref"], [0, 5000, -1]) == [(5005, 5029, False)]
    for bad, word in (("ref\t10\t34\tp\t1", "six columns"), ("ref\t10\t34\tp\t1\t.", "strand"), ("ref\tten\t34\tp\t1\t+", "integers"),
                      ("ref\t34\t34\tp\t1\t+", "interval"), ("ref\t-1\t34\tp\t1\t-", "interval"), ("ref\t10\t34\tp\t1\tplus", "strand")):
        p = str(tmp_path / "bad.bed")
        open(p, "w").write("# x\nref\t1\t5\tok\t1\t+\n\n" + bad + "\n")
        with pytest.raises(pbed.PrimerBedError) as e:
            pbed.read_bed(p)
        assert "bad.bed:4" in str(e.value) and word in str(e.value), (bad, str(e.value))


def test_cli_parses_primers_and_children_get_them_only_when_set(tmp_path, capsys):
    base = cr.base_args(cr.stub_files(tmp_path), "o.fa")
    a = cli.GetArgs(base)
    assert a.primers is None and a.primer_slack == 0 and cli.primers_of(a) is None
    a = cli.GetArgs(base + ["--primers", "p.bed", "--primer-slack", "5"])
    assert (a.primers, a.primer_slack) == ("p.bed", 5)
    for bad in ("1001", "-1", "x"):
        with pytest.raises(SystemExit) as e:
            cli.GetArgs(base + ["--primers", "p.bed", "--primer-slack", bad])
        assert e.value.code == 2, bad
    for single in (True, False):
        for args in ([], ["--primer-slack", "5"]):                             # (a slack alone sets no table)
            argv = cli._child_argv(cli.GetArgs(base + args), single)
            assert "--primers" not in argv and "--primer-slack" not in argv
        argv = cli._child_argv(cli.GetArgs(base + ["--primers", "p.bed", "--primer-slack", "5", "--min-baseq", "13"]), single)
        child = cli.GetArgs(argv if single else argv + ["-i", base[1], "-name", "S", "-o", "o.fa"])
        assert (child.primers, child.primer_slack, child.min_baseq) == ("p.bed", 5, 13)
    with pytest.raises(SystemExit):
        cli.GetArgs(["-h"])
    text = capsys.readouterr().out
    assert text.index("MI355X arguments (additive)") < text.index("--primers") < text.index("--primer-slack")


def test_cli_rows_of_the_bams_reference(tmp_path, capsys):
    """without --per-contig: the rows whose chrom is the BAM's reference name; none is an argument error, and so is a bad BED"""
    rd = rsp.arrays(rsp.mixed()[2][:20])
    bam = str(tmp_path / "A.bam")
    bamwriter.write_bam(bam, rd, ref_len=L)
    base = cr.base_args(cr.stub_files(tmp_path), "o.fa")
    base[1] = bam
    bed = write_primer_bed(str(tmp_path / "p.bed"), SCHEME, extra=["other\t5\t29\tx\t1\t+"])
    rows, slack = cli.primers_of(cli.GetArgs(base + ["--primers", bed, "--primer-slack", "3"]))
    assert rows == list(SCHEME) and slack == 3
    for text in ("other\t5\t29\tx\t1\t+\n", "ref\t5\t29\tx\t1\n"):
        open(bed, "w").write(text)
        with pytest.raises(SystemExit) as e:
            cli.primers_of(cli.GetArgs(base + ["--primers", bed]))
        assert e.value.code == 1 and "--primers" in capsys.readouterr().out


def test_header_declares_and_library_exports_the_symbols():
    text = open(os.path.join(cr.ROOT, "include", "tcmi.h")).read()
    assert re.search(r"int\s+tcmi_ctx_set_primers\(tcmi_ctx \*ctx, int32_t n, const int64_t \*start, const int64_t \*end, const int32_t \*reverse, int32_t slack\);", text)
    assert re.search(r"int\s+tcmi_readset_primers\(const tcmi_readset \*rs, int32_t \*n_primers, int64_t \*n_masked_reads\);", text)
    assert re.search(r"int\s+tcmi_primers_compile\(", text)
    assert "#define TCMI_ABI_VERSION 5" in text
    handle = C.CDLL(_ffi.LIB_PATH)
    for name in ("tcmi_ctx_set_primers", "tcmi_readset_primers", "tcmi_primers_compile"):
        assert getattr(handle, name) is not None
    assert handle.tcmi_abi_version() == 5


# ------------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    with engine.Context(0) as c:
        yield c


def check_file(ctx, path, rd, primers, q=0, want=None, f=(0, 0, 0), slack=0):
    """both packers equal the yardstick; the piled-up count and the extent are those of the same file without a table"""
    want = py.counts(rd, L, primers, q, slack) if want is None else want
    n_pos = len(want[0])
    for how in PACKERS:
        got, piled, end, n_prim, n_masked = through(ctx, how, path, primers, n_pos, q, f, slack)
        _, piled0, end0, n_prim0, n_masked0 = through(ctx, how, path, (), n_pos, q, f)
        bad = np.argwhere(got != want[0])
        assert len(bad) == 0, (how, q, bad[:8].tolist(), got[bad[:8, 0]].tolist(), want[0][bad[:8, 0]].tolist())
        assert (piled, end, n_prim, n_masked, n_prim0, n_masked0) == (piled0, end0, len(primers), want[1], 0, 0), how
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("split_records", (False, True))
def test_mixed_fixture_equals_the_yardstick(ctx, tmp_path, split_records):
    rd = rsp.arrays(rsp.mixed()[2])
    want, base = mixed_yardstick(), mixed_yardstick(False)
    assert 0.90 <= want[2] / want[3] <= 0.99                                    # (non-vacuity: conditions on the fixture)
    assert want[0][:, 5].sum() != base[0][:, 5].sum() and want[0][:, 6].sum() != base[0][:, 6].sum() and want[1] > 0
    path = str(tmp_path / "A.bam")
    bamwriter.write_bam(path, rd, ref_len=L, block=4096, split_records=split_records)
    check_file(ctx, path, rd, SCHEME, want=want)


# the table of the constructed edges: '+' primers of 31, 32 and 33 columns with '-' primers that meet / overlap their masks, a '+' and
# a '-' primer for the starts and ends around a primer's borders, two overlapping '+' primers, primers of the "wrong" strand, and
# primers over deletions, insertions and skips
EDGE_PRIMERS = [(100, 131, False), (131, 170, True), (400, 432, False), (420, 470, True), (700, 733, False),
                (1000, 1024, False), (1010, 1040, False), (1300, 1324, True), (1400, 1424, True), (1500, 1524, False),
                (1600, 1630, False), (1700, 1750, True)]


def edge_reads():
    rng = np.random.default_rng(78)
    out = []

    def add(pos, cig, qual=None, seq=None):
        out.append(rsp.mk(rng, pos, cig, qual, "e%03d" % len(out), seq))
    for start in (100, 400, 700):                                               # head masks that end 31, 32 and 33 columns in; reads shorter than
        for n in (1, 31, 32, 33, 64, 65, 150):                                  # their primer; with the '-' primers: masks that meet (100 + 64 columns)
            add(start, [(n, "M")])                                              # and overlap (400 + 32 .. 65 columns)
    for k in range(11):                                                         # 150-base masked reads: one of them straddles a block boundary
        add(101 + 3 * k, [(150, "M")])
    for p in (999, 1000, 1023, 1024, 1015, 1009, 1010, 1039, 1040):             # starts around a '+' primer's borders; two overlapping '+' primers
        add(p, [(50, "M")])
    for last in (1299, 1300, 1323, 1324):                                       # last columns around a '-' primer's borders
        add(last - 49, [(50, "M")])
    add(1405, [(50, "M")])                                                      # a '-' primer at a read's head: no effect
    add(1461, [(50, "M")])                                                      # a '+' primer at a read's tail (last column 1510): no effect
    add(1003, [(3, "S"), (40, "M")])                                            # soft clips do not count: p = POS
    add(1004, [(4, "S"), (40, "M"), (2, "S")])
    add(1005, [(5, "H"), (40, "M"), (3, "H")])
    add(1006, [(2, "H"), (3, "S"), (40, "M"), (1, "S"), (4, "H")])
    for p in (1620, 1610, 1608, 1606, 1600):                                    # 20M4D20M: the head mask's edge before, at, inside, at the end of, behind the D
        add(p, [(20, "M"), (4, "D"), (20, "M")])
    for p in (1690, 1680, 1678, 1676, 1670):                                    # ... and the tail mask's
        add(p, [(20, "M"), (4, "D"), (20, "M")])
    for p in (1609, 1608, 1610, 1600):                                          # "*+": the mask ends between the D's two columns (X goes, I stays) / behind them
        add(p, [(20, "M"), (2, "D"), (3, "I"), (20, "M")])
    add(1610, [(20, "M"), (2, "I"), (20, "M")])                                 # the mask ends on the column in front of the I: the I mark goes
    add(1611, [(20, "M"), (2, "I"), (20, "M")])                                 # ... one column earlier: it stays
    add(1689, [(20, "M"), (2, "I"), (20, "M")])                                 # a tail mask from the column behind the I's on (1709 stays) ...
    add(1681, [(20, "M"), (2, "I"), (20, "M")])                                 # ... and from that column on
    for p in (1612, 1607, 1602):
        add(p, [(20, "M"), (5, "N"), (20, "M")])
    add(1683, [(20, "M"), (5, "N"), (20, "M")])
    add(1002, [(50, "M")], seq="*")                                             # no floor: the columns outside the mask still count coverage
    add(1001, [(50, "M")], [30] * 20, seq="ACGTTGCAACGTACGTAGCT")               # SEQ shorter than the CIGAR
    add(1007, [(20, "M"), (2, "D"), (20, "M")], [30] * 25, seq="ACGTTGCAACGTACGTAGCTAACCG")   # ... and projected
    add(1614, [(30, "M"), (4, "D")], [30] * 30)                                 # the last reference-consuming op is a D
    add(1008, [(50, "M")], [255] * 50)                                          # no QUAL
    add(1690, [(45, "M"), (40, "D"), (45, "M")])                                # a deletion across pair boundaries, its tail masked from inside the D on
    out.sort(key=lambda r: r["pos"])
    return out


@pytest.mark.gpu
def test_constructed_edges(ctx, tmp_path):
    specs = edge_reads()
    rd = rsp.arrays(specs)
    want = py.counts(rd, L, EDGE_PRIMERS)
    base = py.counts(rd, L)
    assert (want[0][:, 0] < base[0][:, 0]).any() and want[0][:, 5].sum() < base[0][:, 5].sum() and want[0][:, 6].sum() < base[0][:, 6].sum()
    # SEQ "*" and the short SEQ: coverage outside the mask stays (a floor would have dropped it)
    assert want[0][1040:1050, 0].min() >= 2
    for tag, kw in (("whole", dict(block=4096)), ("split", dict(block=512, split_records=True))):
        path = str(tmp_path / (tag + ".bam"))
        bamwriter.write_bam(path, rd, ref_len=L, **kw)
        if tag == "split":                                                      # a masked 150-base read whose first pair (16 bytes of SEQ) straddles a BGZF block boundary
            d = engine.DeviceBam(path)
            starts = rsp.seq_starts(rd, d.inflated_bytes)
            d.close()
            assert any(s // 512 != (s + 15) // 512 for i, s in enumerate(starts)
                       if int(rd["l_qseq"][i]) == 150 and py.read_mask(int(rd["pos"][i]), int(rd["pos"][i]) + 149, EDGE_PRIMERS) != (int(rd["pos"][i]), int(rd["pos"][i]) + 150))
        check_file(ctx, path, rd, EDGE_PRIMERS, want=want)
    check_file(ctx, path, rd, EDGE_PRIMERS, slack=5)                            # (starts at start - 1 .. start - 5 are masked now)
    check_file(ctx, path, rd, EDGE_PRIMERS, q=13)                               # together with a floor: SEQ "*" is gone everywhere


def _long_specs():
    rng = np.random.default_rng(12)
    ref, _ = sy.make_reference(seed=3, L=L, cds=[])
    specs = rsp.background(rng, ref, 200)
    primers = list(SCHEME)
    for k, span in enumerate((520, 555, 599, 700, 700)):
        a, b, pos = int(rng.integers(100, 250)), 7, 50 + 90 * k
        specs.append(fz._read(rng, ref, pos, [(a, "M"), (3, "I"), (120, "M"), (b, "D"), (span - a - 120 - b, "M")], 16 * (k & 1), "long%d" % k))
        primers += [(pos - 4, pos + 20, False), (pos + span - 20, pos + span + 4, True)]
    # ... and one whose head mask reaches the column in front of its insertion, its tail mask into its deletion
    specs.append(fz._read(rng, ref, 600, [(30, "M"), (3, "I"), (500, "M"), (8, "D"), (40, "M")], 0, "long5"))
    primers += [(590, 630, False), (1134, 1180, True)]
    for r in specs:
        r["mapq"] = 60
    specs.sort(key=lambda r: r["pos"])
    return specs, primers


@pytest.mark.gpu
def test_long_reads(ctx, tmp_path):
    """spans of 520 - 700 that start in a '+' primer and end in a '-' primer, each with an insertion and a deletion
    (tally_stream_kernel walks what the packed set leaves out), among short reads"""
    specs, primers = _long_specs()
    rd = rsp.arrays(specs)
    path = str(tmp_path / "long.bam")
    bamwriter.write_bam(path, rd, ref_len=L, block=4096)
    want = check_file(ctx, path, rd, primers)
    check_file(ctx, path, rd, primers, q=13)
    base = py.counts(rd, L)
    assert want[0][:, 6].sum() < base[0][:, 6].sum() and want[0][:, 5].sum() < base[0][:, 5].sum() and want[1] >= 6
    for how in PACKERS:                                                         # the routing, as test_base_quality.test_long_reads asserts it
        ctx.set_option("one_sync", int(how == "one_sync"))
        ctx.set_primers(primers)
        d = engine.DeviceBam(path)
        try:
            rs = ctx.upload_bamfile(d)
            aligned, chunks, general = (C.c_int64(0) for _ in range(3))
            _ffi.check(_ffi.lib().tcmi_readset_sets(rs.handle, C.byref(aligned), C.byref(chunks), C.byref(general)))
            assert (rs.n_piled - aligned.value, general.value) == (6, 0) and aligned.value > 150, how
            ctx.profile(True)
            got = ctx.step(rs, len(want[0]), 0, True)[3]
            n_stream, n_planes = ctx.profile_get(_ffi.K_TALLY_GENERAL)[1], ctx.profile_get(_ffi.K_TALLY)[1]
            ctx.profile(False)
            assert (n_stream, n_planes) == (1, 1) and np.array_equal(got, want[0]), how
            rs.free()
        finally:
            d.close()
            ctx.profile(False)
            ctx.set_option("one_sync", 1)
            ctx.set_primers()


@pytest.mark.gpu
def test_together_with_the_floor_and_the_read_filter(ctx, tmp_path):
    f = (20, 0, 0x400)
    specs = rsp.mixed()[2]
    b, _ = rsp.kept(specs, f)
    rb = rsp.arrays(b)
    path = str(tmp_path / "A.bam")
    bamwriter.write_bam(path, rsp.arrays(specs), ref_len=L, block=4096)
    want = py.counts(rb, L, SCHEME, 13)                                         # the yardstick on the records that pass
    assert want[2] < mixed_yardstick()[2] and want[1] > 0
    check_file(ctx, path, rb, SCHEME, q=13, want=want, f=f)


@pytest.mark.gpu
def test_no_table_and_the_read_set_remembers(ctx, tmp_path):
    rd = rsp.arrays(rsp.mixed()[2])
    want, base = mixed_yardstick(), mixed_yardstick(False)
    n_pos = len(want[0])
    path = str(tmp_path / "A.bam")
    bamwriter.write_bam(path, rd, ref_len=L, block=4096)
    with engine.Context(0) as fresh:                                            # never set
        d = engine.DeviceBam(path)
        t0 = fresh.stat("one_sync_taken")
        rs = fresh.upload_bamfile(d)
        never = (fresh.step(rs, n_pos, 0, True)[3], rs.n_piled, rs.max_end, rs.primers, rs.primer_masked_reads, fresh.stat("one_sync_taken") - t0)
        rs.free()
        d.close()
    d = engine.DeviceBam(path)
    ctx.set_primers(SCHEME)
    ctx.set_primers([], 0)                                                      # n = 0 clears
    t0 = ctx.stat("one_sync_taken")
    rs = ctx.upload_bamfile(d)
    zero = (ctx.step(rs, n_pos, 0, True)[3], rs.n_piled, rs.max_end, rs.primers, rs.primer_masked_reads, ctx.stat("one_sync_taken") - t0)
    rs.free()
    assert np.array_equal(zero[0], never[0]) and zero[1:] == never[1:] and never[3:] == (0, 0, 1)
    assert np.array_equal(never[0], base[0])
    ctx.set_primers(SCHEME)
    rs = ctx.upload_bamfile(d)
    ctx.set_primers()                                                           # the context forgets, the read set does not
    assert (rs.primers, rs.primer_masked_reads) == (12, want[1])
    assert np.array_equal(ctx.step(rs, n_pos, 0, True)[3], want[0])
    ctx.set_primers([(0, 1999, False)])                                         # ... nor when the context's table is replaced
    rs2 = ctx.upload_bamfile(d)
    assert np.array_equal(ctx.step(rs, n_pos, 0, True)[3], want[0]) and rs2.primers == 1
    rs.free()
    rs2.free()
    ctx.set_primers()
    d.close()
    for bad, slack in (([(-1, 5, False)], 0), ([(5, 5, False)], 0), ([(5, 1 << 29, True)], 0), (SCHEME, 1001), (SCHEME, -1)):
        with pytest.raises(_ffi.TcmiError) as e:
            ctx.set_primers(bad, slack)
        assert e.value.code == _ffi.E_ARG
    assert ctx.primers == 0


@pytest.mark.gpu
def test_a_read_masked_from_end_to_end_and_long_read_counts(ctx, tmp_path):
    """one '+' primer over the whole axis: every read is piled up and adds nothing; the masked-read count takes the long reads along"""
    specs, _ = _long_specs()
    rd = rsp.arrays(specs)
    path = str(tmp_path / "long.bam")
    bamwriter.write_bam(path, rd, ref_len=L, block=4096)
    whole = [(0, L + 100, False)]
    want = py.counts(rd, L, whole)
    assert not want[0].any() and want[1] == sum(orc.read_piles_up(rd, i) for i in range(int(rd["n_reads"])))
    check_file(ctx, path, rd, whole, want=want)


@pytest.mark.gpu
def test_flat_array_entry_points_refuse(ctx):
    rd = rsp.arrays(rsp.mixed()[2][:300])
    n_pos = c_oracle.extent(rd, L)
    p = engine.Pipeline(device=0, slots=2, walkers=1)
    try:
        rs = p.ctx.upload(rd)
        ctx.set_primers(SCHEME)
        p.ctx.set_primers(SCHEME)
        for call in (lambda: ctx.upload(rd), lambda: ctx.tally(rd, L=n_pos), lambda: ctx.upload_batch([rd, rd], 2048),
                     lambda: p.run([rs], n_pos, 10, True)):
            with pytest.raises(_ffi.TcmiError) as e:
                call()
            assert e.value.code == _ffi.E_UNSUPPORTED and "--primers" in str(e.value)
        ctx.set_primers()
        p.ctx.set_primers()
        assert np.array_equal(ctx.tally(rd, L=n_pos), c_oracle.tally(rd, n_pos))   # the context is usable afterwards
        assert np.array_equal(p.ctx.step(rs, n_pos, 0, True)[3], c_oracle.tally(rd, n_pos))
        rs.free()
    finally:
        ctx.set_primers()
        p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("split_sub", (1, 2))
def test_one_file_over_three_ranks(tmp_path, split_sub):
    """split_ranks_in_turn(world = 3): the ranges in one piece, and as two sub-ranges each (the helper contexts take the table along).
    The sub-range file holds every record four times: its yardstick is four times the fixture's."""
    ref, orfs, specs = rsp.mixed()
    want = mixed_yardstick()[0]
    n_pos = len(want)
    times = 1 if split_sub == 1 else 4
    big = specs if times == 1 else sorted([dict(r, name="%s_%d" % (r["name"], k)) for k in range(4) for r in specs], key=lambda r: r["pos"])
    path = str(tmp_path / "A.bam")
    bamwriter.write_bam(path, rsp.arrays(big), ref_len=L, block=1024 if split_sub == 2 else 4096)
    tm = {}
    ta = distributed.split_ranks_in_turn(path, n_pos, cr.gff_rows(orfs), 10, 3, return_parts=True, rules=engine.ReadRules(primers=(SCHEME, 0)), split_sub=split_sub, timings=tm)
    tb = distributed.split_ranks_in_turn(path, n_pos, cr.gff_rows(orfs), 10, 1, return_parts=True, rules=engine.ReadRules(primers=(SCHEME, 0)), split_sub=1)
    assert np.array_equal(ta[1], times * want)
    assert ta[0] == tb[0] and np.array_equal(ta[1], tb[1]) and ta[2] == tb[2]
    assert (tm["split_sub_taken"] > 0) == (split_sub == 2)


CONTIG_PRIMERS = {"c0": [(40, 64, False), (300, 330, False), (700, 724, True), (1180, 1204, True)],
                  "c1": [(10, 40, False), (500, 524, False), (640, 664, True), (1100, 1130, True)]}


def _contig_bed(path):
    with open(path, "w") as fh:
        for name, prim in list(CONTIG_PRIMERS.items()) + [("elsewhere", [(5, 29, False)])]:
            for k, (s, e, rev) in enumerate(prim):
                fh.write("%s\t%d\t%d\t%s_%d\t1\t%s\n" % (name, s, e, name, k, "-" if rev else "+"))
    return path


@pytest.mark.gpu
def test_two_reference_contig_layout(ctx, tmp_path):
    """the several-kernel packer under a contig layout, a BED that names both contigs (and one the BAM lacks): every contig's slice
    of the matrix equals the yardstick on that contig's reads under that contig's rows"""
    recs, _, specs = rsp.two_contigs()
    refs = [("c0", 1500), ("c1", 1200)]
    names = [n for n, _ in refs]
    path = str(tmp_path / "A.bam")
    bamwriter.write_bam(path, rsp.arrays(specs), refs=refs, block=4096)
    shift, slot, axis = contigs.layout_for(recs, names, [ln for _, ln in refs])
    rows = pbed.rows_for_layout(pbed.read_bed(_contig_bed(str(tmp_path / "p.bed"))), names, shift)
    assert len(rows) == 8
    info = {}
    counts = contigs.step_contigs(ctx, path, shift, slot, axis, 10, True, names, want_counts=True, rules=engine.ReadRules(primers=(rows, 0)), info=info)[3]
    assert ctx.primers == 0
    seen = np.zeros(axis, bool)
    n_masked = 0
    for t, (name, ln) in enumerate(refs):
        rd = rsp.arrays([dict(r, tid=0) for r in specs if r["tid"] == t])
        want = py.counts(rd, ln, CONTIG_PRIMERS[name])
        n_pos = len(want[0])
        n_masked += want[1]
        assert want[1] > 10 and 0.8 < want[2] / want[3] < 0.995
        assert np.array_equal(counts[int(shift[t]):int(shift[t]) + n_pos], want[0]), t
        seen[int(shift[t]):int(shift[t]) + n_pos] = True
    assert not counts[~seen].any() and info["reads_primer_masked"] == n_masked


# ---- command line ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cli_single_sample_and_batch(tmp_path, monkeypatch):
    """-i with --primers: -doc is the yardstick's coverage column; FASTA, VCF and GFF equal the run WITHOUT the flag whose counts
    --index-override replaces, at every position, by the yardstick's matrix (downstream code only).  --batch equals -i."""
    monkeypatch.chdir(tmp_path)
    ref, orfs, specs = rsp.mixed()
    want, n_masked = mixed_yardstick()[:2]
    assert len(want) == L
    rd = rsp.arrays(specs)
    bamwriter.write_bam("A.bam", rd, ref_len=L, block=4096)
    bamwriter.write_bam("A2.bam", rd, ref_len=L, block=4096, split_records=True)
    common = cr.setup_cli(ref, orfs)
    write_primer_bed("p.bed", SCHEME, extra=["other\t5\t29\tx\t1\t+"])
    cr.write_override("o.csv.gz", want)
    out = lambda t: ["-o", t + ".fa", "-vcf", t + ".vcf", "-ogff", t + ".gff", "-doc", t + ".tsv"]
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + out("a") + ["--primers", "p.bed", "--stats", "a.json"])
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + out("b") + ["--index-override", "o.csv.gz", "--stats", "b.json"])
    assert cr.doc_column("a.tsv") == want[:, 0].tolist()
    assert cr.outputs("a") == cr.outputs("b")
    sa, sb = json.load(open("a.json")), json.load(open("b.json"))
    assert (sa["primers"], sa["reads_primer_masked"], sb["primers"], sb["reads_primer_masked"]) == (12, n_masked, 0, 0)
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + ["-o", "raw.fa", "-doc", "raw.tsv"])   # (the process's context is back at no table)
    assert cr.doc_column("raw.tsv") == mixed_yardstick(False)[0][:, 0].tolist()
    both = py.counts(rd, L, SCHEME, 13, 5)[0]                                   # with the floor and a slack
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + ["-o", "q.fa", "-doc", "q.tsv", "--primers", "p.bed", "--primer-slack", "5", "--min-baseq", "13"])
    assert cr.doc_column("q.tsv") == both[:, 0].tolist()
    with open("m.tsv.in", "w") as fh:
        for k, bam in enumerate(("A.bam", "A2.bam")):
            fh.write("\t".join([bam, "S"] + ["m%d.%s" % (k, e) for e in ("fa", "vcf", "gff", "tsv")]) + "\n")
    cr.run_cli(monkeypatch, ["--batch", "m.tsv.in"] + common + ["--primers", "p.bed", "--stats", "m.json"])
    for k in (0, 1):
        assert cr.outputs("m%d" % k) == cr.outputs("a"), k
    assert json.load(open("m.json"))["primers"] == 12


@pytest.mark.gpu
def test_cli_one_file_over_two_gpus(tmp_path, monkeypatch):
    """--gpus 2 (two ranks rehearsed on this one GPU, gloo for the exchange): -doc is the yardstick's coverage and every output equals
    the single-GPU run of the same file under the same table."""
    monkeypatch.chdir(tmp_path)
    ref, orfs, specs = rsp.mixed()
    want = mixed_yardstick()[0]
    bamwriter.write_bam("A.bam", rsp.arrays(specs), ref_len=L, block=4096, split_records=True)
    common = cr.setup_cli(ref, orfs)
    write_primer_bed("p.bed", SCHEME)
    for tag, extra in (("a", ["--gpus", "2"]), ("b", [])):
        cr.run_two_ranks(["-i", "A.bam", "-name", "S"] + common + cr.out_args(tag) + ["--primers", "p.bed"] + extra)
    assert cr.doc_column("a.tsv") == want[:, 0].tolist()
    assert cr.outputs("a") == cr.outputs("b")


@pytest.mark.gpu
def test_cli_per_contig(tmp_path, monkeypatch):
    """--per-contig: every BED row shifted by its contig's slot; per contig, -doc is the yardstick's coverage and the FASTA record
    equals the single run of that contig's reads alone under the same BED."""
    monkeypatch.chdir(tmp_path)
    recs, rows, specs = rsp.two_contigs()
    refs = [("c0", 1500), ("c1", 1200)]
    bamwriter.write_bam("A.bam", rsp.arrays(specs), refs=refs, block=4096)
    _contig_bed("p.bed")
    cr.setup_contigs(recs, rows)
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-ref", "r.fa", "-gff", "g.gff", "-cov", "10", "-name", "S", "-o", "a.fa", "-doc", "a.tsv",
                             "--per-contig", "--primers", "p.bed", "--stats", "a.json"])
    want_fa, want_tsv, n_masked = "", "", 0
    for t, (name, ln) in enumerate(refs):
        rd = rsp.arrays([dict(r, tid=0) for r in specs if r["tid"] == t])
        want = py.counts(rd, ln, CONTIG_PRIMERS[name])
        n_masked += want[1]
        bamwriter.write_bam("one%d.bam" % t, rd, refs=[(name, ln)], block=4096)
        open("r%d.fa" % t, "w").write(">%s\n%s\n" % recs[t])
        open("g%d.gff" % t, "w").write("##gff-version 3\n" + sy.gff_text(rows[t][1], seqid=name)[1])
        cr.run_cli(monkeypatch, ["-i", "one%d.bam" % t, "-ref", "r%d.fa" % t, "-gff", "g%d.gff" % t, "-cov", "10", "-name", "S_" + name,
                                 "-o", "one%d.fa" % t, "-doc", "one%d.tsv" % t, "--primers", "p.bed"])
        assert cr.doc_column("one%d.tsv" % t) == want[0][:, 0].tolist()
        want_fa += open("one%d.fa" % t).read()
        want_tsv += "".join("%s\t%s" % (name, line) for line in open("one%d.tsv" % t))
    assert open("a.fa").read() == want_fa and want_fa.count(">") == 2
    assert open("a.tsv").read() == want_tsv
    st = json.load(open("a.json"))
    assert (st["primers"], st["reads_primer_masked"]) == (8, n_masked)
