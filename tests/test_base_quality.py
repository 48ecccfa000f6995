"""The base-quality floor (--min-baseq; tcmi_ctx_set_min_base_quality): a pileup token — one read on one column — whose quality is
below Q is skipped: nothing for coverage, A/T/C/G, X or I; nothing else about the read changes.  The yardstick everywhere is the
committed oracle, tally_tokens(pileup_columns(reads, min_base_quality=Q)[c]) per column, zero-padded to c_oracle.extent(reads, L):
a matched base is tested with its own QUAL byte, a D / N token with that of the next query base, a query index at or beyond l_seq
has quality 0, a record without QUAL (0xFF) is never skipped.  Both device packers (one-sync, several-kernel), the drop variant of
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
from tests import cli_run as cr
from tests import fuzz_reads as fz
from tests import read_specs as rsp
from tests.device_file import PACKERS, uploaded
from tests.read_specs import L, mk, oracle_counts, seq_starts, two_contigs
from trueconsense_amd import TrueConsense as cli
from trueconsense_amd import _ffi, contigs, distributed, engine
from trueconsense_amd import synthetic as sy
from trueconsense_amd.io import bamwriter


@functools.lru_cache(maxsize=None)
def mixed_oracle(q):
    """read_specs.mixed() (qualities clustered at 12 / 13, reads without QUAL, insertions, deletions, clips) under floor q"""
    rd = rsp.arrays(rsp.mixed()[2])
    n_pos = c_oracle.extent(rd, L)
    return oracle_counts(rd, q, n_pos), n_pos


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_cli_parses_min_baseq(tmp_path):
    base = cr.base_args(cr.stub_files(tmp_path), "o.fa")
    assert cli.GetArgs(base).min_baseq == 0
    for text, v in (("0", 0), ("13", 13), ("255", 255)):
        assert cli.GetArgs(base + ["--min-baseq", text]).min_baseq == v
    for bad in ("256", "-1", "x"):
        with pytest.raises(SystemExit) as e:
            cli.GetArgs(base + ["--min-baseq", bad])
        assert e.value.code == 2, bad


def test_gpus_children_get_min_baseq_only_when_it_is_set(tmp_path):
    base = cr.base_args(cr.stub_files(tmp_path), "o.fa")
    for single in (True, False):
        assert "--min-baseq" not in cli._child_argv(cli.GetArgs(base), single)
        assert "--min-baseq" not in cli._child_argv(cli.GetArgs(base + ["--min-baseq", "0"]), single)
        argv = cli._child_argv(cli.GetArgs(base + ["--min-baseq", "13", "--min-mapq", "20"]), single)
        child = cli.GetArgs(argv if single else argv + ["-i", base[1], "-name", "S", "-o", "o.fa"])
        assert child.min_baseq == 13 and cli.read_filter_of(child) == (20, 0, 0)


def test_header_declares_and_library_exports_the_two_symbols():
    text = open(os.path.join(cr.ROOT, "include", "tcmi.h")).read()
    assert re.search(r"int\s+tcmi_ctx_set_min_base_quality\(tcmi_ctx \*ctx, int32_t q\);", text)
    assert re.search(r"int\s+tcmi_readset_min_base_quality\(const tcmi_readset \*rs, int32_t \*q\);", text)
    assert "#define TCMI_ABI_VERSION 5" in text
    handle = C.CDLL(_ffi.LIB_PATH)
    for name in ("tcmi_ctx_set_min_base_quality", "tcmi_readset_min_base_quality"):
        assert getattr(handle, name) is not None


# ------------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    with engine.Context(0) as c:
        yield c


def through(ctx, how, path, q, n_pos, f=(0, 0, 0)):
    """the file under floor q on one packer -> (counts, n_piled, max_end, the read set's floor)"""
    with uploaded(ctx, path, q=q, f=f, how=how) as rs:
        return ctx.step(rs, n_pos, 0, True)[3], rs.n_piled, rs.max_end, rs.min_base_quality


def check_file(ctx, path, rd, q, want=None, f=(0, 0, 0)):
    """both packers at floor q equal the oracle; the piled-up count and the extent are those of the same file without a floor"""
    n_pos = c_oracle.extent(rd, L)
    want = oracle_counts(rd, q, n_pos) if want is None else want
    for how in PACKERS:
        got, piled, end, rs_q = through(ctx, how, path, q, n_pos, f)
        _, piled0, end0, rs_q0 = through(ctx, how, path, 0, n_pos, f)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (how, q, bad[:8].tolist(), got[bad[:8, 0]].tolist(), want[bad[:8, 0]].tolist())
        assert (piled, end, rs_q, rs_q0) == (piled0, end0, q, 0), how
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("q", (1, 13, 20, 42, 255))
@pytest.mark.parametrize("split_records", (False, True))
def test_counts_equal_the_oracle(ctx, tmp_path, q, split_records):
    specs = rsp.mixed()[2]
    rd = rsp.arrays(specs)
    want, n_pos = mixed_oracle(q)
    base, _ = mixed_oracle(0)
    share = want[:, 0].sum() / base[:, 0].sum()
    assert 0.02 <= share <= 0.99, share                                         # (non-vacuity: a condition on the fixture)
    assert want[:, 5].sum() != base[:, 5].sum() and want[:, 6].sum() != base[:, 6].sum()
    path = str(tmp_path / "A.bam")
    bamwriter.write_bam(path, rd, ref_len=L, block=4096, split_records=split_records)
    check_file(ctx, path, rd, q, want)


def _one_low(n, at, low=12):
    q = [30] * n
    q[at] = low
    return q


def edge_reads():
    rng = np.random.default_rng(77)
    out, pos = [], [10]

    def add(cig, qual=None, seq=None, step=23):
        out.append(mk(rng, pos[0], cig, qual, "e%d" % len(out), seq))
        pos[0] += step
    for n in (1, 31, 32, 33, 63, 64, 65, 150):                                  # lengths around the 32-base pair
        add([(n, "M")])
    add([(3, "S"), (40, "M")])                                                  # soft clips in front: odd, even
    add([(4, "S"), (40, "M"), (2, "S")])
    for at in (0, 31, 32, 69):                                                  # a single Q12 base
        add([(70, "M")], _one_low(70, at))
    add([(50, "M")], [12] * 50)
    add([(50, "M")], [255] * 50)                                                # no QUAL: never skipped
    add([(50, "M")], seq="*")
    add([(50, "M")], [30] * 20, seq="ACGTTGCAACGTACGTAGCT")                     # SEQ shorter than the CIGAR
    add([(20, "M"), (2, "D"), (20, "M")], [30] * 25, seq="ACGTTGCAACGTACGTAGCTAACCG")   # ... and projected
    for low in (12, 13):
        add([(20, "M"), (3, "D"), (20, "M")], _one_low(40, 20, low))            # the base behind the D
        add([(20, "M"), (2, "I"), (20, "M")], _one_low(42, 19, low))            # the base in front of the I
        add([(20, "M"), (2, "D"), (3, "I"), (20, "M")], _one_low(43, 20, low))  # "*+": the D's quality is the first inserted base's
        add([(20, "M"), (5, "N"), (20, "M")], _one_low(40, 20, low))
        add([(30, "M"), (4, "D"), (5, "S")], _one_low(35, 30, low))             # the last reference-consuming op is a D (a clipped base behind it)
    add([(30, "M"), (4, "D")], [30] * 30)                                       # ... with no base behind it: quality 0
    add([(5, "H"), (40, "M"), (3, "H")])
    add([(2, "H"), (3, "S"), (40, "M"), (1, "S"), (4, "H")])
    add([(45, "M"), (40, "D"), (45, "M")])                                      # a deletion across a pair boundary
    for _ in range(12):                                                         # 150-base reads: one of them straddles a block boundary
        add([(150, "M")], step=7)
    return out


@pytest.mark.gpu
def test_constructed_edges(ctx, tmp_path):
    specs = edge_reads()
    rd = rsp.arrays(specs)
    want = None
    for tag, kw in (("whole", dict(block=4096)), ("split", dict(block=512, split_records=True))):
        path = str(tmp_path / (tag + ".bam"))
        bamwriter.write_bam(path, rd, ref_len=L, **kw)
        if tag == "split":                                                      # a 150-base read whose first pair (16 bytes of SEQ) straddles a BGZF block boundary
            d = engine.DeviceBam(path)
            starts = seq_starts(rd, d.inflated_bytes)
            d.close()
            assert any(s // 512 != (s + 15) // 512 for i, s in enumerate(starts) if int(rd["l_qseq"][i]) == 150)
        want = check_file(ctx, path, rd, 13, want)
    base = oracle_counts(rd, 0, len(want))
    assert (want[:, 0] < base[:, 0]).any() and want[:, 5].sum() < base[:, 5].sum() and want[:, 6].sum() < base[:, 6].sum()


@pytest.mark.gpu
def test_depth_of_three_thousand(ctx, tmp_path):
    """3 000 copies of one read on one position (the fourth counter's carry ripple, several stages, more than one chunk): one base
    Q12, its neighbour Q13; a few reads at neighbouring offsets around them."""
    rng = np.random.default_rng(5)
    one = mk(rng, 500, [(150, "M")], [30] * 70 + [12, 13] + [30] * 78, "deep")
    specs = [mk(rng, 470 + 4 * k, [(int(rng.integers(40, 151)), "M")], None, "n%d" % k) for k in range(7)]
    specs += [dict(one, name="deep%d" % k) for k in range(3000)]
    specs += [mk(rng, 501 + 5 * k, [(int(rng.integers(40, 151)), "M")], None, "m%d" % k) for k in range(7)]
    specs.sort(key=lambda r: r["pos"])
    rd = rsp.arrays(specs)
    path = str(tmp_path / "deep.bam")
    bamwriter.write_bam(path, rd, ref_len=L, block=0xFF00)
    want = check_file(ctx, path, rd, 13)
    assert want[569, 0] >= 3000 and want[570, 0] < 20 and want[571, 0] >= 3000


@pytest.mark.gpu
def test_long_reads(ctx, tmp_path):
    """spans of 520 - 599 and of 700 positions, each with an insertion and a deletion, random qualities (tally_stream_kernel walks
    what the packed set leaves out), among short reads"""
    rng = np.random.default_rng(11)
    ref, _ = sy.make_reference(seed=3, L=L, cds=[])
    specs = rsp.background(rng, ref, 200)
    for k, span in enumerate((520, 555, 599, 700, 700)):
        a, b = int(rng.integers(100, 250)), 7
        specs.append(fz._read(rng, ref, 50 + 90 * k, [(a, "M"), (3, "I"), (120, "M"), (b, "D"), (span - a - 120 - b, "M")], 16 * (k & 1), "long%d" % k))
    for r in specs:
        r["mapq"] = 60
    specs.sort(key=lambda r: r["pos"])
    rd = rsp.arrays(specs)
    path = str(tmp_path / "long.bam")
    bamwriter.write_bam(path, rd, ref_len=L, block=4096)
    want = check_file(ctx, path, rd, 13)
    assert 0.3 < want[:, 0].sum() / oracle_counts(rd, 0, len(want))[:, 0].sum() < 0.95
    # the routing: from a device-decoded stream every one of the five (no cutting into pieces there: that is the host packer's) is
    # left out of the packed set and walked by tally_stream_kernel — one launch in the general-tally bracket per step
    for how in PACKERS:
        ctx.set_option("one_sync", int(how == "one_sync"))
        ctx.set_min_base_quality(13)
        d = engine.DeviceBam(path)
        try:
            rs = ctx.upload_bamfile(d)
            aligned, chunks, general = (C.c_int64(0) for _ in range(3))
            _ffi.check(_ffi.lib().tcmi_readset_sets(rs.handle, C.byref(aligned), C.byref(chunks), C.byref(general)))
            assert (rs.n_piled - aligned.value, general.value) == (5, 0) and aligned.value > 150, how
            ctx.profile(True)
            got = ctx.step(rs, len(want), 0, True)[3]
            n_stream, n_planes = ctx.profile_get(_ffi.K_TALLY_GENERAL)[1], ctx.profile_get(_ffi.K_TALLY)[1]
            ctx.profile(False)
            assert (n_stream, n_planes) == (1, 1) and np.array_equal(got, want), how
            rs.free()
        finally:
            d.close()
            ctx.profile(False)
            ctx.set_option("one_sync", 1)
            ctx.set_min_base_quality()


@pytest.mark.gpu
def test_floor_zero_and_the_read_set_remembers(ctx, tmp_path):
    rd = rsp.arrays(rsp.mixed()[2])
    want13, n_pos = mixed_oracle(13)
    path = str(tmp_path / "A.bam")
    bamwriter.write_bam(path, rd, ref_len=L, block=4096)
    with engine.Context(0) as fresh:                                            # never set
        d = engine.DeviceBam(path)
        t0 = fresh.stat("one_sync_taken")
        rs = fresh.upload_bamfile(d)
        never = (fresh.step(rs, n_pos, 0, True)[3], rs.n_piled, rs.max_end, rs.min_base_quality, fresh.stat("one_sync_taken") - t0)
        rs.free()
        d.close()
    d = engine.DeviceBam(path)
    ctx.set_min_base_quality(0)
    t0 = ctx.stat("one_sync_taken")
    rs = ctx.upload_bamfile(d)
    zero = (ctx.step(rs, n_pos, 0, True)[3], rs.n_piled, rs.max_end, rs.min_base_quality, ctx.stat("one_sync_taken") - t0)
    rs.free()
    assert np.array_equal(zero[0], never[0]) and zero[1:] == never[1:] and never[3:] == (0, 1)
    assert np.array_equal(never[0], mixed_oracle(0)[0])
    ctx.set_min_base_quality(13)
    rs = ctx.upload_bamfile(d)
    ctx.set_min_base_quality(0)                                                 # the context forgets, the read set does not
    assert rs.min_base_quality == 13
    assert np.array_equal(ctx.step(rs, n_pos, 0, True)[3], want13)
    rs.free()
    d.close()
    for bad in (256, -1):
        with pytest.raises(_ffi.TcmiError) as e:
            ctx.set_min_base_quality(bad)
        assert e.value.code == _ffi.E_ARG


@pytest.mark.gpu
def test_together_with_the_read_filter(ctx, tmp_path):
    f = (20, 0, 0x400)
    specs = rsp.mixed()[2]
    b, n_fail = rsp.kept(specs, f)
    rb = rsp.arrays(b)
    path = str(tmp_path / "A.bam")
    bamwriter.write_bam(path, rsp.arrays(specs), ref_len=L, block=4096)
    n_pos = c_oracle.extent(rb, L)
    want = oracle_counts(rb, 13, n_pos)                                         # the oracle on the records that pass
    for how in PACKERS:
        got, piled, end, rs_q = through(ctx, how, path, 13, n_pos, f)
        assert np.array_equal(got, want) and rs_q == 13, how
        assert (piled, end) == through(ctx, how, path, 0, n_pos, f)[1:3]


@pytest.mark.gpu
@pytest.mark.parametrize("split_sub", (1, 2))
def test_one_file_over_three_ranks(tmp_path, split_sub):
    """split_ranks_in_turn(world = 3, min_baseq = 13): the ranges in one piece, and as two sub-ranges each (the helper contexts take
    the floor along).  The sub-range file holds every record four times: its oracle is four times the fixture's."""
    ref, orfs, specs = rsp.mixed()
    want, n_pos = mixed_oracle(13)
    times = 1 if split_sub == 1 else 4
    big = specs if times == 1 else sorted([dict(r, name="%s_%d" % (r["name"], k)) for k in range(4) for r in specs], key=lambda r: r["pos"])
    path = str(tmp_path / "A.bam")
    bamwriter.write_bam(path, rsp.arrays(big), ref_len=L, block=1024 if split_sub == 2 else 4096)
    tm = {}
    ta = distributed.split_ranks_in_turn(path, n_pos, cr.gff_rows(orfs), 10, 3, return_parts=True, rules=engine.ReadRules(min_baseq=13), split_sub=split_sub, timings=tm)
    tb = distributed.split_ranks_in_turn(path, n_pos, cr.gff_rows(orfs), 10, 1, return_parts=True, rules=engine.ReadRules(min_baseq=13), split_sub=1)
    assert np.array_equal(ta[1], times * want)
    assert ta[0] == tb[0] and np.array_equal(ta[1], tb[1]) and ta[2] == tb[2]
    assert (tm["split_sub_taken"] > 0) == (split_sub == 2)


@pytest.mark.gpu
def test_two_reference_contig_layout(ctx, tmp_path):
    """the several-kernel packer under a contig layout: every contig's slice of the matrix equals the oracle on that contig's reads"""
    recs, _, specs = two_contigs()
    refs = [("c0", 1500), ("c1", 1200)]
    path = str(tmp_path / "A.bam")
    bamwriter.write_bam(path, rsp.arrays(specs), refs=refs, block=4096)
    shift, slot, axis = contigs.layout_for(recs, [n for n, _ in refs], [ln for _, ln in refs])
    t0 = ctx.stat("one_sync_taken")
    counts = contigs.step_contigs(ctx, path, shift, slot, axis, 10, True, [n for n, _ in refs], want_counts=True, rules=engine.ReadRules(min_baseq=13))[3]
    assert ctx.stat("one_sync_taken") == t0
    seen = np.zeros(axis, bool)
    for t, (_, ln) in enumerate(refs):
        rd = rsp.arrays([dict(r, tid=0) for r in specs if r["tid"] == t])
        n_pos = c_oracle.extent(rd, ln)
        want = oracle_counts(rd, 13, n_pos)
        assert 0.3 < want[:, 0].sum() / oracle_counts(rd, 0, n_pos)[:, 0].sum() < 0.95
        assert np.array_equal(counts[int(shift[t]):int(shift[t]) + n_pos], want), t
        seen[int(shift[t]):int(shift[t]) + n_pos] = True
    assert not counts[~seen].any()


@pytest.mark.gpu
def test_flat_array_entry_points_refuse(ctx):
    rd = rsp.arrays(rsp.mixed()[2][:300])
    n_pos = c_oracle.extent(rd, L)
    p = engine.Pipeline(device=0, slots=2, walkers=1)
    try:
        rs = p.ctx.upload(rd)
        ctx.set_min_base_quality(13)
        p.ctx.set_min_base_quality(13)
        for call in (lambda: ctx.upload(rd), lambda: ctx.tally(rd, L=n_pos), lambda: ctx.upload_batch([rd, rd], 2048),
                     lambda: p.run([rs], n_pos, 10, True)):
            with pytest.raises(_ffi.TcmiError) as e:
                call()
            assert e.value.code == _ffi.E_UNSUPPORTED and "--min-baseq" in str(e.value)
        ctx.set_min_base_quality(0)
        p.ctx.set_min_base_quality(0)
        assert np.array_equal(ctx.tally(rd, L=n_pos), c_oracle.tally(rd, n_pos))   # the context is usable afterwards
        assert np.array_equal(p.ctx.step(rs, n_pos, 0, True)[3], c_oracle.tally(rd, n_pos))
        rs.free()
    finally:
        ctx.set_min_base_quality(0)
        p.close()


# ---- command line ---------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
def test_cli_single_sample_and_batch(tmp_path, monkeypatch):
    """-i with --min-baseq 13: -doc is the oracle's coverage column; FASTA, VCF and GFF equal the run WITHOUT the flag whose counts
    --index-override replaces, at every position, by the oracle's Q 13 matrix (downstream code only).  --batch equals -i."""
    monkeypatch.chdir(tmp_path)
    ref, orfs, specs = rsp.mixed()
    want, n_pos = mixed_oracle(13)
    assert n_pos == L
    rd = rsp.arrays(specs)
    bamwriter.write_bam("A.bam", rd, ref_len=L, block=4096)
    bamwriter.write_bam("A2.bam", rd, ref_len=L, block=4096, split_records=True)
    common = cr.setup_cli(ref, orfs)
    cr.write_override("o.csv.gz", want)
    out = lambda t: ["-o", t + ".fa", "-vcf", t + ".vcf", "-ogff", t + ".gff", "-doc", t + ".tsv"]
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + out("a") + ["--min-baseq", "13", "--stats", "a.json"])
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + out("b") + ["--index-override", "o.csv.gz", "--stats", "b.json"])
    assert cr.doc_column("a.tsv") == want[:, 0].tolist()
    assert cr.outputs("a") == cr.outputs("b")
    assert json.load(open("a.json"))["min_baseq"] == 13 and json.load(open("b.json"))["min_baseq"] == 0
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + ["-o", "raw.fa", "-doc", "raw.tsv"])   # (the process's context is back at no floor)
    assert cr.doc_column("raw.tsv") == mixed_oracle(0)[0][:, 0].tolist() and open("raw.fa").read() != open("a.fa").read()
    with open("m.tsv.in", "w") as fh:
        for k, bam in enumerate(("A.bam", "A2.bam")):
            fh.write("\t".join([bam, "S"] + ["m%d.%s" % (k, e) for e in ("fa", "vcf", "gff", "tsv")]) + "\n")
    cr.run_cli(monkeypatch, ["--batch", "m.tsv.in"] + common + ["--min-baseq", "13"])
    for k in (0, 1):
        assert cr.outputs("m%d" % k) == cr.outputs("a"), k


@pytest.mark.gpu
def test_cli_one_file_over_two_gpus(tmp_path, monkeypatch):
    """--gpus 2 (two ranks rehearsed on this one GPU, gloo for the exchange) refuses --index-override: -doc is the oracle's coverage
    and every output equals the single-GPU run of the same file under the same floor."""
    monkeypatch.chdir(tmp_path)
    ref, orfs, specs = rsp.mixed()
    want, _ = mixed_oracle(13)
    bamwriter.write_bam("A.bam", rsp.arrays(specs), ref_len=L, block=4096, split_records=True)
    common = cr.setup_cli(ref, orfs)
    for tag, extra in (("a", ["--gpus", "2"]), ("b", [])):
        cr.run_two_ranks(["-i", "A.bam", "-name", "S"] + common + cr.out_args(tag) + ["--min-baseq", "13"] + extra)
    assert cr.doc_column("a.tsv") == want[:, 0].tolist()
    assert cr.outputs("a") == cr.outputs("b")


@pytest.mark.gpu
def test_cli_per_contig(tmp_path, monkeypatch):
    """--per-contig refuses --index-override: per contig, -doc is the oracle's coverage and the FASTA record equals the single run
    of that contig's reads alone under the same floor."""
    monkeypatch.chdir(tmp_path)
    recs, rows, specs = two_contigs()
    refs = [("c0", 1500), ("c1", 1200)]
    bamwriter.write_bam("A.bam", rsp.arrays(specs), refs=refs, block=4096)
    cr.setup_contigs(recs, rows)
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-ref", "r.fa", "-gff", "g.gff", "-cov", "10", "-name", "S", "-o", "a.fa", "-doc", "a.tsv",
                             "--per-contig", "--min-baseq", "13", "--stats", "a.json"])
    assert json.load(open("a.json"))["min_baseq"] == 13
    want_fa, want_tsv = "", ""
    for t, (name, ln) in enumerate(refs):
        rd = rsp.arrays([dict(r, tid=0) for r in specs if r["tid"] == t])
        want = oracle_counts(rd, 13, c_oracle.extent(rd, ln))
        bamwriter.write_bam("one%d.bam" % t, rd, refs=[(name, ln)], block=4096)
        open("r%d.fa" % t, "w").write(">%s\n%s\n" % recs[t])
        open("g%d.gff" % t, "w").write("##gff-version 3\n" + sy.gff_text(rows[t][1], seqid=name)[1])
        cr.run_cli(monkeypatch, ["-i", "one%d.bam" % t, "-ref", "r%d.fa" % t, "-gff", "g%d.gff" % t, "-cov", "10", "-name", "S_" + name,
                                 "-o", "one%d.fa" % t, "-doc", "one%d.tsv" % t, "--min-baseq", "13"])
        assert cr.doc_column("one%d.tsv" % t) == want[:, 0].tolist()
        want_fa += open("one%d.fa" % t).read()
        want_tsv += "".join("%s\t%s" % (name, line) for line in open("one%d.tsv" % t))
    assert open("a.fa").read() == want_fa and want_fa.count(">") == 2
    assert open("a.tsv").read() == want_tsv
