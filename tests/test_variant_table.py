"""The variant table on the GPU (csrc/variants.hip; tcmi_variants_dev, tcmi_variants, tcmi_ctx_set_variants, tcmi_step_variants, the
file runner's tables, --variant-table): every comparison is exact equality of record arrays — order included — or of the table's text
with the yardstick (tests/variant_yardstick.py, plain Python integers).  The rule itself, the row writer and the argument handling
are checked without a GPU in tests/test_variant_rule.py."""
import functools
import json
import os

import numpy as np
import pytest

from oracle import c_oracle
from tests import cli_run as cr
from tests import device_file as dvf
from tests import primer_yardstick as py
from tests import read_specs as rsp
from tests import schemes as sch
from tests import synth_small as ss
from tests import variant_yardstick as vy
from trueconsense_amd import _ffi, contigs, engine
from trueconsense_amd.io import bamwriter

pytestmark = pytest.mark.gpu
RULE = (1, 10, 2, 5)                # min_af 1/10, min_alt_depth 2, min_depth 5
KW = dict(min_af="1/10", min_alt_depth=2, min_depth=5)
REF_BYTES = np.frombuffer(b"ACGTacgtACGTACGTN\0", np.uint8)


@pytest.fixture(scope="module")
def ctx():
    with engine.Context(0) as c:
        yield c


def random_case(L, seed, n_ref=None):
    """counts [L, 7] whose alleles sit around the thresholds (ties of count * 10 == cov among them) and a reference of n_ref bytes"""
    rng = np.random.default_rng(seed)
    c = np.zeros((L, 7), np.int64)
    c[:, 0] = rng.choice([0, 4, 5, 10, 20, 30, 50], L)
    for a in range(1, 7):
        frac = rng.choice([0, 0, 0.04, 0.1, 0.1, 0.2, 0.5, 1.0], L)
        c[:, a] = np.floor(c[:, 0] * frac + rng.choice([0, 0, 0, 1, -1], L)).clip(0)
    n_ref = L if n_ref is None else n_ref
    return c.astype(np.int32), rng.choice(REF_BYTES, n_ref).tobytes()


def planes(counts, ld, seed=5):
    """rows [L, 7] -> the body of an int32 [7][ld] matrix whose padding [L, ld) holds garbage that would give records"""
    L = len(counts)
    body = np.random.default_rng(seed).integers(1, 1 << 20, (7, ld)).astype(np.int32)
    body[:, :L] = counts.T
    return body


def on_device(ctx, counts, ref, ld=None, off=0, cap=None, rec_lead=0, rule_kw=KW):
    """tcmi_variants_dev on a matrix between guards (off: words past an 8-byte boundary), a guarded reference and a guarded record
    buffer of `cap` records -> (records read back, n_found, TcmiError or None); the matrix must be bit-identical afterwards"""
    L = len(counts)
    ld = L if ld is None else ld
    m = dvf.Matrix(L, ld, off, planes(counts, ld))
    r = dvf.Guarded(len(ref), np.uint8, 0, np.frombuffer(ref, np.uint8)) if len(ref) else None
    room = 5 * min(L, len(ref)) if cap is None else cap
    out = dvf.Guarded(4 * room, np.int32, rec_lead, salt=77) if room else None
    err = None
    try:
        n = ctx.variants_dev(m.ptr, L, ld, r.ptr if r else 0, len(ref), d_records=out.ptr if out else 0, cap=room, **rule_kw)
    except _ffi.TcmiError as e:
        err, n = e, e.n_found
    assert m.untouched(), "the matrix was written"
    assert r is None or r.untouched()
    body = out.read() if out else np.zeros(0, np.int32)       # (read() checks both guards)
    recs = body.view(vy.DTYPE)
    k = min(n, room)
    if out is not None:
        assert np.array_equal(body[4 * k:], out.init[out.lo + 4 * k:out.lo + 4 * room]), "something was written behind the records"
    return recs[:k].copy(), n, err


@pytest.mark.parametrize("L", (1, 63, 64, 255, 256, 257, 1000))
def test_random_matrices_on_both_entry_points(ctx, L):
    """ld = L, an odd ld, ld rounded up to 256; the matrix 4 bytes past an 8-byte boundary; n_ref = 0, L - 1, L, L + 5; the record
    buffer on and off a 16-byte boundary; tcmi_variants on the same input"""
    total = 0
    for k, n_ref in enumerate((0, L - 1, L, L + 5)):
        counts, ref = random_case(L, 100 * L + k, n_ref)
        want = vy.as_array(vy.records(counts, ref, *RULE))
        total += len(want)
        assert np.array_equal(ctx.variants(counts, ref, **KW), want), (L, n_ref)
        for ld, off, lead in ((L, 1, 0), (L + 1 + L % 2, 0, 1), ((L + 255) // 256 * 256, 1, 1), ((L + 255) // 256 * 256, 0, 0)):
            got, n, err = on_device(ctx, counts, ref, ld, off, rec_lead=lead)
            assert err is None and n == len(want) and np.array_equal(got, want), (L, n_ref, ld, off, lead)
    assert total > 0 or L == 1


def test_densest_and_emptiest_blocks_side_by_side(ctx):
    L = 768
    counts = np.zeros((L, 7), np.int32)
    ref = bytearray(b"A" * L)
    counts[:256] = (100, 0, 20, 20, 20, 20, 20)                                     # block 0: five records a position
    counts[256:512] = (100, 100, 0, 0, 0, 0, 0)                                     # block 1: none (the reference allele, an N, no coverage)
    ref[300:340] = b"N" * 40
    counts[400:512, 0] = 0
    for lane in (0, 63, 64, 255):                                                   # block 2: the wavefronts' edges, one record each
        counts[512 + lane] = (50, 40, 0, 0, 10, 0, 0)
    want = vy.as_array(vy.records(counts, bytes(ref), *RULE))
    assert len(want) == 1280 + 4 and want["pos"][1280:].tolist() == [512, 575, 576, 767] and (want["pos"][:1280] == np.repeat(np.arange(256), 5)).all()
    assert want["allele"][:10].tolist() == [2, 3, 4, 5, 6] * 2
    got, n, err = on_device(ctx, counts, bytes(ref), 768)
    assert err is None and n == 1284 and np.array_equal(got, want)
    assert np.array_equal(ctx.variants(counts, bytes(ref), **KW), want)


def test_the_scans_carry(ctx):
    """1 025 blocks + 3 positions: the one-workgroup scan takes its second chunk with a carry; a record-bearing position in each of
    blocks 0, 1023, 1024 and 1025, a sprinkle elsewhere"""
    L = 256 * 1025 + 3
    rng = np.random.default_rng(9)
    counts = np.zeros((L, 7), np.int32)
    where = rng.choice(L, 3000, replace=False)
    counts[where] = random_case(3000, 10)[0]
    for p in (7, 256 * 1023 + 255, 256 * 1024, L - 1):
        counts[p] = (40, 0, 0, 0, 30, 10, 0)
    ref = b"A" * L
    want = vy.as_array(vy.records(counts, ref, *RULE))
    for p in (7, 256 * 1023 + 255, 256 * 1024, L - 1):
        assert (want["pos"] == p).sum() == 2
    assert len(want) > 1000 and (np.diff(want["pos"].astype(np.int64)) >= 0).all()
    got, n, err = on_device(ctx, counts, ref, 256 * 1026)
    assert err is None and n == len(want) and np.array_equal(got, want)


def test_capacity(ctx):
    counts, ref = random_case(1000, 3)
    want = vy.as_array(vy.records(counts, ref, *RULE))
    n = len(want)
    assert n > 300
    got, found, err = on_device(ctx, counts, ref, 1024, cap=n)
    assert err is None and found == n and np.array_equal(got, want)
    for lead in (0, 1):                                                             # one record short: the first n - 1, nothing behind them, E_ARG
        got, found, err = on_device(ctx, counts, ref, 1024, cap=n - 1, rec_lead=lead)
        assert err is not None and err.code == _ffi.E_ARG and found == n and np.array_equal(got, want[:n - 1])
    got, found, err = on_device(ctx, counts, ref, 1024, cap=0)                      # cap = 0, no buffer: count only
    assert err is None and found == n and len(got) == 0
    small = np.zeros(7, vy.DTYPE)                                                   # the host convenience: the same contract
    f = _ffi.C.c_int64(0)
    num, den = 1, 10
    rc = _ffi.lib().tcmi_variants(ctx.handle, _ffi.ptr(counts), 1000, _ffi.ptr(np.frombuffer(ref, np.uint8)), 1000, num, den, 2, 5, _ffi.ptr(small), 6, _ffi.C.byref(f))
    assert rc == _ffi.E_ARG and f.value == n and np.array_equal(small[:6], want[:6]) and small[6].tolist() == (0, 0, 0, 0)
    rc = _ffi.lib().tcmi_variants(ctx.handle, _ffi.ptr(counts), 1000, _ffi.ptr(np.frombuffer(ref, np.uint8)), 1000, num, den, 2, 5, None, 0, _ffi.C.byref(f))
    assert rc == 0 and f.value == n


def test_argument_errors(ctx):
    counts, ref = random_case(64, 1)
    lib, h, f = _ffi.lib(), ctx.handle, _ffi.C.c_int64(0)
    r = np.frombuffer(ref, np.uint8)
    out = np.zeros(320, vy.DTYPE)
    for num, den, mad, md in ((1, 0, 1, 0), (1, 1000001, 1, 0), (2, 1, 1, 0), (-1, 10, 1, 0), (1, 10, 0, 0), (1, 10, 1, -1)):
        assert lib.tcmi_variants(h, _ffi.ptr(counts), 64, _ffi.ptr(r), 64, num, den, mad, md, _ffi.ptr(out), 320, _ffi.C.byref(f)) == _ffi.E_ARG
        assert lib.tcmi_ctx_set_variants(h, _ffi.ptr(r), 64, num, den, mad, md) == _ffi.E_ARG
    assert lib.tcmi_variants(h, _ffi.ptr(counts), 64, _ffi.ptr(r), -1, 1, 10, 1, 0, _ffi.ptr(out), 320, _ffi.C.byref(f)) == _ffi.E_ARG
    assert lib.tcmi_variants(h, _ffi.ptr(counts), 64, _ffi.ptr(r), 64, 1, 10, 1, 0, _ffi.ptr(out), -1, _ffi.C.byref(f)) == _ffi.E_ARG
    assert lib.tcmi_ctx_set_variants(h, _ffi.ptr(r), -1, 1, 10, 1, 0) == _ffi.E_ARG
    with pytest.raises(_ffi.TcmiError):                                             # none of them left a setting behind
        ctx.step_variants()
    assert lib.tcmi_variants(h, _ffi.ptr(counts), 64, _ffi.ptr(r), 64, 1, 1000000, 1, 0, _ffi.ptr(out), 320, _ffi.C.byref(f)) == 0


# ---- the step path --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_files():
    """one tests/synth_small.py case with planted minor alleles, a deletion and an insertion -> (reference, reads A, reads B): B is
    every second record of A"""
    spec = ss.read_specs(np.random.default_rng(4242))[3]
    a = spec["reads"]
    return spec["ref"], ss.reads_from_spec({"reads": a}), ss.reads_from_spec({"reads": a[::2]})


STEP_KW = dict(min_af="1/20", min_alt_depth=1, min_depth=1)
STEP_RULE = (1, 20, 1, 1)


@pytest.mark.parametrize("one_sync", (1, 0))
def test_step_path(ctx, tmp_path, one_sync):
    ref, ra, rb = small_files()
    L = len(ref)
    paths = []
    for tag, rd in (("A", ra), ("B", rb)):
        paths.append(str(tmp_path / (tag + ".bam")))
        bamwriter.write_bam(paths[-1], rd, "ref", L)
    plain, tallies = [], []
    with engine.Context(0) as bare:                                                 # the same files on a context without the setting
        for p, rd in zip(paths, (ra, rb)):
            d = engine.DeviceBam(p)
            rs, pl, al, fl, counts = bare.bamfile_step(d, L, 5, True, want_counts=True)
            rs.free()
            d.close()
            plain.append((pl, al, fl))
            tallies.append(bare.tally(rd, ref_len=L))
            assert np.array_equal(counts, tallies[-1])
    want = [vy.as_array(vy.records(t, ref.encode(), *STEP_RULE)) for t in tallies]
    assert set(want[0]["allele"].tolist()) >= {5, 6} and len(set(want[0]["allele"].tolist()) & {1, 2, 3, 4}) >= 3      # (non-vacuity)
    assert len(want[0]) > 20 and len(want[1]) > 10 and not np.array_equal(want[0], want[1])
    try:
        ctx.set_option("one_sync", one_sync)
        with pytest.raises(_ffi.TcmiError):
            ctx.step_variants()                                                     # no step has computed a table yet
        ctx.set_variants(ref, **STEP_KW)
        for want_counts in (False, True):
            for k in (0, 1, 0):                                                     # the second and third step: the other file's records, then the first's again
                d = engine.DeviceBam(paths[k])
                before = (ctx.stat("one_sync_taken"), ctx.stat("one_sync_declined"))
                rs, pl, al, fl, counts = ctx.bamfile_step(d, L, 5, True, want_counts=want_counts)
                # the file really took the route asked for: the one-sync packer delivered it, or was never tried (the several-kernel path)
                assert (ctx.stat("one_sync_taken"), ctx.stat("one_sync_declined")) == (before[0] + one_sync, before[1]), (one_sync, k)
                got = ctx.step_variants()
                rs.free()
                d.close()
                assert np.array_equal(got, want[k]), (one_sync, want_counts, k)
                assert all(np.array_equal(x, y) for x, y in zip((pl, al, fl), plain[k]))
                assert (counts is None) if not want_counts else np.array_equal(counts, tallies[k])
        rs = ctx.upload(ra)                                                         # ... and through tcmi_step from flat arrays
        ctx.step(rs, len(tallies[0]), 5, True, want_counts=False)
        assert np.array_equal(ctx.step_variants(), want[0])
        ctx.set_variants(ref[:40], **STEP_KW)                                       # a shorter reference: nothing behind it, and no stale records
        with pytest.raises(_ffi.TcmiError):
            ctx.step_variants()
        ctx.step(rs, len(tallies[0]), 5, True, want_counts=True)
        assert np.array_equal(ctx.step_variants(), want[0][want[0]["pos"] < 40])
        ctx.set_variants(None)
        with pytest.raises(_ffi.TcmiError) as e:
            ctx.step_variants()
        assert e.value.code == _ffi.E_ARG
        assert np.array_equal(ctx.step(rs, len(tallies[0]), 5, True)[3], tallies[0])
        with pytest.raises(_ffi.TcmiError):
            ctx.step_variants()                                                     # a step without the setting computes none
        rs.free()
    finally:
        ctx.set_option("one_sync", 1)
        ctx.set_variants(None)


def test_array_pipeline_refuses(ctx):
    ref, ra, _ = small_files()
    n_pos = c_oracle.extent(ra, len(ref))
    p = engine.Pipeline(device=0, slots=2, walkers=1)
    try:
        rs = p.ctx.upload(ra)
        for k in range(2):
            p.slot_context(k).set_variants(ref, **STEP_KW)
        with pytest.raises(_ffi.TcmiError) as e:
            p.run([rs], n_pos, 10, True)
        assert e.value.code == _ffi.E_UNSUPPORTED and "--variant-table" in str(e.value)
        for k in range(2):
            p.slot_context(k).set_variants(None)
        assert np.array_equal(p.ctx.step(rs, n_pos, 0, True)[3], c_oracle.tally(ra, n_pos))    # usable afterwards
        rs.free()
    finally:
        p.close()


def test_file_runner_tables_and_the_host_reader_fallback(tmp_path):
    ref, ra, rb = small_files()
    L = len(ref)
    paths, tables = [], []
    for tag, rd in (("A", ra), ("B", rb), ("C", ra)):
        paths.append(str(tmp_path / (tag + ".bam")))
        tables.append(None if tag == "C" else str(tmp_path / (tag + ".tsv")))
        bamwriter.write_bam(paths[-1], rd, "ref", L)
    want = [engine.VARIANTS_HEADER + vy.text(vy.records(c_oracle.tally(rd, c_oracle.extent(rd, L)), ref.encode(), *STEP_RULE), "ref", ref.encode())
            for rd in (ra, rb)]
    for device_decode in (True, False):
        runner = engine.FileRunner(0, [], 5, gpu_streams=2, variants=dict(STEP_KW, ref=ref))
        runner.device_decode = device_decode
        runner.set_outputs("ref", ref, "##vcf\n", "##gff\n", [])
        fasta = [str(tmp_path / ("%d%d.fa" % (k, device_decode))) for k in range(3)]
        runner.run_files(paths, ["S"] * 3, fasta, ref_len=L, table=tables)
        assert runner.decoded_on == ({"device": 3, "host": 0} if device_decode else {"device": 0, "host": 3})
        assert [open(t).read() for t in tables[:2]] == want and not os.path.exists(str(tmp_path / "C.tsv"))
        assert runner.variant_records == sum(w.count("\n") - 1 for w in want)
        for t in tables[:2]:
            os.remove(t)
        runner.close()
    unset = engine.FileRunner(0, [], 5, gpu_streams=1, variants=dict(STEP_KW, ref=ref))   # a table without the reference of set_outputs: refused up front
    with pytest.raises(_ffi.TcmiError) as e:
        unset.run_files(paths[:1], ["S"], [str(tmp_path / "y.fa")], ref_len=L, table=tables[:1])
    assert e.value.code == _ffi.E_ARG and "tcmi_filerunner_set_outputs" in str(e.value) and not os.path.exists(tables[0])
    unset.close()
    bare = engine.FileRunner(0, [], 5, gpu_streams=1)                               # a table without the setting: refused, nothing silently skipped
    bare.set_outputs("ref", ref, "##vcf\n", "##gff\n", [])
    with pytest.raises(_ffi.TcmiError) as e:
        bare.run_files(paths[:1], ["S"], [str(tmp_path / "x.fa")], ref_len=L, table=tables[:1])
    assert e.value.code == _ffi.E_ARG and "tcmi_ctx_set_variants" in str(e.value)
    bare.close()


# ---- command line ---------------------------------------------------------------------------------------------------------------
FLAGS = ["--min-af", "0.02", "--min-alt-depth", "2", "--variant-min-depth", "8"]
CLI_RULE = (1, 50, 2, 8)


def table_text(counts, ref, region="ref", rule=CLI_RULE):
    return engine.VARIANTS_HEADER + vy.text(vy.records(counts, ref.encode(), *rule), region, ref.encode())


def test_cli_single_sample_and_batch(tmp_path, monkeypatch):
    """-i with --variant-table: the table is the yardstick's over the oracle's matrix, the four other outputs are those of the run
    without the flag; with --min-baseq 20 --primers it follows the masked matrix, with --index-override the overridden one; --batch
    with a 7-column manifest writes each sample's -i table, a 6-column manifest none"""
    monkeypatch.chdir(tmp_path)
    ref, orfs, specs = rsp.mixed()
    L = rsp.L
    rd, rd3 = rsp.arrays(specs), rsp.arrays(specs[::2])
    bamwriter.write_bam("A.bam", rd, ref_len=L, block=4096)
    bamwriter.write_bam("A2.bam", rd, ref_len=L, block=4096, split_records=True)
    bamwriter.write_bam("A3.bam", rd3, ref_len=L, block=4096)
    common = cr.setup_cli(ref, orfs)
    counts = c_oracle.tally(rd, c_oracle.extent(rd, L))
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + cr.out_args("a") + ["--variant-table", "a.var", "--stats", "a.json"] + FLAGS)
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + cr.out_args("b") + ["--stats", "b.json"])
    want = table_text(counts, ref)
    assert open("a.var").read() == want and want.count("\n") > 50 and "\t*\t" in want and "\t+\t" in want
    assert cr.outputs("a") == cr.outputs("b") and not os.path.exists("b.var")
    assert (json.load(open("a.json"))["variant_records"], json.load(open("b.json"))["variant_records"]) == (want.count("\n") - 1, 0)
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + ["-o", "d.fa", "--variant-table", "d.var"])       # the defaults: 3 %, 1, 10
    assert open("d.var").read() == table_text(counts, ref, rule=(3, 100, 1, 10))
    # the floor and the primer mask: the table follows the masked matrix
    sch.write_primer_bed("p.bed", sch.PRIMER_SCHEME)
    masked = py.counts(rd, L, sch.PRIMER_SCHEME, 20)[0]
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + ["-o", "q.fa", "--variant-table", "q.var", "--min-baseq", "20", "--primers", "p.bed"] + FLAGS)
    assert open("q.var").read() == table_text(masked, ref) != want
    # --index-override: the table is taken behind the override
    over = counts.copy()
    over[100:140] = (60, 10, 20, 0, 30, 6, 3)
    cr.write_override("o.csv.gz", over)
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + ["-o", "o.fa", "--variant-table", "o.var", "--index-override", "o.csv.gz"] + FLAGS)
    assert open("o.var").read() == table_text(over, ref) != want
    # --batch: three samples, the manifest's 7th column
    cr.run_cli(monkeypatch, ["-i", "A3.bam", "-name", "S"] + common + cr.out_args("a3") + ["--variant-table", "a3.var"] + FLAGS)
    with open("m7.tsv", "w") as fh:
        for k, bam in enumerate(("A.bam", "A2.bam", "A3.bam")):
            fh.write("\t".join([bam, "S"] + ["m%d.%s" % (k, e) for e in ("fa", "vcf", "gff", "tsv", "var")]) + "\n")
    cr.run_cli(monkeypatch, ["--batch", "m7.tsv"] + common + FLAGS + ["--stats", "m.json"])
    for k, tag in enumerate(("a", "a", "a3")):
        assert open("m%d.var" % k).read() == open(tag + ".var").read(), k
        assert cr.outputs("m%d" % k) == cr.outputs(tag), k
    assert json.load(open("m.json"))["variant_records"] == 2 * (want.count("\n") - 1) + open("a3.var").read().count("\n") - 1
    with open("m6.tsv", "w") as fh:
        for k, bam in enumerate(("A.bam", "A2.bam", "A3.bam")):
            fh.write("\t".join([bam, "S"] + ["s%d.%s" % (k, e) for e in ("fa", "vcf", "gff", "tsv")]) + "\n")
    cr.run_cli(monkeypatch, ["--batch", "m6.tsv"] + common)
    for k, tag in enumerate(("a", "a", "a3")):
        assert cr.outputs("s%d" % k) == cr.outputs(tag) and not os.path.exists("s%d.var" % k)


def test_cli_per_contig(tmp_path, monkeypatch):
    """--per-contig: one file for both contigs in axis order, rows with the contig's name and its own positions; nothing from the
    guard columns behind a contig's end or from the slots' padding"""
    monkeypatch.chdir(tmp_path)
    recs, rows, specs = rsp.two_contigs()
    refs = [("c0", 1500), ("c1", 1200)]
    bamwriter.write_bam("A.bam", rsp.arrays(specs), refs=refs, block=4096)
    cr.setup_contigs(recs, rows)
    args = ["-i", "A.bam", "-ref", "r.fa", "-gff", "g.gff", "-cov", "10", "-name", "S", "--per-contig"]
    cr.run_cli(monkeypatch, args + ["-o", "a.fa", "-doc", "a.tsv", "--variant-table", "a.var", "--stats", "a.json"] + FLAGS)
    cr.run_cli(monkeypatch, args + ["-o", "b.fa", "-doc", "b.tsv"])
    want = engine.VARIANTS_HEADER
    for t, (name, ln) in enumerate(refs):
        rd = rsp.arrays([dict(r, tid=0) for r in specs if r["tid"] == t])
        counts = c_oracle.tally(rd, c_oracle.extent(rd, ln))
        part = vy.text(vy.records(counts, recs[t][1].encode(), *CLI_RULE), name, recs[t][1].encode())
        assert part.count("\n") > 10
        want += part
    got = open("a.var").read()
    assert got == want
    regions = [ln.split("\t")[0] for ln in got.split("\n")[1:] if ln]
    assert regions == sorted(regions) and set(regions) == {"c0", "c1"}
    assert max(int(ln.split("\t")[1]) for ln in got.split("\n")[1:] if ln.startswith("c1\t")) <= 1200
    assert open("a.fa").read() == open("b.fa").read() and open("a.tsv").read() == open("b.tsv").read()
    assert json.load(open("a.json"))["variant_records"] == got.count("\n") - 1


def test_cli_split_worker_at_world_one(tmp_path, monkeypatch):
    """`-i --gpus N`'s worker (trueconsense_amd.split_main) as one rank: rank 0 takes the table from the reduced counts; the parent
    forwards the flags (tests/test_variant_rule.py checks the children's command line)"""
    monkeypatch.chdir(tmp_path)
    ref, orfs, specs = rsp.mixed()
    rd = rsp.arrays(specs)
    bamwriter.write_bam("A.bam", rd, ref_len=rsp.L, block=4096, split_records=True)
    common = cr.setup_cli(ref, orfs)
    cr.run_split_worker(["-i", "A.bam", "-name", "S"] + common + cr.out_args("w") + ["--variant-table", "w.var", "--gpus", "1"] + FLAGS)
    assert open("w.var").read() == table_text(c_oracle.tally(rd, c_oracle.extent(rd, rsp.L)), ref)
