"""--mate-overlap on the GPU (csrc/mate_join.hip and what takes its clip along): both packers against the yardstick
(tests/mate_overlap_yardstick.py) on the hand-made cases and two fuzz seeds, plain, under a floor, under a primer table, each with a read
filter; mates in different BGZF blocks; a file past one trip of the join's grid; the stream-walking tables under the rule; the refusals
through the ABI; the command line.  The rule's text and what the fuzz holds: tests/test_mate_rule.py."""
import ctypes as C
import contextlib
import json

import numpy as np
import pytest

from tests import cli_run as cr
from tests import device_file as dvf
from tests import evidence_yardstick as ey
from tests import mate_big as mb
from tests import mate_overlap_cases as mc
from tests import mate_overlap_yardstick as my
from tests import primer_yardstick as py
from tests import repeat_bam as rb
from tests import rules_marks as rm
from tests import schemes as sch
from trueconsense_amd import _ffi, distributed, engine
from trueconsense_amd import synthetic as sy
from trueconsense_amd.io import bamwriter

pytestmark = pytest.mark.gpu
SCHEME = list(sch.PRIMER_SCHEME)
DATA = ("cases",) + tuple("seed%d" % s for s in mc.FUZZ_SEEDS)
# mode -> (primer table, floor, read filter)
MODES = {"plain": ((), 0, my.NONE), "floor": ((), mc.FLOOR, my.NONE), "primers": (SCHEME, 0, my.NONE),
         "plain_filter": ((), 0, mc.FILTER), "floor_filter": ((), mc.FLOOR, mc.FILTER), "primers_filter": (SCHEME, 0, mc.FILTER)}
SC_BLOCK, SC_WG_PER_CU = rb.stream_count_caps()


@pytest.fixture(scope="module")
def ctx():
    with engine.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    """the module's directory, the files written once and the yardsticks computed once: {key: value}"""
    return {"dir": tmp_path_factory.mktemp("mate")}


def once(store, key, make):
    if key not in store:
        store[key] = make()
    return store[key]


def data(store, key, **kw):
    """-> (path, flat arrays) of the case file / a fuzz seed's file"""
    def make():
        specs = mc.cases()[0] if key == "cases" else mc.fuzz_specs(int(key[4:]))
        rd = mc.arrays(specs)
        path = str(store["dir"] / (key + ".bam"))
        bamwriter.write_bam(path, rd, refs=mc.REFS if key == "cases" else mc.FUZZ_REFS, block=4096)
        return path, rd
    return once(store, ("data", key), make)


def yard(store, key, mode, mate=True):
    primers, q, f = MODES[mode]
    return once(store, ("yard", key, mode, mate), lambda: my.counts(data(store, key)[1], mc.L, primers, q, f=f, mate=mate))


@contextlib.contextmanager
def uploaded(ctx, path, mode="plain", how=None, mate=True):
    """device_file.uploaded with the mate-overlap rule on for the upload alone: the read set must remember it"""
    primers, q, f = MODES[mode]
    ctx.set_mate_overlap(mate)
    try:
        with dvf.uploaded(ctx, path, primers, q, f, how=how) as rs:
            ctx.set_mate_overlap(False)
            yield rs
    finally:
        ctx.set_mate_overlap(False)


def counters(rs):
    return {k: rs.mate_overlap[k] for k in my.COUNTERS}


def check(ctx, rs, y):
    got = ctx.step(rs, len(y["counts"]), 0, True)[3]
    bad = np.argwhere(got != y["counts"])
    assert len(bad) == 0, (len(bad), bad[:6].tolist(), got[tuple(bad[:6].T)].tolist(), y["counts"][tuple(bad[:6].T)].tolist())
    assert rs.mate_overlap["on"] == 1 and counters(rs) == y["counters"], (rs.mate_overlap, y["counters"])
    assert (rs.n_piled, rs.max_end, rs.primer_masked_reads) == (y["n_piled"], y["max_end"], y["n_masked"])


# ---- packers and planes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("how", dvf.PACKERS)
@pytest.mark.parametrize("key", DATA)
def test_both_packers_equal_the_yardstick(ctx, store, key, how, mode):
    path, _ = data(store, key)
    y = yard(store, key, mode)
    assert y["counters"]["clipped_columns"] > 0
    with uploaded(ctx, path, mode, how) as rs:
        assert rs.route == how
        check(ctx, rs, y)


@pytest.mark.parametrize("mode", ("plain", "floor", "primers"))
@pytest.mark.parametrize("how", dvf.PACKERS)
def test_setting_off_is_the_existing_yardstick(ctx, store, how, mode):
    path, rd = data(store, "seed11")
    primers, q, _ = MODES[mode]
    want = py.counts(rd, mc.FUZZ_L, primers, q)
    with uploaded(ctx, path, mode, how, mate=False) as rs:
        got = ctx.step(rs, len(want[0]), 0, True)[3]
        assert np.array_equal(got, want[0]) and rs.mate_overlap == dict(on=0, pairs=0, clipped_reads=0, clipped_columns=0, ambiguous=0)
        assert rs.primer_masked_reads == want[1]
    assert not np.array_equal(want[0], yard(store, "seed11", mode)["counts"])


def test_the_read_set_remembers_and_every_run_gives_the_same(ctx, store):
    path, _ = data(store, "seed12")
    y = yard(store, "seed12", "plain")
    with uploaded(ctx, path, "plain", "one_sync") as rs:
        assert not ctx.mate_overlap
        for _ in range(3):
            check(ctx, rs, y)


def test_one_sync_packer_with_every_array_of_its_scratch(ctx, store):
    """the largest list the one-sync packer takes from the arena (csrc/pack_caps.h pk_one_sync_scratch), all at once: the mate join's
    table and clip, and pk_prefix's three arrays, which a file of a few blocks gets only when the option asks for them; under a primer
    table and a read filter (pk_place_bq, pk_mask_long)"""
    path, _ = data(store, "cases")
    d = engine.DeviceBam(path)
    assert 1 < d.n_blocks < 16384                               # (several workgroups; the prefix kernels are the option's doing)
    d.close()
    y = yard(store, "cases", "primers_filter")
    try:
        ctx.set_option("prefix_kernels", 1)
        with uploaded(ctx, path, "primers_filter", "one_sync") as rs:
            assert rs.route == "one_sync"
            check(ctx, rs, y)
    finally:
        ctx.set_option("prefix_kernels", 0)


# ---- mates in different BGZF blocks and workgroups -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", dvf.PACKERS)
def test_mates_in_different_blocks(ctx, store, how):
    """the case file's records with every pair's loser behind all other records (the rule does not depend on the file's order), in BGZF
    blocks of 248 bytes filled to the brim: the mates of every pair start a dozen blocks apart, those of one pair three dozen"""
    block = 248

    def make():
        specs = mc.cases()[0]
        losers = {lo for lo, _ in yard(store, "cases", "plain")["pairs"]}
        moved = [r for i, r in enumerate(specs) if i not in losers] + [r for i, r in enumerate(specs) if i in losers]
        rd = mc.arrays(moved)
        path = str(store["dir"] / "small_blocks.bam")
        bamwriter.write_bam(path, rd, refs=mc.REFS, block=block, split_records=True)
        return path, rd, my.counts(rd, mc.L)
    path, rd, y = once(store, "small_blocks", make)
    assert y["counters"] == yard(store, "cases", "plain")["counters"] and np.array_equal(y["counts"], yard(store, "cases", "plain")["counts"])
    _, rec = dvf.host_stream_and_records(path)
    blk = (rec // block).astype(np.int64)                       # (block b holds bytes [248 b, 248 b + 248) of the stream)
    gaps = [abs(int(blk[lo]) - int(blk[wi])) for lo, wi in y["pairs"]]
    assert min(gaps) >= 8 and max(gaps) >= 24, gaps
    assert len(set(blk.tolist())) > 30                          # (... and more workgroups of the one-sync packer than that)
    with uploaded(ctx, path, "plain", how) as rs:
        check(ctx, rs, y)


# ---- past one trip of the join's grid ------------------------------------------------------------------------------------------------------------
def test_past_one_trip_of_the_grid(ctx, store):
    cap = ctx.stat("compute_units") * SC_WG_PER_CU * SC_BLOCK
    n = cap + 257
    rd = mb.generate(n)
    path = mb.write(store["dir"] / "big.bam", rd)
    clip, cnt = mb.join(rd)
    assert cnt["pairs"] > cap // 3 and cnt["clipped_reads"] > cap // 4 and int(clip[cap:].sum()) > 0      # (the ragged second trip has losers)
    want = mb.matrix(rd, mb.L, clip)
    for how in dvf.PACKERS:
        ctx.set_mate_overlap(True)
        try:
            with dvf.uploaded(ctx, path, how=how) as rs:
                ctx.set_mate_overlap(False)
                assert rs.n_reads == n and counters(rs) == cnt, (rs.mate_overlap, cnt)
                got = ctx.step(rs, mb.L, 0, True)[3]
                assert np.array_equal(got, want), np.argwhere(got != want)[:6].tolist()
        finally:
            ctx.set_mate_overlap(False)


# ---- the tables that walk the records, under the rule ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("floor", "primers_filter"))
@pytest.mark.parametrize("how", dvf.PACKERS)
def test_strand_and_evidence_counts_under_the_rule(ctx, store, how, mode):
    path, rd = data(store, "cases")
    primers, q, f = MODES[mode]
    y = yard(store, "cases", mode)
    n_pos = len(y["counts"])
    cols = np.arange(n_pos)
    fwd, rev, ev = once(store, ("walked", mode), lambda: rm.walked(rd, y, primers, q, f))
    with uploaded(ctx, path, mode, how) as rs:
        matrix = ctx.step(rs, n_pos, 0, True)[3]
        sc = ctx.strand_counts(rs, cols)
        assert np.array_equal(sc["fwd"] + sc["rev"], matrix)                # (what the writer checks: else no table)
        assert np.array_equal(sc["fwd"], fwd) and np.array_equal(sc["rev"], rev)
        ec = ctx.evidence_counts(rs, cols)
        assert np.array_equal(ec["n"], matrix)
        for k in ("qual", "mapq", "dist"):
            assert np.array_equal(ec[k], ev[k]), k


def test_cli_strand_and_evidence_writers_accept(tmp_path, monkeypatch):
    """-i --mate-overlap --variant-table --variant-strand --variant-evidence: both writers refuse counts that do not add up to the
    (clipped) matrix — they write, and their rows are the existing yardsticks' texts fed the clipped tokens"""
    from tests import strand_yardstick as sty
    from tests import variant_yardstick as vy
    monkeypatch.chdir(tmp_path)
    ref, orfs, specs = cli_case()
    rd = mc.arrays(specs)
    y = my.counts(rd, mc.FUZZ_L)
    fwd, rev, ev = rm.walked(rd, y)
    bamwriter.write_bam("A.bam", rd, refs=mc.FUZZ_REFS, block=4096)
    common = cr.setup_cli(ref, orfs)
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + ["-o", "s.fa", "--mate-overlap", "--variant-table", "s.var", "--variant-strand",
                             "--variant-evidence", "s.ev", "--stats", "s.json"])
    refb = ref.encode()
    recs = vy.records(y["counts"], refb, 3, 100, 1, 10)                     # (the command line's defaults)
    assert len(recs) > 10
    strand = {p: (fwd[p], rev[p]) for p, _, _, _ in recs}
    assert open("s.var").read() == engine.VARIANTS_STRAND_HEADER + sty.text(recs, strand, "ref", refb, 10, 1, 10)
    evd = {p: (ev["n"][p], ev["qual"][p], ev["mapq"][p], ev["dist"][p]) for p, _, _, _ in recs}
    assert open("s.ev").read() == engine.VARIANTS_EVIDENCE_HEADER + ey.text(recs, evd, "ref", refb, 20, 20, 5)
    st = json.load(open("s.json"))
    assert st["mate_overlap"] is True and st["mate_pairs"] == y["counters"]["pairs"] and st["variant_records"] == len(recs)


# ---- refusals through the ABI ----------------------------------------------------------------------------------------------------------------------
def refused(call):
    with pytest.raises(_ffi.TcmiError) as e:
        call()
    assert e.value.code == _ffi.E_UNSUPPORTED and "--mate-overlap" in str(e.value), str(e.value)
    return str(e.value)


def test_block_ranges_and_flat_arrays_are_refused(ctx, store):
    path, rd = data(store, "seed11")
    n_pos = mc.FUZZ_L + 700
    d = engine.DeviceBam(path)
    ctx.set_mate_overlap(True)
    try:
        assert d.n_blocks >= 3
        for blocks in ((0, d.n_blocks - 1), (1, -1), (1, 1)):
            refused(lambda: ctx.upload_bamfile(d, blocks))
        ctx.upload_bamfile(d, (0, d.n_blocks)).free()                                           # (the whole file as a range is the whole file)
        for call in (lambda: ctx.upload(rd), lambda: ctx.tally(rd, L=n_pos), lambda: ctx.upload_batch([rd, rd], 4096)):
            refused(call)
        with pytest.raises(_ffi.TcmiError) as e:
            _ffi.check(_ffi.lib().tcmi_ctx_set_mate_overlap(ctx.handle, 2), ctx.handle)     # (on is 0 or 1)
        assert e.value.code == _ffi.E_ARG
    finally:
        ctx.set_mate_overlap(False)
        d.close()
    assert np.array_equal(ctx.tally(rd, L=n_pos)[:mc.FUZZ_L], my.counts(rd, mc.FUZZ_L, mate=False)["counts"][:mc.FUZZ_L])     # (usable afterwards)


def test_split_step_is_refused_and_tallies_nothing(store):
    """tcmi_split_step: refused before anything is queued; the matrix stays as it was"""
    import torch
    path, _ = data(store, "seed11")
    n_pos = mc.FUZZ_L + 700
    ld, n_words = distributed.split_words(n_pos, 1)
    d = engine.DeviceBam(path)
    sctx = engine.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    try:
        sctx.set_mate_overlap(True)
        t = torch.zeros(n_words, dtype=torch.int32, device="cuda")
        hook = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)(lambda user, p, n, s: 0)
        rc, rs, planes = distributed._split_step(sctx, d, 0, 1, n_pos, ld, t, 10, True, hook, None)
        said = (_ffi.lib().tcmi_last_error(sctx.handle) or b"").decode()
        torch.cuda.synchronize()
        assert rc == _ffi.E_UNSUPPORTED and rs is None and "--mate-overlap" in said and not bool(t.any()), (rc, said)
    finally:
        sctx.close()
        d.close()


def test_array_pipeline_is_refused(store):
    _, rd = data(store, "seed11")
    p = engine.Pipeline(device=0, slots=2, walkers=1)
    try:
        rs = p.ctx.upload(rd)
        p.ctx.set_mate_overlap(True)
        refused(lambda: p.run([rs], mc.FUZZ_L + 700, 10, True))
        p.ctx.set_mate_overlap(False)
        rs.free()
    finally:
        p.close()


def test_file_runner_refuses_the_host_reader_fallback(ctx, store):
    path, _ = data(store, "seed11")
    _, orfs = sy.make_reference(L=600, cds=[(50, 500)])
    rows = [{"start": o["start"], "end": o["end"], "strand": "+"} for o in orfs]
    runner = engine.FileRunner(ctx, rows, 10, gpu_streams=1, rules=engine.ReadRules(mate_overlap=True))
    try:
        runner.device_decode = False
        said = refused(lambda: runner.run([path], names=["s"], ref_len=mc.FUZZ_L))
        assert "--mate-overlap needs the device path (the host packer knows no mate join), which this file left" in said and path in said, said
        assert list(runner.last_status) == [_ffi.E_UNSUPPORTED] and runner.decoded_on == {"device": 0, "host": 0}
    finally:
        runner.close()


# ---- the command line --------------------------------------------------------------------------------------------------------------------------------
def cli_case():
    ref, orfs = sy.make_reference(seed=3, L=mc.FUZZ_L, cds=[(100, 900), (1100, 1900)])
    return ref, orfs, mc.fuzz_specs(21, n_pairs=700, ref=ref)


def test_cli_single_sample_and_batch(tmp_path, monkeypatch):
    """-i --mate-overlap --variant-table: -doc is the yardstick's coverage; FASTA, VCF, GFF and the table equal the run WITHOUT the flag
    whose counts --index-override replaces by the yardstick's matrix.  --batch (two samples) equals -i."""
    monkeypatch.chdir(tmp_path)
    ref, orfs, specs = cli_case()
    rd = mc.arrays(specs)
    y = my.counts(rd, mc.FUZZ_L)
    want = y["counts"]
    assert len(want) == mc.FUZZ_L and y["counters"]["clipped_reads"] >= 100
    bamwriter.write_bam("A.bam", rd, refs=mc.FUZZ_REFS, block=4096)
    bamwriter.write_bam("A2.bam", rd, refs=mc.FUZZ_REFS, block=4096, split_records=True)
    common = cr.setup_cli(ref, orfs)
    cr.write_override("o.csv.gz", want)
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + cr.out_args("a") + ["--mate-overlap", "--variant-table", "a.var", "--stats", "a.json"])
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + cr.out_args("b") + ["--index-override", "o.csv.gz", "--variant-table", "b.var", "--stats", "b.json"])
    assert cr.doc_column("a.tsv") == want[:, 0].tolist()
    assert cr.outputs("a") == cr.outputs("b") and open("a.var").read() == open("b.var").read() and open("a.var").read().count("\n") > 10
    sa, sb = json.load(open("a.json")), json.load(open("b.json"))
    c = y["counters"]
    assert {k: sa[k] for k in ("mate_overlap", "mate_pairs", "reads_mate_clipped", "columns_mate_clipped", "mate_ambiguous")} == \
        {"mate_overlap": True, "mate_pairs": c["pairs"], "reads_mate_clipped": c["clipped_reads"], "columns_mate_clipped": c["clipped_columns"], "mate_ambiguous": c["ambiguous"]}
    assert sb["mate_overlap"] is False and sb["mate_pairs"] == 0
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + ["-o", "raw.fa", "-doc", "raw.tsv"])       # (the process's context is back at off)
    assert cr.doc_column("raw.tsv") == my.counts(rd, mc.FUZZ_L, mate=False)["counts"][:, 0].tolist()
    with open("m.tsv.in", "w") as fh:
        for k, bam in enumerate(("A.bam", "A2.bam")):
            fh.write("\t".join([bam, "S"] + ["m%d.%s" % (k, e) for e in ("fa", "vcf", "gff", "tsv", "var")]) + "\n")
    cr.run_cli(monkeypatch, ["--batch", "m.tsv.in"] + common + ["--mate-overlap", "--stats", "m.json"])
    for k in (0, 1):
        assert cr.outputs("m%d" % k) == cr.outputs("a") and open("m%d.var" % k).read() == open("a.var").read(), k
    sm = json.load(open("m.json"))
    assert sm["mate_overlap"] is True and sm["mate_pairs"] == 2 * c["pairs"] and sm["columns_mate_clipped"] == 2 * c["clipped_columns"]


def test_cli_per_contig(tmp_path, monkeypatch):
    """--per-contig --mate-overlap: pairs never cross contigs; per contig, -doc is the yardstick's coverage and the FASTA record and the
    table's rows equal the single run of that contig's records alone."""
    monkeypatch.chdir(tmp_path)
    refs = [("c0", 1500), ("c1", 1200)]
    recs, rows, specs = [], [], []
    for t, (name, ln) in enumerate(refs):
        ref, orfs = sy.make_reference(seed=30 + t, L=ln, cds=[(100, 700)])
        recs.append((name, ref))
        rows.append((name, orfs))
        specs += mc.fuzz_specs(40 + t, n_pairs=300, n_single=40, ref_len=ln, tid=t, ref=ref)
    bamwriter.write_bam("A.bam", mc.arrays(specs), refs=refs, block=4096)
    cr.setup_contigs(recs, rows)
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-ref", "r.fa", "-gff", "g.gff", "-cov", "10", "-name", "S", "-o", "a.fa", "-doc", "a.tsv",
                             "--per-contig", "--mate-overlap", "--variant-table", "a.var", "--stats", "a.json"])
    want_fa, want_tsv, want_var, pairs = "", "", "", 0
    for t, (name, ln) in enumerate(refs):
        rd = mc.arrays(mc.on_reference_0(specs, t))
        y = my.counts(rd, ln)
        pairs += y["counters"]["pairs"]
        bamwriter.write_bam("one%d.bam" % t, rd, refs=[(name, ln), ("elsewhere", 100)], block=4096)
        open("r%d.fa" % t, "w").write(">%s\n%s\n" % recs[t])
        open("g%d.gff" % t, "w").write("##gff-version 3\n" + sy.gff_text(rows[t][1], seqid=name)[1])
        cr.run_cli(monkeypatch, ["-i", "one%d.bam" % t, "-ref", "r%d.fa" % t, "-gff", "g%d.gff" % t, "-cov", "10", "-name", "S_" + name,
                                 "-o", "one%d.fa" % t, "-doc", "one%d.tsv" % t, "--mate-overlap", "--variant-table", "one%d.var" % t])
        assert cr.doc_column("one%d.tsv" % t) == y["counts"][:, 0].tolist()
        want_fa += open("one%d.fa" % t).read()
        want_tsv += "".join("%s\t%s" % (name, line) for line in open("one%d.tsv" % t))
        want_var += "".join(ln_ for k, ln_ in enumerate(open("one%d.var" % t)) if k or not t)
    assert open("a.fa").read() == want_fa and want_fa.count(">") == 2
    assert open("a.tsv").read() == want_tsv and open("a.var").read() == want_var
    st = json.load(open("a.json"))
    assert st["mate_overlap"] is True and st["mate_pairs"] == pairs > 100
