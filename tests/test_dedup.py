"""--dedup on the GPU (csrc/dedup.hip, the mate join's mate_idx, and what takes clip[] along): both packers against the yardstick
(tests/dedup_yardstick.py) on the hand-made cases and two fuzz seeds — plain, under a floor, a primer table, a read filter, each with
the mate rule off and on —; the setting off; duplicate sets and pairs across BGZF blocks, two uploads, another file order; one key with
20 000 templates; a file past one trip of the kernels' grid; long reads; the stream-walking tables; the refusals through the ABI; the
command line.  The rule's text and what the fuzz holds: tests/test_dedup_rule.py."""
import ctypes as C
import contextlib
import json

import numpy as np
import pytest

from tests import cli_run as cr
from tests import dedup_big as db
from tests import dedup_cases as dc
from tests import dedup_yardstick as dy
from tests import device_file as dvf
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
DATA = ("cases",) + tuple("seed%d" % s for s in dc.FUZZ_SEEDS)
# mode -> (primer table, floor, read filter)
MODES = {"plain": ((), 0, dy.NONE), "floor": ((), dc.FLOOR, dy.NONE), "primers": (SCHEME, 0, dy.NONE), "filter": ((), 0, dc.FILTER)}
SC_BLOCK, SC_WG_PER_CU = rb.stream_count_caps()
OFF = dict.fromkeys(("on",) + dy.COUNTERS, 0)


@pytest.fixture(scope="module")
def ctx():
    with engine.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    """the module's directory, the files written once and the yardsticks computed once: {key: value}"""
    return {"dir": tmp_path_factory.mktemp("dedup")}


def once(store, key, make):
    if key not in store:
        store[key] = make()
    return store[key]


def specs_of(key):
    return dc.cases() if key == "cases" else dc.fuzz_specs(int(key[4:]))


def data(store, key):
    """-> (path, flat arrays) of the case file / a fuzz seed's file"""
    def make():
        rd = dc.arrays(specs_of(key))
        path = str(store["dir"] / (key + ".bam"))
        bamwriter.write_bam(path, rd, refs=dc.REFS if key == "cases" else dc.FUZZ_REFS, block=4096)
        return path, rd
    return once(store, ("data", key), make)


def yard(store, key, mode, mate=False, dedup=True):
    primers, q, f = MODES[mode]
    return once(store, ("yard", key, mode, mate, dedup), lambda: dy.counts(data(store, key)[1], dc.L, primers, q, f=f, mate=mate, dedup=dedup))


@contextlib.contextmanager
def uploaded(ctx, path, mode="plain", how=None, mate=False, dedup=True):
    """device_file.uploaded with the duplicate rule (and the mate rule) on for the upload alone: the read set must remember them"""
    primers, q, f = MODES[mode]
    ctx.set_mate_overlap(mate)
    ctx.set_dedup(dedup)
    try:
        with dvf.uploaded(ctx, path, primers, q, f, how=how) as rs:
            ctx.set_mate_overlap(False)
            ctx.set_dedup(False)
            yield rs
    finally:
        ctx.set_mate_overlap(False)
        ctx.set_dedup(False)


def check(ctx, rs, y, mate=False):
    got = ctx.step(rs, len(y["counts"]), 0, True)[3]
    bad = np.argwhere(got != y["counts"])
    assert len(bad) == 0, (len(bad), bad[:6].tolist(), got[tuple(bad[:6].T)].tolist(), y["counts"][tuple(bad[:6].T)].tolist())
    assert rs.dedup == dict(y["dedup_counters"], on=1), (rs.dedup, y["dedup_counters"])
    assert rs.mate_overlap == dict(y["counters"], on=int(mate)), (rs.mate_overlap, y["counters"])
    assert (rs.n_piled, rs.max_end, rs.primer_masked_reads) == (y["n_piled"], y["max_end"], y["n_masked"])
    dup = rs.duplicates()
    assert dup.dtype == bool and np.array_equal(dup, y["dup"]), np.flatnonzero(dup != y["dup"])[:10].tolist()


# ---- 1. packers and planes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mate", (False, True))
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("how", dvf.PACKERS)
@pytest.mark.parametrize("key", DATA)
def test_both_packers_equal_the_yardstick(ctx, store, key, how, mode, mate):
    path, _ = data(store, key)
    y = yard(store, key, mode, mate)
    assert y["dedup_counters"]["duplicate_records"] > 0
    assert not np.array_equal(y["counts"], yard(store, key, mode, mate, dedup=False)["counts"])
    with uploaded(ctx, path, mode, how, mate) as rs:
        assert rs.route == how
        check(ctx, rs, y, mate)


# ---- 2. the setting off ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("plain", "floor", "primers"))
@pytest.mark.parametrize("how", dvf.PACKERS)
def test_setting_off_is_the_existing_yardstick(ctx, store, how, mode):
    key = "seed%d" % dc.FUZZ_SEEDS[0]
    path, rd = data(store, key)
    primers, q, _ = MODES[mode]
    want = py.counts(rd, dc.FUZZ_L, primers, q)
    with uploaded(ctx, path, mode, how, dedup=False) as rs:
        got = ctx.step(rs, len(want[0]), 0, True)[3]
        assert np.array_equal(got, want[0]) and rs.dedup == OFF
        assert rs.mate_overlap == dict(on=0, pairs=0, clipped_reads=0, clipped_columns=0, ambiguous=0)
        assert rs.primer_masked_reads == want[1]
        with pytest.raises(_ffi.TcmiError) as e:
            rs.duplicates()
        assert e.value.code == _ffi.E_UNSUPPORTED
    assert not np.array_equal(want[0], yard(store, key, mode)["counts"])           # (the file for which test 1 asserts the other matrix)
    ym = my.counts(rd, dc.FUZZ_L, primers, q)                                       # the mate rule alone: exactly as before
    with uploaded(ctx, path, mode, how, mate=True, dedup=False) as rs:
        assert np.array_equal(ctx.step(rs, len(ym["counts"]), 0, True)[3], ym["counts"]) and rs.dedup == OFF
        assert rs.mate_overlap == dict(ym["counters"], on=1)


# ---- 3. across blocks, two uploads, another file order ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", dvf.PACKERS)
def test_across_blocks_two_uploads_and_file_order(ctx, store, how):
    block = 4096
    sorted_specs = dc.fuzz_specs(dc.FUZZ_SEEDS[1])

    def make():
        specs = dc.permuted(sorted_specs, 7)
        rd = dc.arrays(specs)
        path = str(store["dir"] / "permuted.bam")
        bamwriter.write_bam(path, rd, refs=dc.FUZZ_REFS, block=block, split_records=True)
        return path, rd, specs, dy.counts(rd, dc.FUZZ_L, mate=True)
    path, rd, specs, y = once(store, "permuted", make)
    _, rec = dvf.host_stream_and_records(path)
    blk = (rec // block).astype(np.int64)                       # (block b holds bytes [4096 b, 4096 b + 4096) of the stream)
    v = y["verdicts"]
    apart = [ts for ts in v["templates"].values() if len(ts) >= 2 and len({int(blk[i]) for t in ts for i in t[2]}) >= 2]
    pair_apart = [t for ts in v["templates"].values() for t in ts if len(t[2]) == 2 and blk[t[2][0]] != blk[t[2][1]]]
    assert len(apart) >= 20 and len(pair_apart) >= 20 and any(len(ts) >= 2 for ts in v["templates"].values() if any(t in pair_apart for t in ts))
    dups = []
    for _ in range(2):
        with uploaded(ctx, path, "plain", how, mate=True) as rs:
            check(ctx, rs, y, mate=True)
            dups.append(rs.duplicates())
    assert np.array_equal(dups[0], dups[1])
    # the same records in the sorted order: the same templates, another winner where scores tie
    ys = yard(store, "seed%d" % dc.FUZZ_SEEDS[1], "plain", True)
    assert ys["dedup_counters"] == y["dedup_counters"]
    ident = lambda r: (r["name"], r["flag"], r["pos"], r["cigar"], tuple(r["qual"]))
    a = {ident(r) for i, r in enumerate(sorted_specs) if ys["dup"][i]}
    b = {ident(r) for i, r in enumerate(specs) if dups[0][i]}
    assert a != b and len(a ^ b) >= 4


# ---- 4. one key, many templates ---------------------------------------------------------------------------------------------------------------
def test_one_key_with_many_templates(ctx, store):
    """20 000 fragments of 30 bases at one place — 30 qualities cannot give 20 000 distinct scores (30 x 93 < 20 000): they are as
    distinct as they can be and ONE is the best, in the middle of the set — next to 20 000 fragments at 20 000 places.  A lane's work
    must not grow with its key's templates, and 64 lanes on one slot are one atomic: a chain over members would not end in seconds."""
    n_each = 20000
    path = str(store["dir"] / "one_key.bam")
    dup, cov, L = once(store, "one_key", lambda: db.one_key_and_distinct(path, n_each))
    assert int((~dup[:n_each]).sum()) == 1 and not dup[n_each:].any()
    for how in dvf.PACKERS:
        with uploaded(ctx, path, "plain", how) as rs:
            assert rs.route == how and rs.n_reads == 2 * n_each == rs.n_piled
            assert rs.dedup == dict(on=1, templates=2 * n_each, duplicate_templates=n_each - 1, duplicate_records=n_each - 1, duplicate_sets=1)
            assert np.array_equal(rs.duplicates(), dup)
            got = ctx.step(rs, L, 0, True)[3]
            assert np.array_equal(got[:, 0], cov), np.flatnonzero(got[:, 0] != cov)[:6].tolist()


# ---- 5. past one trip of the kernels' grid ------------------------------------------------------------------------------------------------------
def test_past_one_trip_of_the_grid(ctx, store):
    cap = ctx.stat("compute_units") * SC_WG_PER_CU * SC_BLOCK
    n = cap + 257
    rd = mb.generate(n)
    path = mb.write(store["dir"] / "big.bam", rd)
    dup, cnt = db.verdicts(rd)
    clip, mcnt = mb.join(rd)
    assert cnt["duplicate_sets"] > 1000 and dup[cap:].any() and not dup[cap:].all()          # (the ragged second trip has both)
    want = mb.matrix(rd, mb.L, np.where(dup, mb.LEN, clip))
    for how in dvf.PACKERS:
        with uploaded(ctx, path, "plain", how, mate=True) as rs:
            assert rs.n_reads == n and rs.dedup == dict(cnt, on=1), (rs.dedup, cnt)
            assert rs.mate_overlap == dict(mcnt, on=1)
            assert np.array_equal(rs.duplicates(), dup)
            got = ctx.step(rs, mb.L, 0, True)[3]
            assert np.array_equal(got, want), np.argwhere(got != want)[:6].tolist()


# ---- 6. long reads -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", dvf.PACKERS)
def test_long_reads(ctx, store, how):
    """reference spans beyond what the packed set takes (1 200 columns): tally_stream_kernel walks them in the stream, under clip[]"""
    def make():
        rng = np.random.default_rng(5)
        specs = [dc._frag(rng, "long_a", 0, 100, "50M1100N50M", 20, True), dc._frag(rng, "long_b", 0, 100, "50M1100N50M", 30, False),
                 dc._frag(rng, "long_c", 0, 103, "3S47M1100N50M", 25, True), dc._frag(rng, "long_rev", 16, 100, "50M1100N50M", 10, False),
                 dc._frag(rng, "short_a", 0, 300, "50M", 30, False), dc._frag(rng, "short_b", 0, 305, "5S45M", 20, True)]
        rd = dc.arrays(specs)
        path = str(store["dir"] / "long.bam")
        bamwriter.write_bam(path, rd, refs=[("ref", 1400)], block=4096)
        return path, rd, specs, dy.counts(rd, 1400)
    path, rd, specs, y = once(store, "long", make)
    assert [bool(x) for x in y["dup"]] == [r["dup"] for r in specs] and y["max_end"] == 1300
    with uploaded(ctx, path, "plain", how) as rs:
        check(ctx, rs, y)


# ---- 7. the tables that walk the records, under the rule ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mate", (False, True))
@pytest.mark.parametrize("how", dvf.PACKERS)
def test_strand_and_evidence_counts_under_the_rule(ctx, store, how, mate):
    path, rd = data(store, "cases")
    mode = "floor"
    primers, q, f = MODES[mode]
    y = yard(store, "cases", mode, mate)
    n_pos = len(y["counts"])
    cols = np.arange(n_pos)
    fwd, rev, ev = once(store, ("walked", mode, mate), lambda: rm.walked(rd, y, primers, q, f))
    with uploaded(ctx, path, mode, how, mate) as rs:
        matrix = ctx.step(rs, n_pos, 0, True)[3]
        sc = ctx.strand_counts(rs, cols)
        assert np.array_equal(sc["fwd"] + sc["rev"], matrix)                # (what the writer checks: else no table)
        assert np.array_equal(sc["fwd"], fwd) and np.array_equal(sc["rev"], rev)
        ec = ctx.evidence_counts(rs, cols)
        assert np.array_equal(ec["n"], matrix)
        for k in ("qual", "mapq", "dist"):
            assert np.array_equal(ec[k], ev[k]), k


# ---- 8. refusals through the ABI ---------------------------------------------------------------------------------------------------------------------
def refused(call):
    with pytest.raises(_ffi.TcmiError) as e:
        call()
    assert e.value.code == _ffi.E_UNSUPPORTED and "--dedup" in str(e.value), str(e.value)
    return str(e.value)


def test_block_ranges_and_flat_arrays_are_refused(ctx, store):
    path, rd = data(store, "seed%d" % dc.FUZZ_SEEDS[0])
    n_pos = dc.FUZZ_L + 700
    d = engine.DeviceBam(path)
    ctx.set_dedup(True)
    try:
        assert d.n_blocks >= 3
        for blocks in ((0, d.n_blocks - 1), (1, -1), (1, 1)):
            refused(lambda: ctx.upload_bamfile(d, blocks))
        first = ctx.upload_bamfile(d, (0, d.n_blocks))                                          # (the whole file as a range is the whole file)
        assert first.dedup["on"] == 1 and first.duplicates().any()
        second = ctx.upload_bamfile(d)
        with pytest.raises(_ffi.TcmiError) as e:                                                # (the verdicts lie beside the stream: gone with it)
            first.duplicates()
        assert e.value.code == _ffi.E_UNSUPPORTED and "no longer" in str(e.value)
        assert second.duplicates().any()
        first.free()
        second.free()
        for call in (lambda: ctx.upload(rd), lambda: ctx.tally(rd, L=n_pos), lambda: ctx.upload_batch([rd, rd], 4096)):
            refused(call)
        with pytest.raises(_ffi.TcmiError) as e:
            _ffi.check(_ffi.lib().tcmi_ctx_set_dedup(ctx.handle, 2), ctx.handle)            # (on is 0 or 1)
        assert e.value.code == _ffi.E_ARG
    finally:
        ctx.set_dedup(False)
        d.close()
    assert np.array_equal(ctx.tally(rd, L=n_pos)[:dc.FUZZ_L], my.counts(rd, dc.FUZZ_L, mate=False)["counts"][:dc.FUZZ_L])     # (usable afterwards)


def test_split_step_is_refused_and_tallies_nothing(store):
    """tcmi_split_step: refused before anything is queued; the matrix stays as it was"""
    import torch
    path, _ = data(store, "seed%d" % dc.FUZZ_SEEDS[0])
    n_pos = dc.FUZZ_L + 700
    ld, n_words = distributed.split_words(n_pos, 1)
    d = engine.DeviceBam(path)
    sctx = engine.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    try:
        sctx.set_dedup(True)
        t = torch.zeros(n_words, dtype=torch.int32, device="cuda")
        hook = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)(lambda user, p, n, s: 0)
        rc, rs, planes = distributed._split_step(sctx, d, 0, 1, n_pos, ld, t, 10, True, hook, None)
        said = (_ffi.lib().tcmi_last_error(sctx.handle) or b"").decode()
        torch.cuda.synchronize()
        assert rc == _ffi.E_UNSUPPORTED and rs is None and "--dedup" in said and not bool(t.any()), (rc, said)
    finally:
        sctx.close()
        d.close()


def test_array_pipeline_is_refused(store):
    _, rd = data(store, "seed%d" % dc.FUZZ_SEEDS[0])
    p = engine.Pipeline(device=0, slots=2, walkers=1)
    try:
        rs = p.ctx.upload(rd)
        p.ctx.set_dedup(True)
        refused(lambda: p.run([rs], dc.FUZZ_L + 700, 10, True))
        p.ctx.set_dedup(False)
        rs.free()
    finally:
        p.close()


def test_file_runner_refuses_the_host_reader_fallback(ctx, store):
    path, _ = data(store, "seed%d" % dc.FUZZ_SEEDS[0])
    _, orfs = sy.make_reference(L=600, cds=[(50, 500)])
    rows = [{"start": o["start"], "end": o["end"], "strand": "+"} for o in orfs]
    runner = engine.FileRunner(ctx, rows, 10, gpu_streams=1, rules=engine.ReadRules(dedup=True))
    try:
        runner.device_decode = False
        said = refused(lambda: runner.run([path], names=["s"], ref_len=dc.FUZZ_L))
        assert "--dedup needs the device path (the host packer knows no duplicate templates), which this file left" in said and path in said, said
        assert list(runner.last_status) == [_ffi.E_UNSUPPORTED] and runner.decoded_on == {"device": 0, "host": 0}
    finally:
        runner.close()


# ---- 9. the command line ---------------------------------------------------------------------------------------------------------------------------
STAT_KEYS = ("dedup", "dedup_templates", "duplicate_templates", "duplicate_records", "duplicate_sets")


def stats_of(c, times=1):
    return {"dedup": True, "dedup_templates": times * c["templates"], "duplicate_templates": times * c["duplicate_templates"],
            "duplicate_records": times * c["duplicate_records"], "duplicate_sets": times * c["duplicate_sets"]}


def cli_case():
    ref, orfs = sy.make_reference(seed=3, L=dc.FUZZ_L, cds=[(100, 900), (1100, 1900)])
    return ref, orfs, dc.fuzz_specs(41, n_pairs=500, n_sets=240, ref=ref)


def test_cli_single_sample_and_batch(tmp_path, monkeypatch):
    """-i --dedup --variant-table --variant-strand --variant-evidence: -doc is the yardstick's coverage; FASTA, VCF, GFF and the table equal
    the run WITHOUT the flag whose counts --index-override replaces by the yardstick's matrix, and differ from the run without either;
    both record-stream tables come out (their sums matched the matrix).  --batch (two samples) equals -i."""
    monkeypatch.chdir(tmp_path)
    ref, orfs, specs = cli_case()
    rd = dc.arrays(specs)
    y = dy.counts(rd, dc.FUZZ_L)
    want = y["counts"]
    assert len(want) == dc.FUZZ_L and y["dedup_counters"]["duplicate_records"] >= 300
    bamwriter.write_bam("A.bam", rd, refs=dc.FUZZ_REFS, block=4096)
    bamwriter.write_bam("A2.bam", rd, refs=dc.FUZZ_REFS, block=4096, split_records=True)
    common = cr.setup_cli(ref, orfs)
    cr.write_override("o.csv.gz", want)
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + cr.out_args("a") + ["--dedup", "--variant-table", "a.var", "--stats", "a.json"])
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + cr.out_args("b") + ["--index-override", "o.csv.gz", "--variant-table", "b.var", "--stats", "b.json"])
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + cr.out_args("raw"))       # (the process's context is back at off)
    assert cr.doc_column("a.tsv") == want[:, 0].tolist()
    assert cr.outputs("a") == cr.outputs("b") and open("a.var").read() == open("b.var").read() and open("a.var").read().count("\n") > 10
    assert cr.doc_column("raw.tsv") == dy.counts(rd, dc.FUZZ_L, dedup=False)["counts"][:, 0].tolist() and cr.outputs("raw") != cr.outputs("a")
    sa, sb = json.load(open("a.json")), json.load(open("b.json"))
    assert {k: sa[k] for k in STAT_KEYS} == stats_of(y["dedup_counters"]) and sa["mate_overlap"] is False and sa["mate_pairs"] == 0
    assert {k: sb[k] for k in STAT_KEYS} == {"dedup": False, "dedup_templates": 0, "duplicate_templates": 0, "duplicate_records": 0, "duplicate_sets": 0}
    # the record-stream tables under the rule, with the mate rule too
    ym = dy.counts(rd, dc.FUZZ_L, mate=True)
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + ["-o", "s.fa", "-doc", "s.tsv", "--dedup", "--mate-overlap", "--variant-table", "s.var",
                             "--variant-strand", "--variant-evidence", "s.ev", "--stats", "s.json"])
    assert cr.doc_column("s.tsv") == ym["counts"][:, 0].tolist()
    assert open("s.var").read().count("\n") > 10 and open("s.ev").read().count("\n") > 10
    ss_ = json.load(open("s.json"))
    assert {k: ss_[k] for k in STAT_KEYS} == stats_of(ym["dedup_counters"]) and ss_["mate_pairs"] == ym["counters"]["pairs"] > 0
    with open("m.tsv.in", "w") as fh:
        for k, bam in enumerate(("A.bam", "A2.bam")):
            fh.write("\t".join([bam, "S"] + ["m%d.%s" % (k, e) for e in ("fa", "vcf", "gff", "tsv", "var")]) + "\n")
    cr.run_cli(monkeypatch, ["--batch", "m.tsv.in"] + common + ["--dedup", "--stats", "m.json"])
    for k in (0, 1):
        assert cr.outputs("m%d" % k) == cr.outputs("a") and open("m%d.var" % k).read() == open("a.var").read(), k
    sm = json.load(open("m.json"))
    assert {k: sm[k] for k in STAT_KEYS} == stats_of(y["dedup_counters"], 2)


def test_cli_per_contig(tmp_path, monkeypatch):
    """--per-contig --dedup on a two-contig file whose contigs hold the SAME records (the same keys on two references: neither sees the
    other): per contig, -doc is the yardstick's coverage and the FASTA record equals the single run of that contig's records alone."""
    monkeypatch.chdir(tmp_path)
    refs = [("c0", 1500), ("c1", 1500)]
    ref, orfs = sy.make_reference(seed=30, L=1500, cds=[(100, 700)])
    recs, rows, specs = [], [], []
    for t, (name, ln) in enumerate(refs):
        recs.append((name, ref))
        rows.append((name, orfs))
        specs += dc.fuzz_specs(50, n_pairs=200, n_single=40, n_sets=120, ref_len=ln, tid=t, ref=ref)
    bamwriter.write_bam("A.bam", dc.arrays(specs), refs=refs, block=4096)
    cr.setup_contigs(recs, rows)
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-ref", "r.fa", "-gff", "g.gff", "-cov", "10", "-name", "S", "-o", "a.fa", "-doc", "a.tsv",
                             "--per-contig", "--dedup", "--stats", "a.json"])
    want_fa, want_tsv, total = "", "", dict.fromkeys(dy.COUNTERS, 0)
    for t, (name, ln) in enumerate(refs):
        rd = dc.arrays(mc.on_reference_0(specs, t))
        y = dy.counts(rd, ln)
        assert y["dedup_counters"]["duplicate_records"] > 100
        for k in dy.COUNTERS:
            total[k] += y["dedup_counters"][k]
        bamwriter.write_bam("one%d.bam" % t, rd, refs=[(name, ln), ("elsewhere", 100)], block=4096)
        open("r%d.fa" % t, "w").write(">%s\n%s\n" % recs[t])
        open("g%d.gff" % t, "w").write("##gff-version 3\n" + sy.gff_text(rows[t][1], seqid=name)[1])
        cr.run_cli(monkeypatch, ["-i", "one%d.bam" % t, "-ref", "r%d.fa" % t, "-gff", "g%d.gff" % t, "-cov", "10", "-name", "S_" + name,
                                 "-o", "one%d.fa" % t, "-doc", "one%d.tsv" % t, "--dedup"])
        assert cr.doc_column("one%d.tsv" % t) == y["counts"][:, 0].tolist()
        want_fa += open("one%d.fa" % t).read()
        want_tsv += "".join("%s\t%s" % (name, line) for line in open("one%d.tsv" % t))
    assert open("a.fa").read() == want_fa and want_fa.count(">") == 2
    assert open("a.tsv").read() == want_tsv
    st = json.load(open("a.json"))
    assert {k: st[k] for k in STAT_KEYS} == stats_of(total)
