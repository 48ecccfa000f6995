"""GPU: the records of tests/odd_cigars.py — CIGARs that are well-formed as bytes but not as an alignment — through both device packers
and every kernel that walks a record.  The tolerated files (four seeds, the hand-made list) in three modes against the existing
yardsticks: the step's matrix and call rows, strand and evidence counts, link counts (staged and in memory), codon counts at two
frames, indel events under two sets of thresholds, amplicon reads, the modal tokens, each table's "adds up to the matrix"; one seed
under --mate-overlap, one under --dedup, one under both; tally_variant 1 and the flat-array upload on both packers.  The large but
legal query totals alone and past one trip of the record grid.  The refused files (csrc/cigar_rule.h: a kept record with a query total
of 2^29 or more): refused by both packers, the flat-array upload and tcmi_split_step wherever the liar lies, the context usable
afterwards, the liar accepted where it is ignored anyway.  The command line.  Every comparison is exact equality.
The refused records were never run against a build without the rule: that such a record sends a 32-bit query index out of the record
was found by reading the walkers (DESIGN.md "CIGARs no aligner writes")."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from oracle import c_oracle
from tests import amplicon_reads_cases as arc
from tests import amplicon_reads_yardstick as ry
from tests import cli_run as cr
from tests import codon_cases as cc
from tests import codon_yardstick as cy
from tests import dedup_yardstick as dy
from tests import device_file as dvf
from tests import fuzz_masked as fm
from tests import indel_cases as ic
from tests import indel_yardstick as iy
from tests import link_cases as lkc
from tests import links_yardstick as ly
from tests import mate_overlap_cases as mc
from tests import mate_overlap_yardstick as my
from tests import odd_cigars as oc
from tests import read_specs as rs_
from tests import repeat_bam as rb
from tests import rules_marks as rm
from tests import schemes as sch
from tests import strand_yardstick as sty
from tests import variant_yardstick as vy
from trueconsense_amd import _ffi
from trueconsense_amd import distributed
from trueconsense_amd import engine
from trueconsense_amd import synthetic as sy
from trueconsense_amd.io import bamwriter

pytestmark = pytest.mark.gpu
NONE = dvf.NONE
RULES = rm.RULES
SC_BLOCK, SC_WG_PER_CU = rb.stream_count_caps()
MODE_NAMES = ("plain", "floor", "primers_filter")
REFUSALS = (_ffi.E_FORMAT, _ffi.E_UNSUPPORTED)


def mode_of(key, mode):
    """-> (primer table, floor, read filter): the modes of tests/test_stream_tables_under_rules.py; the table of a seed is the scheme's
    primers and the seed's own random ones, on whose mask edges the generator has put a fifth of the records"""
    own = list(fm.table_of(int(key[4:]))) if key.startswith("seed") else []
    return {"plain": ((), 0, NONE), "floor": ((), mc.FLOOR, NONE), "primers_filter": (list(sch.PRIMER_SCHEME) + own, 0, mc.FILTER)}[mode]


@pytest.fixture(scope="module")
def ctx():
    with engine.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    return {"dir": tmp_path_factory.mktemp("odd")}


def once(store, key, make):
    if key not in store:
        store[key] = make()
    return store[key]


def data(store, key):
    """-> (path, specs, flat arrays) of "seed<n>" or "hand" """
    def make():
        specs = oc.hand_specs() if key == "hand" else oc.seed_case(int(key[4:]))[0]
        rd = rs_.arrays(specs)
        path = str(store["dir"] / (key + ".bam"))
        bamwriter.write_bam(path, rd, ref_len=oc.L, block=4096)
        return path, specs, rd
    return once(store, ("data", key), make)


def yard(store, key, rule, mode):
    """the yardsticks of a file under a rule (None: neither) and a mode, computed once"""
    def make():
        _, specs, rd = data(store, key)
        primers, q, f = mode_of(key, mode)
        mate, dedup = RULES[rule] if rule else (False, False)
        y = dy.counts(rd, oc.L, primers, q, f=f, mate=mate, dedup=dedup)
        cls, ins = rm.marks(rd, y, primers, q, f=f)
        events, totals = rm.events(specs, rd, y, primers, q, f=f)
        fwd, rev, ev = rm.walked(rd, y, primers, q, f=f)
        return {"y": y, "cls": cls, "ins": ins, "events": events, "totals": totals, "fwd": fwd, "rev": rev, "ev": ev}
    return once(store, ("yard", key, rule, mode), make)


@contextlib.contextmanager
def uploaded(ctx, path, key, rule, mode, how):
    primers, q, f = mode_of(key, mode)
    mate, dedup = RULES[rule] if rule else (False, False)
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


def check_tables(ctx, rs, w, label, path=None, f=NONE, events=True):
    """every table of the read set against the yardsticks in w, each with its invariant on the step's matrix -> the matrix"""
    want = w["y"]["counts"]
    n_pos = len(want)
    plain, alt, flags, matrix = ctx.step(rs, n_pos, 30, True)
    bad = np.argwhere(matrix != want)
    assert len(bad) == 0, (label, len(bad), bad[:6].tolist(), matrix[bad[:6, 0]].tolist(), want[bad[:6, 0]].tolist())
    wp, wa, wf = c_oracle.call(want, 30, True)
    assert np.array_equal(plain, wp) and np.array_equal(alt, wa) and np.array_equal(flags, wf), (label, "call rows")
    cols = np.arange(n_pos)
    sc = ctx.strand_counts(rs, cols)
    assert np.array_equal(sc["fwd"] + sc["rev"], matrix), (label, "strand counts do not add up")
    assert np.array_equal(sc["fwd"], w["fwd"]) and np.array_equal(sc["rev"], w["rev"]), (label, "strand counts")
    ec = ctx.evidence_counts(rs, cols)
    assert np.array_equal(ec["n"], matrix), (label, "evidence counts do not add up")
    for k in ("qual", "mapq", "dist"):
        assert np.array_equal(ec[k], w["ev"][k]), (label, "evidence", k)
    rng = np.random.default_rng(len(str(label)))
    staged = sorted({int(c) for c in rng.choice(n_pos, 30, replace=False)} | {int(c) for c in np.argsort(matrix[:, 6])[-10:]})
    assert len(staged) * 2 <= lkc.LDS < 300 * 3
    for cols_k, k in ((staged, 2), (lkc.window_columns(want), 3)):
        got = lkc.device_links(ctx, rs, cols_k, k)
        msg = lkc.differ(got, ly.joint(w["cls"], cols_k, k), label + ("links", k))
        assert not msg, msg
        assert not ly.invariant(got, k, matrix), ly.invariant(got, k, matrix)
    c0s = cc.two_frames(want)
    assert len(c0s) == 100 > cc.LDS
    for q_c0 in (c0s, c0s[:cc.LDS]):
        got = cc.device_codons(ctx, rs, q_c0)
        msg = cc.differ(got, cy.joint(w["cls"], w["ins"], q_c0), label + ("codons", len(q_c0)))
        assert not msg, msg
        assert not cy.invariant(got, matrix), cy.invariant(got, matrix)
    if events:
        every = list(range(n_pos))
        cov = matrix[every, 0]
        for thresholds in (ic.EVERYTHING, ic.TENTH):
            want_ev = iy.reported(w["events"], every, cov, **thresholds)
            got, got_tot = ic.device_events(ctx, rs, every, cov, **thresholds)
            msg = ic.differ(got, want_ev, label + ("events", thresholds["num"]))
            assert not msg, msg
            assert np.array_equal(got_tot, iy.totals_at(w["totals"], every)), (label, "event totals")
            assert np.array_equal(got_tot["ins_total"], matrix[every, 6]), (label, "the insertions do not add up to the I plane")
    if path is not None:
        amps4 = arc.tiled(6)
        reads = arc.device_counts(ctx, rs, amps4, 0)
        assert np.array_equal(reads, ry.counts(arc.host_columns(path, read_filter=f if f != NONE else None), amps4, 0)), (label, "amplicon reads")
    return matrix


# ---- 1. the tolerated files ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODE_NAMES)
@pytest.mark.parametrize("how", dvf.PACKERS)
@pytest.mark.parametrize("key", ["seed%d" % s for s in oc.SEEDS] + ["hand"])
def test_tolerated_shapes_every_table(ctx, store, key, how, mode):
    path, specs, rd = data(store, key)
    w = yard(store, key, None, mode)
    if key != "hand":
        assert oc.fm.n_long(specs) >= 100                                       # tally_stream_kernel's share
    with uploaded(ctx, path, key, None, mode, how) as rs:
        assert rs.route == how and rs.n_reads == len(specs)
        matrix = check_tables(ctx, rs, w, (key, how, mode), path, mode_of(key, mode)[2])
        assert matrix[:, 5].sum() > 0 and matrix[:, 6].sum() > 0


@pytest.mark.parametrize("how", dvf.PACKERS)
@pytest.mark.parametrize("key", ["seed%d" % s for s in oc.SEEDS] + ["hand"])
def test_modal_tokens_of_the_tolerated_shapes(ctx, store, key, how):
    """ins_entries and the host's vote against the host sweep over the same records (64-bit, insert_tokens.cpp), at the forty columns
    with the most insertions and at both ends.  The device looks at no token of a long read (it says so and leaves the file to the
    host sweep), so the seeds go without their long records here — and on the seed's whole file the device must decline in those
    words, with TCMI_E_UNSUPPORTED, which is what sends the callers to the host sweep."""
    whole, specs, _ = data(store, key)
    short = [r for r in specs if oc.sums(oc.words_of(r))[0] <= oc.LONG]
    assert len(short) >= 100 and len({oc.class_of(r) for r in short}) == (1 if key == "hand" else len(oc.CLASSES))
    rd = rs_.arrays(short)
    path = str(store["dir"] / (key + "_short.bam"))
    bamwriter.write_bam(path, rd, ref_len=oc.L, block=4096)
    ins = c_oracle.tally(rd, oc.L)[:, 6]
    cols = sorted({int(c) + 1 for c in np.argsort(ins)[-40:]} | {1, oc.L})
    want = engine.modal_tokens(rd, cols)
    if key == "hand":                                                           # (two records a shape: the insertions are the modal tokens)
        assert sum(1 for t, _ in want.values() if t and "+" in t) >= 5
    else:
        assert sum(n for _, n in want.values()) > 100
    with dvf.uploaded(ctx, path, how=how) as rs:
        assert ctx.readset_modal_tokens(rs, cols) == want, (key, how)
    if key != "hand":
        with dvf.uploaded(ctx, whole, how=how) as rs:
            with pytest.raises(_ffi.TcmiError) as e:
                ctx.readset_modal_tokens(rs, cols)
            assert e.value.code == _ffi.E_UNSUPPORTED and "long reads" in str(e.value) and "host sweep" in str(e.value), str(e.value)


@pytest.mark.parametrize("key,rule", [("seed1", "mate"), ("seed2", "dedup"), ("seed3", "both")])
def test_tolerated_shapes_under_the_mate_and_duplicate_rules(ctx, store, key, rule):
    path, specs, rd = data(store, key)
    w, w0 = yard(store, key, rule, "plain"), yard(store, key, None, "plain")
    assert not np.array_equal(w["y"]["counts"], w0["y"]["counts"])
    if rule != "dedup":
        assert w["y"]["counters"]["clipped_reads"] >= 100
    if rule != "mate":
        assert w["y"]["dedup_counters"]["duplicate_records"] >= 100
    with uploaded(ctx, path, key, rule, "plain", "one_sync") as rs:
        check_tables(ctx, rs, w, (key, rule))
        if rule != "mate":
            assert np.array_equal(rs.duplicates(), w["y"]["dup"])


@pytest.mark.parametrize("seed", oc.SEEDS)
def test_tally_variant_1_and_the_flat_array_upload(ctx, store, seed):
    _, _, rd = data(store, "seed%d" % seed)
    want = yard(store, "seed%d" % seed, None, "plain")["y"]["counts"]
    try:
        for variant in (0, 1):
            ctx.set_option("tally_variant", variant)
            for device_pack in (0, 1):
                ctx.set_option("device_pack", device_pack)
                rs = ctx.upload(rd)
                try:
                    assert np.array_equal(ctx.step(rs, len(want), 0, True)[3], want), (variant, device_pack)
                finally:
                    rs.free()
    finally:
        ctx.set_option("tally_variant", 0)
        ctx.set_option("device_pack", 1)


# ---- 2. large but legal query totals -----------------------------------------------------------------------------------------------------------
def large_file(store):
    def make():
        specs = oc.large_specs()
        rd = rs_.arrays(specs)
        path = str(store["dir"] / "large.bam")
        bamwriter.write_bam(path, rd, ref_len=400, block=4096)
        return path, specs, rd
    return once(store, "large", make)


def large_reads(path):
    return ry.counts(arc.host_columns(path), [(90, 95, 260, 265), (90, 101, 140, 146)], 0)


def check_large(ctx, rs, specs, want_reads, times=1, q=0, clip=None):
    """the tables that never walk the bases of an insertion (an insertion of 2^29 bases is hashed base by base by the indel table and
    spelled out by the token vote: seconds of one lane's time, and nothing an address is formed from), each against the classes
    tests/odd_cigars.large_classes states by hand; times: every record that often in the file"""
    n_pos = 400
    cls, ins = oc.large_classes(specs, n_pos, q, clip)
    want = oc.large_matrix(specs, n_pos, q, clip)
    matrix = ctx.step(rs, n_pos, 0, True)[3]
    assert np.array_equal(matrix, times * want), np.argwhere(matrix != times * want)[:6].tolist()
    cols = np.arange(n_pos)
    rev = np.array([bool(r["flag"] & 16) for r in specs])
    sc = ctx.strand_counts(rs, cols)
    assert np.array_equal(sc["fwd"] + sc["rev"], matrix)
    assert np.array_equal(sc["rev"], times * oc.large_matrix([r for r, v in zip(specs, rev) if v], n_pos, q, [c for c, v in zip(clip, rev) if v] if clip is not None else None))
    assert np.array_equal(ctx.evidence_counts(rs, cols)["n"], matrix)
    pair = list(range(118, 150))
    links = lkc.device_links(ctx, rs, pair, 2)
    msg = lkc.differ(links, times * ly.joint(cls, pair, 2), ("large", "links", times, q))
    assert not msg, msg
    assert not ly.invariant(links, 2, matrix), ly.invariant(links, 2, matrix)
    want_codons = cy.joint(cls, ins, pair[:-2])
    want_codons["j"] *= times
    want_codons["ins_inside"] *= times
    codons = cc.device_codons(ctx, rs, pair[:-2])
    msg = cc.differ(codons, want_codons, ("large", "codons", times, q))
    assert not msg, msg
    assert not cy.invariant(codons, matrix), cy.invariant(codons, matrix)
    assert want_codons["ins_inside"].any() and ly.joint(cls, pair, 2).any()
    amps4 = [(90, 95, 260, 265), (90, 101, 140, 146)]
    reads = arc.device_counts(ctx, rs, amps4, 0)
    assert np.array_equal(reads, times * want_reads) and reads.sum() == times * 7, reads.tolist()


@pytest.mark.parametrize("how", dvf.PACKERS)
def test_large_but_legal_query_totals(ctx, store, how):
    path, specs, rd = large_file(store)
    want = oc.large_matrix(specs, 400)
    assert np.array_equal(c_oracle.tally(rd, 400), want)
    with dvf.uploaded(ctx, path, how=how) as rs:
        assert rs.n_piled == len(specs)
        check_large(ctx, rs, specs, large_reads(path))
    floor = oc.large_matrix(specs, 400, q=13)                                   # under a floor a base beyond SEQ has quality 0: it counts nothing
    assert not floor[100:112].any() and not floor[150:220].any() and 0 < floor[225:245, 0].sum() < 20 and floor[:, 6].sum() == 2
    with dvf.uploaded(ctx, path, q=13, how=how) as rs:
        assert np.array_equal(ctx.step(rs, 400, 0, True)[3], floor)
    # the pair whose query total is 2^29 - 1 under --mate-overlap and --dedup: the mate join and the duplicate ends read both records,
    # the later mate loses the fifteen columns it shares with the first
    clip, counters = my.join(rd)[:2]
    assert clip == [0, 0, 15, 0, 0, 0, 0] and counters["pairs"] == 1 and not dy.verdicts(rd)["dup"].any()
    if how == "one_sync":
        ctx.set_mate_overlap(True)
        ctx.set_dedup(True)
        try:
            with dvf.uploaded(ctx, path, how=how) as rs:
                ctx.set_mate_overlap(False)
                ctx.set_dedup(False)
                assert not rs.duplicates().any()
                check_large(ctx, rs, specs, large_reads(path), clip=clip)
        finally:
            ctx.set_mate_overlap(False)
            ctx.set_dedup(False)
    for device_pack in (0, 1):
        ctx.set_option("device_pack", device_pack)
        try:
            flat = ctx.upload(rd)
            assert np.array_equal(ctx.step(flat, 400, 0, True)[3], want), device_pack
            flat.free()
        finally:
            ctx.set_option("device_pack", 1)


def test_large_but_legal_query_totals_past_one_trip_of_the_grid(ctx, store):
    path, specs, _ = large_file(store)
    cap = ctx.stat("compute_units") * SC_WG_PER_CU * SC_BLOCK
    times = cap // len(specs) + 40
    big = str(store["dir"] / "large_big.bam")
    n = rb.repeat_records(path, big, times)
    assert n == times * len(specs) > cap + 256
    with dvf.uploaded(ctx, big) as rs:
        assert rs.n_reads == n
        check_large(ctx, rs, specs, large_reads(path), times)


# ---- 3. the refused files ----------------------------------------------------------------------------------------------------------------------
def good_counts(store):
    def make():
        path = str(store["dir"] / "good.bam")
        oc.good_file(path)
        return path, c_oracle.tally(c_oracle.read_bam(path), oc.GOOD_L)
    return once(store, "good", make)


def refused(call):
    with pytest.raises(_ffi.TcmiError) as e:
        call()
    assert e.value.code in REFUSALS, (e.value.code, str(e.value))
    return e.value


@pytest.mark.parametrize("kind", list(oc.LIARS))
def test_a_liar_is_refused_wherever_it_lies(ctx, store, kind):
    good, want = good_counts(store)
    try:
        for place in oc.PLACES:
            path = str(store["dir"] / ("liar_%s_%s.bam" % (kind, place)))
            at = oc.refused_file(path, kind, place)
            for one_sync in (1, 0):
                for crc in (1, 0):
                    ctx.set_option("one_sync", one_sync)
                    ctx.set_option("verify_crc", crc)
                    d = engine.DeviceBam(path)
                    try:
                        refused(lambda: ctx.upload_bamfile(d))
                    finally:
                        d.close()
            ctx.set_option("one_sync", 1)
            ctx.set_option("verify_crc", 1)
            b = engine.BamFile(path)
            for device_pack in (0, 1):                                          # the flat-array upload: the host packer words it
                ctx.set_option("device_pack", device_pack)
                e = refused(lambda: ctx.upload(b))
                assert e.code == _ffi.E_FORMAT and "read %d " % at in str(e) and "query bases" in str(e), (device_pack, str(e))
            ctx.set_option("device_pack", 1)
            b.close()
            # the same context then takes the good file
            with dvf.uploaded(ctx, good) as rs:
                assert np.array_equal(ctx.step(rs, oc.GOOD_L, 0, True)[3], want), (kind, place)
    finally:
        ctx.set_option("one_sync", 1)
        ctx.set_option("verify_crc", 1)
        ctx.set_option("device_pack", 1)


@pytest.mark.parametrize("kind,place,rank", [("S_x17", "first", 0), ("I_x9", "last", 1)])
def test_split_step_refuses_on_the_rank_that_holds_the_liar(store, kind, place, rank):
    import torch
    path = str(store["dir"] / ("split_%s.bam" % kind))
    oc.refused_file(path, kind, place)
    ld, n_words = distributed.split_words(oc.GOOD_L, 2)
    d = engine.DeviceBam(path)
    sctx = engine.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    try:
        t = torch.zeros(n_words, dtype=torch.int32, device="cuda")
        hook = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)(lambda user, p, n, s: 0)
        rc, rs, _ = distributed._split_step(sctx, d, rank, 2, oc.GOOD_L, ld, t, 10, True, hook, None)
        torch.cuda.synchronize()
        assert rc in REFUSALS and rs is None, rc
    finally:
        sctx.close()
        d.close()


@pytest.mark.parametrize("kind", list(oc.LIARS))
def test_a_liar_that_is_ignored_anyway_is_accepted(ctx, store, kind):
    _, want = good_counts(store)
    for form in oc.IGNORED:
        path = str(store["dir"] / ("ignored_%s_%s.bam" % (kind, form)))
        oc.refused_file(path, kind, "middle", form)
        f = oc.F if form == "filtered" else NONE
        for how in dvf.PACKERS:
            with dvf.uploaded(ctx, path, f=f, how=how) as rs:
                assert rs.n_reads == 41 and rs.n_piled == 40
                matrix = ctx.step(rs, oc.GOOD_L, 0, True)[3]
                assert np.array_equal(matrix, want), (kind, form, how)
                sc = ctx.strand_counts(rs, np.arange(oc.GOOD_L))
                assert np.array_equal(sc["fwd"] + sc["rev"], matrix)
        if form != "filtered":                                                  # (flat arrays carry no MAPQ: the filter is the file routes')
            b = engine.BamFile(path)
            for device_pack in (0, 1):
                ctx.set_option("device_pack", device_pack)
                try:
                    assert np.array_equal(ctx.tally(b, L=oc.GOOD_L), want), (kind, form, device_pack)
                finally:
                    ctx.set_option("device_pack", 1)
            b.close()


# ---- 4. the command line -----------------------------------------------------------------------------------------------------------------------
def test_cli_tables_of_a_tolerated_seed(store, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    path, specs, rd = data(store, "seed4")
    ref, orfs = sy.make_reference(seed=3, L=oc.L, cds=[(100, 900), (1100, 1900)])
    refb = ref.encode()
    w = yard(store, "seed4", None, "plain")
    whole, cls, ins, events = w["y"]["counts"], w["cls"], w["ins"], w["events"]
    assert len(whole) == oc.L
    recs = vy.records(whole, refb, 3, 100, 1, 10)                               # (the command line's defaults)
    cols = sorted({p for p, *_ in recs})
    arr = ly.records(cols, 2, ly.joint(cls, cols, 2))
    want_links = ly.text(recs, {(int(r["a"]), int(r["b"])): r["j"] for r in arr if r["b"] >= 0}, 2, "ref", refb, 10, 9, 10)
    icols = sorted({p for p, a, *_ in recs if a in (5, 6)})
    rep = iy.reported(events, icols, [int(whole[c, 0]) for c in icols], num=3, den=100, min_alt_depth=1, min_depth=10)
    want_indels = iy.text(rep, "ref", refb)
    frames = [(o["start"] - 1, o["end"], 1, 0) for o in orfs]
    codons = cy.joint(cls, ins, cy.select(recs, frames))
    want_codons = cy.text(codons, frames, ["orf%d" % k for k in range(len(orfs))], "ref", refb, 3, 100, 1, 10)
    assert want_links.count("\n") > 10 and len(rep) > 3 and want_codons.count("\n") > 10
    common = cr.setup_cli(ref, orfs)
    cr.run_cli(monkeypatch, ["-i", path, "-name", "S"] + common + ["-o", "a.fa", "-doc", "a.tsv", "--variant-table", "a.var", "--variant-strand",
                                                                   "--variant-links", "a.lnk", "--indel-table", "a.ind", "--codon-table", "a.cod",
                                                                   "--stats", "a.json"])
    assert cr.doc_column("a.tsv") == whole[:, 0].tolist()
    strand = {c: (w["fwd"][c], w["rev"][c]) for c in cols}                      # (--variant-strand: the variant table with its strand columns)
    assert open("a.var").read() == engine.VARIANTS_STRAND_HEADER + sty.text(recs, strand, "ref", refb, 10, 1, 10)
    assert [ln.split("\t")[:7] for ln in open("a.var").read().splitlines()[1:]] == [ln.split("\t") for ln in vy.text(recs, "ref", refb).splitlines()]
    assert open("a.lnk").read() == engine.VARIANTS_LINKS_HEADER + want_links
    assert open("a.ind").read() == engine.INDELS_HEADER + want_indels
    assert open("a.cod").read() == engine.CODONS_HEADER + want_codons


def test_cli_refuses_a_file_with_a_liar(store, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    at = oc.refused_file("liar.bam", "S_x17", "middle")
    ref, orfs = sy.make_reference(seed=3, L=oc.GOOD_L, cds=[(10, 300)])
    common = cr.setup_cli(ref, orfs, seqid="c")
    said = ""
    with pytest.raises((SystemExit, _ffi.TcmiError)) as e:
        cr.run_cli(monkeypatch, ["-i", "liar.bam", "-name", "S"] + common + ["-o", "a.fa"])
    if isinstance(e.value, SystemExit):
        assert e.value.code not in (0, None)
        out = capsys.readouterr()
        said = out.out + out.err
    else:                                                                       # (an exception that leaves main ends the process with status 1)
        said = str(e.value)
    assert "read %d " % at in said and "query bases" in said, said
