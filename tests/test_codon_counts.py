"""--codon-table on the GPU (csrc/codon_counts.hip; tcmi_readset_codon_counts, Context.codon_counts): every comparison is exact equality.
The yardstick is tests/codon_yardstick — the class of a record at a column is tests/links_yardstick.classes', the I mark the same
single-record matrix's I plane, the joint counts accumulated in Python —, the invariant is that the classes at each of a codon's three
columns add up to the matrix the step tallied from the same read set.  The inputs are hand-made records around one codon of a
100-column reference, the fuzz of tests/fuzz_masked.py and the fixed reads of tests/fixed_reads.py.  The host record buffer lies
between guard words that are checked after every call.  The rule, the writer and the argument handling are checked without a GPU in
tests/test_codon_rule.py and tests/test_cli_codons.py."""
import ctypes as C

import numpy as np
import pytest

from tests import codon_cases as cc
from tests import codon_yardstick as cy
from tests import dedup_cases as dc
from tests import device_file as dvf
from tests import fixed_reads as fx
from tests import fuzz_masked as fm
from tests import link_cases as lkc
from tests import read_specs as rsp
from tests import repeat_bam as rb
from tests.codon_cases import C0, HL, LDS, device_codons, differ
from tests.device_file import uploaded
from trueconsense_amd import _ffi, engine
from trueconsense_amd import distributed as td
from trueconsense_amd.io import bamwriter

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with engine.Context(0) as c:
        yield c


def hand_file(tmp_path, specs, name="H.bam"):
    path = str(tmp_path / name)
    bamwriter.write_bam(path, rsp.arrays(specs), ref_len=HL, block=4096)
    return path


def check(ctx, rs, c0s, want, whole, label):
    """the device's records at c0s equal the yardstick's and add up to the matrix the step tallies -> the records"""
    matrix = ctx.step(rs, len(whole), 0, True)[3]
    assert np.array_equal(matrix, whole), label
    got = device_codons(ctx, rs, c0s)
    msg = differ(got, want, label)
    assert not msg, msg
    assert not cy.invariant(got, matrix), (label, cy.invariant(got, matrix))
    return got


# ---- 1. hand-made records ----------------------------------------------------------------------------------------------------------------
def test_record_edges(ctx, tmp_path):
    specs = cc.edge_specs()
    want, whole, cls, _ = cc.yard(specs, HL, [C0])
    at = {r["name"]: tuple(int(x) != 0 for x in cls[i, C0:C0 + 3]) for i, r in enumerate(specs)}
    # the yardstick sees what the records were made for: every way of covering one or two of the three columns
    assert at == {"begins_0": (True, True, True), "begins_1": (False, True, True), "begins_2": (False, False, True), "ends_0": (True, False, False),
                  "ends_1": (True, True, False), "ends_2": (True, True, True), "over": (True, True, True), "one_column": (False, True, False),
                  "in_front": (False, False, False), "behind": (False, False, False)}, at
    assert want["j"][0].sum() == 8 and want["j"][0][1:, 1:, 1:].sum() == 3
    with uploaded(ctx, hand_file(tmp_path, specs)) as rs:
        check(ctx, rs, [C0], want, whole, "edges")
        for c0s in ([0], [C0 - 30], [C0 + 40, HL - 3, HL + 5], [0, 1, 2, C0 - 22, C0 - 21]):          # around the first and behind the last record
            check(ctx, rs, c0s, cy.joint(cls, np.zeros_like(cls), c0s), whole, ("edges", c0s))
    with uploaded(ctx, hand_file(tmp_path, [r for r in specs if r["name"] in ("in_front", "behind")], "N.bam")) as rs:
        assert not device_codons(ctx, rs, [C0])["j"].any()                      # a record that covers none of the columns adds nothing


def test_overlapping_frames(ctx, tmp_path):
    specs = cc.overlap_specs()
    c0s = cc.OVERLAP_C0
    want, whole, cls, ins = cc.yard(specs, HL, c0s)
    starts = {r["pos"] for r in specs}
    assert set(c0s) <= starts and {C0 - 1, C0 + 5, C0 + 12} <= starts and all(w["j"][1:, 1:, 1:].sum() >= 3 for w in want)
    assert all(w["j"][0].any() and w["j"][:, :, 0].any() for w in want)           # records that begin and that end inside every codon
    with uploaded(ctx, hand_file(tmp_path, specs)) as rs:
        got = check(ctx, rs, c0s, want, whole, "overlapping")
        for e, c in enumerate(c0s):                                             # each codon alone: the same counters
            alone = device_codons(ctx, rs, [c])
            assert alone["j"][0].tobytes() == got["j"][e].tobytes() and alone["ins_inside"][0] == got["ins_inside"][e], c
        dense = list(range(C0 - 8, C0 + 20))                                    # every column a codon: 28 codons in memory, the register shifts by one
        assert len(dense) > LDS
        check(ctx, rs, dense, cy.joint(cls, ins, dense), whole, "every column")
        two = sorted(set(range(C0 - 7, C0 + 20, 3)) | set(range(C0 - 6, C0 + 20, 3)))
        check(ctx, rs, two, cy.joint(cls, ins, two), whole, "two frames")
        gaps = [C0 - 6, C0 - 3, C0 + 1, C0 + 6, C0 + 7, C0 + 12]                # gaps of 0, 1, 2 columns between codons, and overlaps
        check(ctx, rs, gaps, cy.joint(cls, ins, gaps), whole, "gaps")


def test_cigar_shapes(ctx, tmp_path):
    specs, expect = cc.cigar_specs()
    want, whole, cls, ins = cc.yard(specs, HL, [C0])
    seen = {r["name"]: (tuple(int(x) for x in cls[i, C0:C0 + 3]), bool(ins[i, C0] or ins[i, C0 + 1])) for i, r in enumerate(specs)}
    assert seen == expect, seen                                                 # the yardstick sees what the records were made for
    assert want["ins_inside"][0] == 3 and want["j"][0][5, 5, 5] == 1 and want["j"][0][6, 6, 6] == 2 and want["j"][0][1, 1, 1] == 4
    with uploaded(ctx, hand_file(tmp_path, specs)) as rs:
        got = check(ctx, rs, [C0], want, whole, "shapes")
        assert got["ins_inside"][0] == 3
        around = [C0 - 3, C0 - 2, C0, C0 + 1, C0 + 3]
        check(ctx, rs, around, cy.joint(cls, ins, around), whole, "shapes, neighbours")
    for r in specs:                                                             # ... and each record alone
        w1, whole1, _, _ = cc.yard([r], HL, [C0])
        with uploaded(ctx, hand_file(tmp_path, [r], "one.bam")) as rs:
            got = check(ctx, rs, [C0], w1, whole1, r["name"])
            assert got["j"][0][expect[r["name"]][0]] == 1 and got["j"][0].sum() == 1 and got["ins_inside"][0] == int(expect[r["name"]][1]), r["name"]


def test_wave_join_and_flush(ctx, tmp_path):
    """600 records on one codon, five triplets in turn: several leaders a round, three workgroups on the same counters, staged and in memory"""
    specs = cc.join_specs()
    want, whole, cls, ins = cc.yard(specs[:5], HL, [C0])
    want["j"] *= len(specs) // 5
    whole = whole * (len(specs) // 5)
    assert len(specs) == 600 and (want["j"][0] > 0).sum() == 5 and want["j"][0].sum() == 600
    padded = [C0] + [HL + 10 * k for k in range(1, LDS + 1)]
    with uploaded(ctx, hand_file(tmp_path, specs)) as rs:
        assert rs.n_reads == 600
        staged = check(ctx, rs, [C0], want, whole, "join, LDS")
        memory = device_codons(ctx, rs, padded)
        assert memory["j"][0].tobytes() == staged["j"][0].tobytes() and not memory["j"][1:].any()


# ---- 2. the fuzz: both counter paths, every mode -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(fm.MODES))
@pytest.mark.parametrize("seed", fm.SEEDS[:2])
def test_fuzz_equals_the_yardstick_and_adds_up_to_the_matrix(ctx, tmp_path, seed, mode):
    tabled, slack, q, f = fm.MODES[mode]
    cls, ins, n_pos, whole = cc.marks_of(seed, mode)
    c0s = cc.two_frames(whole)
    assert len(c0s) == 100 and set(np.diff(c0s).tolist()) == {1, 2}
    want = cy.joint(cls, ins, c0s)
    j = want["j"].astype(np.int64)
    assert want["ins_inside"].any() and j[:, 0].any() and j[:, :, :, 0].any() and j[:, 5].any() and j[:, 6].any() and (j[:, 1:5, 1:5, 1:5].sum((1, 2, 3)) > 0).all()
    path = fm.write(tmp_path, fm.fuzz(seed))
    with uploaded(ctx, path, fm.table_of(seed) if tabled else (), q, f, slack) as rs:
        got = check(ctx, rs, c0s, want, whole, (seed, mode, "memory"))
        staged, over = device_codons(ctx, rs, c0s[:LDS]), device_codons(ctx, rs, c0s[:LDS + 1])        # n = TCMI_CODONS_LDS and one more
        assert staged.tobytes() == got[:LDS].tobytes() and over.tobytes() == got[:LDS + 1].tobytes(), (seed, mode, "the staging edge")


@pytest.mark.parametrize("rule", ("mate", "dedup", "both"))
@pytest.mark.parametrize("seed", fm.SEEDS[:2])
def test_fuzz_under_the_mate_rule_and_the_duplicate_rule_adds_up_to_the_matrix(ctx, tmp_path, seed, rule):
    """the yardstick's classes model neither rule: the matrix invariant alone, on the fuzz and on a paired fuzz with planted duplicates"""
    tabled, slack, q, f = fm.MODES["all"]
    files = [(fm.write(tmp_path, fm.fuzz(seed)), fm.table_of(seed), q, f, slack, fm.L)]
    paired = str(tmp_path / "P.bam")
    bamwriter.write_bam(paired, dc.arrays(dc.fuzz_specs(dc.FUZZ_SEEDS[seed - 1])), refs=dc.FUZZ_REFS, block=4096)
    files.append((paired, (), dc.FLOOR, dvf.NONE, 0, dc.FUZZ_L))
    for path, table, q, f, slack, n_pos in files:
        ctx.set_mate_overlap(rule in ("mate", "both"))
        ctx.set_dedup(rule in ("dedup", "both"))
        try:
            with uploaded(ctx, path, table, q, f, slack) as rs:
                ctx.set_mate_overlap(False)
                ctx.set_dedup(False)
                matrix = ctx.step(rs, max(n_pos, rs.max_end), 0, True)[3]
                c0s = cc.two_frames(matrix)
                for q_c0 in (c0s, c0s[:LDS]):
                    got = device_codons(ctx, rs, q_c0)
                    assert got["j"].any() and not cy.invariant(got, matrix), (seed, rule, path, cy.invariant(got, matrix))
                if path == paired:
                    changed = rs.mate_overlap["clipped_columns"] if rule == "mate" else rs.dedup["duplicate_records"]
                    assert changed > 0, (rule, rs.mate_overlap, rs.dedup)
        finally:
            ctx.set_mate_overlap(False)
            ctx.set_dedup(False)


# ---- 3. sub-ranges -------------------------------------------------------------------------------------------------------------------------
def test_sub_ranges_add_up_to_the_file(ctx, tmp_path):
    """a read set of two sub-ranges (tcmi_split_step, "split_sub") answers with the sum over its parts: the same records four times
    over in 1 024-byte blocks, four times the counts"""
    import torch
    seed = fm.SEEDS[1]
    tabled, slack, q, f = fm.MODES["all"]
    cls, ins, n_pos, whole = cc.marks_of(seed, "all")
    table = fm.table_of(seed)
    c0s = cc.two_frames(whole)
    want = cy.joint(cls, ins, c0s)
    big = sorted([dict(r, name="%s_%d" % (r["name"], k)) for k in range(4) for r in fm.fuzz(seed)], key=lambda r: r["pos"])
    path4 = str(tmp_path / "A4.bam")
    bamwriter.write_bam(path4, rsp.arrays(big), ref_len=fm.L, block=1024)
    c = engine.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    d = engine.DeviceBam(path4)
    try:
        c.set_option("split_sub", 2)
        c.set_rules(engine.ReadRules(f, q, (table, slack)))
        ld, n_words = td.split_words(n_pos, 1)
        t = torch.zeros(n_words, dtype=torch.int32, device="cuda")
        hook = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)(lambda user, p, n, stream: 0)
        rc, rs, _ = td._split_step(c, d, 0, 1, n_pos, ld, t, 10, True, hook, None)
        assert rc == 0 and c.stat("split_sub_taken") == 1
        for q_c0 in (c0s, c0s[:LDS]):
            got = device_codons(c, rs, q_c0)
            assert np.array_equal(got["j"], 4 * want["j"][:len(q_c0)]) and np.array_equal(got["ins_inside"], 4 * want["ins_inside"][:len(q_c0)])
        rs.free()
    finally:
        d.close()
        c.close()


# ---- 4. one trip past the grid ---------------------------------------------------------------------------------------------------------------
def test_one_record_past_one_trip_of_the_grid(ctx, tmp_path):
    """CAP + 1 fixed reads: CAP = compute units x SC_WG_PER_CU x SC_BLOCK records are one trip of each_record; the one live lane of the
    second trip holds a record that counts"""
    block, per_cu = rb.stream_count_caps()
    cap = ctx.stat("compute_units") * per_cu * block
    rd = fx.generate(cap + 1, 7)
    rd["qual"][-1, :3] = 30                                                     # (the one live lane of the second trip holds a record that counts at its first columns)
    path = fx.write(tmp_path / "C.bam", rd)
    last = int(rd["pos"][-1])
    c0s = sorted(set(range(700, 760, 3)) | set(range(701, 760, 3)) | {last - 1, last, last + fx.LEN - 2, last + fx.LEN - 1, fx.L + 7})
    c0s = [c for c in c0s if c >= 0]
    want = cc.fixed_codons(rd, c0s, 13)
    e = c0s.index(last)
    assert want["j"][e][1:, 1:, 1:].sum() > 0 and want["j"].astype(np.int64).sum((1, 2, 3)).max() > 4096
    with uploaded(ctx, path, (), 13, how="one_sync") as rs:
        assert rs.n_reads == cap + 1
        matrix = ctx.step(rs, fx.L, 0, True)[3]
        for q_c0 in (c0s, c0s[:LDS]):
            got = device_codons(ctx, rs, q_c0)
            msg = differ(got, want[:len(q_c0)], ("cap + 1", len(q_c0)))
            assert not msg, msg
            assert not cy.invariant(got, matrix), cy.invariant(got, matrix)
        one_less = device_codons(ctx, rs, [last])["j"][0].astype(np.int64)
    tail = {k: v[-1:] for k, v in rd.items()}
    assert (one_less - cc.fixed_codons(fx.head(rd, cap), [last], 13)["j"][0] == cc.fixed_codons(tail, [last], 13)["j"][0]).all()
    assert cc.fixed_codons(tail, [last], 13)["j"][0].sum() == 1                  # the record of the second trip is counted, once


# ---- 5. refusals and edge inputs -------------------------------------------------------------------------------------------------------------
def test_refusals_and_edge_inputs(ctx, tmp_path):
    specs = fm.fuzz(fm.SEEDS[0])
    pa = fm.write(tmp_path, specs[:400])
    pb_ = str(tmp_path / "B.bam")
    bamwriter.write_bam(pb_, rsp.arrays(specs[400:700]), ref_len=fm.L, block=4096)
    da, db = engine.DeviceBam(pa), engine.DeviceBam(pb_)
    try:
        ra = ctx.upload_bamfile(da)
        assert ctx.codon_counts(ra, [10, 500, 1500])["j"].any()
        guarded = dvf.sentinel(2 * cc.G + cc.W * 4, np.int32, salt=3).copy()
        top = (1 << 29) - 2
        for bad, word in (([5, 5], "strictly ascending"), ([7, 5], "strictly ascending"), ([1, 2, 2, 9], "strictly ascending"), ([], "1..16384"),
                          (np.arange((1 << 14) + 1), "1..16384"), ([3, top], "2^29 - 2"), ([top], "2^29 - 2"), ([-1, 4], "2^29 - 2")):
            with pytest.raises(_ffi.TcmiError) as e:
                ctx.codon_counts(ra, bad)
            assert e.value.code == _ffi.E_ARG and word in str(e.value) and "codon counts" in str(e.value), (bad[:4], str(e.value))
            if 0 < len(bad) <= 4:                                               # ... and nothing is written when the call refuses
                before = guarded.copy()
                rc = _ffi.lib().tcmi_readset_codon_counts(ctx.handle, ra.handle, len(bad), _ffi.ptr(np.ascontiguousarray(bad, np.int64)),
                                                          C.c_void_p(guarded.ctypes.data + 4 * cc.G))
                assert rc == _ffi.E_ARG and np.array_equal(guarded, before)
        most = ctx.codon_counts(ra, np.arange(1 << 14))                          # the most codons of one call
        assert len(most) == 1 << 14 and np.array_equal(most["pos"], np.arange(1 << 14)) and not most["reserved"].any()
        assert ctx.codon_counts(ra, [top - 1])["pos"][0] == top - 1              # the last column a codon may start on
        rb_ = ctx.upload_bamfile(db)                                            # another upload on the context: ra's stream is displaced
        with pytest.raises(_ffi.TcmiError) as e:
            ctx.codon_counts(ra, [10, 500])
        assert e.value.code == _ffi.E_UNSUPPORTED and "no longer resident" in str(e.value) and "codon counts" in str(e.value)
        assert ctx.codon_counts(rb_, [10, 500, 1500])["j"].any()                # the newer one answers
        ra.free()
        rb_.free()
    finally:
        da.close()
        db.close()
    bam = engine.BamFile(pa)
    flat = ctx.upload(bam)                                                      # the host reader: packed, but no record stream
    with pytest.raises(_ffi.TcmiError) as e:
        ctx.codon_counts(flat, [10, 500])
    assert e.value.code == _ffi.E_UNSUPPORTED and "not decoded on the device" in str(e.value)
    flat.free()
    bam.close()
    with uploaded(ctx, pa, (), 0, (0, 0x1000, 0)) as rs:                        # a FLAG bit no record has is required: an empty read set gives zeros
        assert rs.n_piled == 0
        got = device_codons(ctx, rs, [10, 11, 500])
        assert not got["j"].any() and not got["ins_inside"].any()


def test_the_launch_is_filed_under_the_link_counts_bracket(ctx, tmp_path):
    path = fm.write(tmp_path, fm.fuzz(fm.SEEDS[0])[:500])
    try:
        ctx.profile(True)
        with uploaded(ctx, path) as rs:
            assert ctx.profile_get(_ffi.K_LINK_COUNTS)[1] == 0
            ctx.codon_counts(rs, [100, 900])
            ctx.codon_counts(rs, np.arange(LDS + 1))
            ms, n = ctx.profile_get(_ffi.K_LINK_COUNTS)
            assert n == 2 and ms > 0
    finally:
        ctx.profile(False)


def test_context_selects_the_codons_of_the_records(ctx, tmp_path):
    specs, _ = cc.cigar_specs()
    cds = np.array([(C0 - 9, C0 + 30, 1, 0), (C0 - 9, C0 + 30, -1, 1)], engine.CDS_DTYPE)
    recs = np.array([(C0 + 1, 5, 3, 10), (C0 + 1, 6, 2, 10), (C0 + 4, 6, 2, 10)], engine.VARIANT_DTYPE)
    c0s = cy.select(recs.tolist(), cds.tolist())
    assert len(c0s) == 2
    with uploaded(ctx, hand_file(tmp_path, specs)) as rs:
        got = ctx.codon_counts_of(rs, recs, cds)
        assert got.tobytes() == device_codons(ctx, rs, c0s).tobytes()
        assert len(ctx.codon_counts_of(rs, recs[2:], cds)) == 0 and len(ctx.codon_counts_of(rs, recs, cds[:0])) == 0
