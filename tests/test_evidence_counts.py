"""--variant-evidence on the GPU (csrc/evidence_counts.hip; tcmi_readset_evidence_counts, Context.evidence_counts): every comparison is
exact equality.  The yardstick is tests/evidence_yardstick.py — a CIGAR walk of its own in Python's integers, tied to
tc_oracle.read_tokens and tests/primer_yardstick.counts —, the invariant is n == the matrix the step tallied from the same read set,
and the independent device route is the sum over Q of the matrix of the same file uploaded under floor Q (min_mapq Q).  The inputs
are those of tests/test_floor_mask_fuzz.py (tests/fuzz_masked.specs: every CIGAR op, SEQ '*', short SEQ, no QUAL, long reads, planted
insertion sites, FLAG 16 on a third of the records), hand-made records for the distance rule, and files past one trip of the grid
(tests/repeat_bam.py, tests/fixed_reads.py).  The host record buffer lies between guard words that are checked after every call
(tests/evidence_cases.device_counts).  The rule, the writer, the LDS bound and the argument handling are checked without a GPU in
tests/test_evidence_rule.py."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from tests import cli_run as cr
from tests import device_file as dvf
from tests import evidence_cases as ec
from tests import evidence_yardstick as ey
from tests import fixed_reads as fx
from tests import fuzz_masked as fm
from tests import read_specs as rsp
from tests import repeat_bam as rb
from tests import schemes as sch
from tests import strand_cases as stc
from tests import variant_yardstick as vy
from tests.device_file import uploaded
from tests.evidence_cases import LDS, G, L, WORDS, device_counts, differ, not_vacuous, sparse_columns, sums_of, take, times
from trueconsense_amd import TrueConsense as cli
from trueconsense_amd import _ffi, engine
from trueconsense_amd import distributed as td
from trueconsense_amd import synthetic as syn
from trueconsense_amd.io import bamwriter

pytestmark = pytest.mark.gpu
SC_BLOCK, SC_WG_PER_CU = rb.stream_count_caps()
SEEDS = fm.SEEDS


@pytest.fixture(scope="module")
def ctx():
    with engine.Context(0) as c:
        yield c


# ---- 1. both routes, three modes, both packers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_sync", (1, 0))
@pytest.mark.parametrize("mode", sorted(fm.MODES))
@pytest.mark.parametrize("seed", SEEDS)
def test_both_routes_equal_the_yardstick_and_n_is_the_matrix(ctx, tmp_path, seed, mode, one_sync):
    tabled, slack, q, f = fm.MODES[mode]
    sums, marks, n_pos = sums_of(seed, mode)
    sparse, dense = sparse_columns(seed, n_pos), list(range(n_pos))
    assert len(sparse) <= LDS < len(dense)
    for cols in (sparse, dense):
        not_vacuous(sums, marks, cols, (seed, mode, len(cols)))
        if mode == "all":
            ec.removed_by_each(seed, cols, (seed, len(cols)))
    path = fm.write(tmp_path, fm.fuzz(seed))
    with uploaded(ctx, path, fm.table_of(seed) if tabled else (), q, f, slack, one_sync) as rs:
        matrix = ctx.step(rs, n_pos, 0, True)[3]
        for route, cols in (("LDS", sparse), ("memory", dense)):
            got = device_counts(ctx, rs, cols)
            msg = differ(got, take(sums, cols), cols, (seed, mode, one_sync, route))
            assert not msg, msg
            assert np.array_equal(got[0], matrix[cols]), (seed, mode, one_sync, route, "the invariant")


# ---- 2. the staging edge -------------------------------------------------------------------------------------------------------------
def test_the_largest_staged_query_and_the_smallest_in_memory(ctx, tmp_path):
    seed = SEEDS[1]
    sums, marks, n_pos = sums_of(seed, "floor")
    cols = sorted(int(c) for c in np.random.default_rng(9).choice(n_pos, LDS + 1, replace=False))
    assert len(cols) == 129 and LDS == 128
    not_vacuous(sums, marks, cols[:LDS], seed)
    path = fm.write(tmp_path, fm.fuzz(seed))
    with uploaded(ctx, path, (), 13) as rs:
        staged, memory = device_counts(ctx, rs, cols[:LDS]), device_counts(ctx, rs, cols)
    assert not differ(staged, take(sums, cols[:LDS]), cols, "staged"), differ(staged, take(sums, cols[:LDS]), cols, "staged")
    assert not differ(memory, take(sums, cols), cols, "memory"), differ(memory, take(sums, cols), cols, "memory")
    assert all(np.array_equal(s, m[:LDS]) for s, m in zip(staged, memory))


# ---- 3. small and ragged -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rec", (1, 63, 65, 257))
def test_small_files(ctx, tmp_path, n_rec):
    """1, 63, 65 and 257 records (fewer than a wavefront, one more, one more than a workgroup); a column nobody covers, a column beyond
    every read; the same records under a filter that all of them fail: zeros, and TCMI_OK"""
    every = [r for r in fm.fuzz(fm.SEEDS[2]) if fm._piles_up(r)]
    step = len(every) // n_rec
    one = next(r for r in every if "D" in r["cigar"] and "I" in r["cigar"] and fm._span(r) > 20 and r["seq"] != "*" and r["qual"] and r["qual"][0] != 255)
    specs = every[::step][:n_rec] if n_rec > 1 else [one]
    assert len(specs) == n_rec
    rd = rsp.arrays(specs)
    sums, marks = ey.whole(rd, L, (), 13)
    whole = sums[0]
    n_pos = len(whole)
    beyond = n_pos + 700
    bare = [c for c in range(n_pos) if not whole[c].any()]
    assert bare and whole[:, 0].any() and len({int(m[:, 0].sum()) for m in sums}) == 4 and whole[:, 5].any() and whole[:, 6].any()
    dense = list(range(n_pos)) + [beyond]
    sparse = sorted(set(int(c) for c in np.random.default_rng(n_rec).choice(n_pos, 60, replace=False)) | {bare[0], int(np.argmax(whole[:, 0])), beyond})
    if n_rec > 1:
        not_vacuous(sums, marks, dense[:-1], n_rec)
    want = ey.at(sums, dense)
    path = fm.write(tmp_path, specs)
    with uploaded(ctx, path, (), 13) as rs:
        assert rs.n_reads == n_rec
        matrix = ctx.step(rs, n_pos, 0, True)[3]
        for cols in (sparse, dense):
            idx = [dense.index(c) for c in cols]
            got = device_counts(ctx, rs, cols)
            msg = differ(got, take(want, idx), cols, (n_rec, len(cols)))
            assert not msg, msg
            assert np.array_equal(got[0][:-1], matrix[cols[:-1]]) and not any(g[-1].any() for g in got)
            assert not any(g[cols.index(bare[0])].any() for g in got)
    with uploaded(ctx, path, (), 13, (0, 0x1000, 0)) as rs:                     # a FLAG bit no record has is required: every record fails
        assert rs.n_reads == n_rec and rs.n_piled == 0 and rs.filtered == n_rec
        assert not any(g.any() for g in device_counts(ctx, rs, sparse))


def test_a_wavefront_on_64_columns_and_a_ragged_one_behind_it(ctx, tmp_path):
    """the join's worst case: strand_cases.one_column_a_record, one queried column per record — 64 distinct counters a round"""
    specs, cols = stc.one_column_a_record()
    rd = rsp.arrays(specs)
    sums, _ = ey.whole(rd, L)
    padded = cols + [len(sums[0]) + 700 + j for j in range(LDS + 1 - len(cols))]
    assert len(specs) == 65 and len(cols) == 64 <= LDS < len(padded)
    want = ey.at(sums, padded)
    assert want[0][:, 0].tolist() == [2] + [1] * 63 + [0] * (len(padded) - 64) and want[1][0, 0] == 60 and want[3][:64, 0].tolist() == [0] + [r % 6 if r % 6 < 3 else 5 - r % 6 for r in range(1, 64)]
    path = fm.write(tmp_path, specs)
    with uploaded(ctx, path) as rs:
        for route, q in (("LDS", cols), ("memory", padded)):
            msg = differ(device_counts(ctx, rs, q), take(want, list(range(len(q)))), q, ("one column a record", route))
            assert not msg, msg


# ---- 4. the distance rule on hand-made records -----------------------------------------------------------------------------------------
def test_hand_made_records(ctx, tmp_path):
    """5S20M5S, 3H4S10M, a 700-base read whose middle is capped at 255, 10M3D10M, 10M2D5S (the D starts at a1: distance 0), an insertion
    mark, MAPQ 0 / 60 / 255 and a record without QUAL: tests/evidence_cases.HAND states the numbers by hand (pinned to the yardstick in
    tests/test_evidence_rule.py)"""
    specs, _ = ec.hand_records()
    sums, marks = ey.whole(rsp.arrays(specs), L)
    n_pos = len(sums[0])
    sparse, dense = sorted(ec.HAND), list(range(n_pos))
    not_vacuous(sums, marks, sparse, "hand", capped=True)
    path = fm.write(tmp_path, specs)
    with uploaded(ctx, path) as rs:
        assert rs.n_reads == rs.n_piled == len(specs)
        matrix = ctx.step(rs, n_pos, 0, True)[3]
        for cols in (sparse, dense):
            got = device_counts(ctx, rs, cols)
            msg = differ(got, take(sums, cols), cols, ("hand", len(cols)))
            assert not msg, msg
            assert np.array_equal(got[0], matrix[cols])
        got = device_counts(ctx, rs, sparse)
    for k, c in enumerate(sparse):
        qi, mapq, dist = ec.HAND[c]
        assert tuple(int(g[k, 0]) for g in got) == (1, 255 if c >= 1400 else ec.hand_quality(qi), mapq, dist), c


# ---- 5. the independent device route -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def thinned():
    """every fourth piled-up record of a fuzz seed, qualities at most 40 (no record without QUAL), MAPQ at most 60"""
    out = []
    for r in [r for r in fm.fuzz(fm.SEEDS[3]) if fm._piles_up(r)][::4]:
        qual = [40] * len(r["qual"]) if r["qual"] and r["qual"][0] == 255 else [min(int(x), 40) for x in r["qual"]]
        out.append(dict(r, qual=qual, mapq=37 if r["mapq"] == 255 else r["mapq"]))
    return out


def test_the_sums_equal_the_devices_own_matrices_summed_over_the_floor_and_over_min_mapq(ctx, tmp_path):
    """a token of quality q <= 40 is in the matrix under floor Q for Q = 1..q: the quality sums are the sum of those forty matrices;
    likewise MAPQ <= 60 and the read filter's min_mapq = 1..60"""
    specs = thinned()
    rd = rsp.arrays(specs)
    assert 200 <= len(specs) <= 600 and max(max(r["qual"]) for r in specs if r["qual"]) == 40 and {r["mapq"] for r in specs} >= {0, 1, 60} and max(r["mapq"] for r in specs) == 60
    sums, marks = ey.whole(rd, L)
    n_pos = len(sums[0])
    cols = list(range(n_pos))
    not_vacuous(sums, marks, cols, "thinned")
    path = fm.write(tmp_path, specs)
    by_floor = sum(dvf.through(ctx, "one_sync", path, (), n_pos, q)[0].astype(np.int64) for q in range(1, 41))
    by_mapq = sum(dvf.through(ctx, "one_sync", path, (), n_pos, 0, (m, 0, 0))[0].astype(np.int64) for m in range(1, 61))
    assert by_floor.any() and by_mapq.any() and not np.array_equal(by_floor, by_mapq)
    with uploaded(ctx, path) as rs:
        for use in (cols, cols[5::17][:LDS]):
            got = device_counts(ctx, rs, use)
            assert np.array_equal(got[1], by_floor[use]), ("quality", len(use), np.argwhere(got[1] != by_floor[use])[:5].tolist())
            assert np.array_equal(got[2], by_mapq[use]), ("MAPQ", len(use), np.argwhere(got[2] != by_mapq[use])[:5].tolist())
            assert not differ(got, take(sums, use), use, "thinned")


# ---- 6. past one trip of the grid --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cap(ctx):
    """the records one trip of each_record covers on this device"""
    n = ctx.stat("compute_units") * SC_WG_PER_CU * SC_BLOCK
    assert n > 0
    return n


@pytest.mark.parametrize("mode", ("all", "table"))
def test_the_deep_file_repeated_past_one_trip(ctx, tmp_path, cap, mode):
    """every record of the deep fuzz file R times in place, R odd with R * records just above CAP and so chosen that a workgroup's
    staged counter passes 65 535 (a workgroup with lanes in both trips on one column: tests/evidence_cases.lds_peak): R times the
    yardstick of the small file, staged and in memory"""
    seed, window = fm.DEEP_SEED, fm.DEEP_WINDOW
    tabled, slack, q, f = fm.MODES[mode]
    table = fm.table_of(seed) if tabled else ()
    every = fm.fuzz(seed, None, window)
    sums, marks, n_pos = sums_of(seed, mode, window)
    sparse = sorted(set(range(window[0] - 20, window[1] + 60, 3)) | set(stc.sparse_columns(seed, n_pos, 20)))[:LDS]
    dense = list(range(n_pos))
    for cols in (sparse, dense):
        not_vacuous(sums, marks, cols, ("deep", mode, len(cols)))
    per = ec.token_table(ec.fuzz_arrays(seed, window), sparse, table, q, slack, f)
    r = cap // len(every) + 1
    r += r % 2 == 0
    first = r
    while (r * len(every)) % 64 == 0 or ec.lds_peak(per, len(every), len(sparse), r, cap, SC_BLOCK) <= 65535:
        r += 2
        assert r < first + 200, "no repeat count takes a staged counter past 65 535"
    n = r * len(every)
    assert cap < n < 2 * cap and n % 64 != 0 and engine.EVIDENCE_LDS == LDS
    src = fm.write(tmp_path, every)
    dst = str(tmp_path / "R.bam")
    assert rb.repeat_records(src, dst, r) == n
    with uploaded(ctx, dst, table, q, f, slack, how="one_sync", events_may_overflow=True) as rs:
        assert rs.n_reads == n
        matrix = ctx.step(rs, n_pos, 0, True)[3]
        for route, cols in (("LDS", sparse), ("memory", dense)):
            got = device_counts(ctx, rs, cols)
            msg = differ(got, times(take(sums, cols), r), cols, ("deep", mode, r, route))
            assert not msg, msg
            assert np.array_equal(got[0], matrix[cols])


C_COLS = sorted(int(c) for c in np.random.default_rng(41).choice(fx.L, LDS, replace=False))
C_MODES = {"plain": (0, fm.NONE, (), 0), "all": (13, fx.MQ, tuple(sch.PRIMER_SCHEME), 3)}


@pytest.mark.parametrize("which", ("cap_plus_1", "three_trips"))
def test_fixed_reads_at_the_bounds_of_each_record(ctx, tmp_path, cap, which):
    """tests/fixed_reads.py's 20M records at CAP + 1 (a second trip with one live lane) and 2 CAP + 256 + 65 (three trips, a full and a
    ragged workgroup in the last); the yardstick is tests/evidence_cases.fixed_counts (pinned in tests/test_evidence_rule.py)"""
    n = {"cap_plus_1": cap + 1, "three_trips": 2 * cap + SC_BLOCK + 65}[which]
    rd = fx.generate(n, 200 + len(which))
    rd["mapq"][-1] = 60                                                         # (the last lane holds a record that passes the filter)
    path = fx.write(tmp_path / "C.bam", rd)
    for mode, (q, f, table, slack) in C_MODES.items():
        with uploaded(ctx, path, table, q, f, slack, how="one_sync") as rs:
            assert rs.n_reads == n
            matrix = ctx.step(rs, fx.L, 0, True)[3]
            for route, cols in (("LDS", C_COLS), ("memory", list(range(fx.L)))):
                want = ec.fixed_counts(rd, cols, q, f, table, slack)
                assert len({int(m[:, 0].sum()) for m in want}) == 4 and want[0][:, 1:5].sum(0).all()
                got = device_counts(ctx, rs, cols)
                msg = differ(got, want, cols, (which, mode, route))
                assert not msg, msg
                assert np.array_equal(got[0], matrix[cols])


# ---- 7. refusals, the profiling slot -------------------------------------------------------------------------
def test_refusals(ctx, tmp_path):
    specs = fm.fuzz(fm.SEEDS[0])
    pa = fm.write(tmp_path, specs[:400])
    pb_ = str(tmp_path / "B.bam")
    bamwriter.write_bam(pb_, rsp.arrays(specs[400:700]), ref_len=L, block=4096)
    da, db = engine.DeviceBam(pa), engine.DeviceBam(pb_)
    try:
        ra = ctx.upload_bamfile(da)
        ok = ctx.evidence_counts(ra, [10, 500, 1500])
        assert ok["n"][:, 0].any() and ok["qual"][:, 0].any()
        guarded = dvf.sentinel(2 * G + WORDS * 4, np.int32, salt=3).copy()
        for bad, word in (([5, 5], "strictly ascending"), ([7, 5], "strictly ascending"), ([1, 2, 2, 9], "strictly ascending"), ([], "1..1048576"),
                          (np.arange((1 << 20) + 1), "1..1048576"), ([3, 1 << 29], "2^29"), ([-1, 4], "2^29")):
            with pytest.raises(_ffi.TcmiError) as e:
                ctx.evidence_counts(ra, bad)
            assert e.value.code == _ffi.E_ARG and word in str(e.value) and "evidence counts" in str(e.value), (bad[:4], str(e.value))
            if 0 < len(bad) <= 4:                                               # ... and nothing is written when the call refuses
                before = guarded.copy()
                rc = _ffi.lib().tcmi_readset_evidence_counts(ctx.handle, ra.handle, len(bad), _ffi.ptr(np.ascontiguousarray(bad, np.int64)),
                                                             C.c_void_p(guarded.ctypes.data + 4 * G))
                assert rc == _ffi.E_ARG and np.array_equal(guarded, before)
        rb_ = ctx.upload_bamfile(db)                                            # another upload on the context: ra's stream is displaced
        with pytest.raises(_ffi.TcmiError) as e:
            ctx.evidence_counts(ra, [10, 500])
        assert e.value.code == _ffi.E_UNSUPPORTED and "no longer resident" in str(e.value)
        assert ctx.evidence_counts(rb_, [10, 500, 1500])["n"].any()             # the newer one answers
        ra.free()
        rb_.free()
    finally:
        da.close()
        db.close()
    bam = engine.BamFile(pa)
    flat = ctx.upload(bam)                                                      # flat arrays: packed, but no record stream
    with pytest.raises(_ffi.TcmiError) as e:
        ctx.evidence_counts(flat, [10, 500])
    assert e.value.code == _ffi.E_UNSUPPORTED and "not decoded on the device" in str(e.value)
    flat.free()
    bam.close()


def test_the_launch_is_profiled_and_nothing_runs_without_the_call(ctx, tmp_path):
    path = fm.write(tmp_path, fm.fuzz(fm.SEEDS[0])[:500])
    try:
        ctx.profile(True)
        with uploaded(ctx, path) as rs:
            ctx.step(rs, L, 10, True)
            assert ctx.profile_get(_ffi.K_EVIDENCE_COUNTS)[1] == 0
            ctx.evidence_counts(rs, [100, 900])
            ctx.evidence_counts(rs, np.arange(LDS + 1))
            ms, n = ctx.profile_get(_ffi.K_EVIDENCE_COUNTS)
            assert n == 2 and ms > 0 and ctx.profile_get(_ffi.K_STRAND_COUNTS)[1] == 0
    finally:
        ctx.profile(False)


# ---- 8. the command line ---------------------------------------------------------------------------------------------------------------
CL = 1200
LOWQ_AT, LOWMQ_AT, END_AT, DEL_AT, INS_AT = 300, 500, 700, 900, 1000             # the planted alleles' 0-based columns


@functools.lru_cache(maxsize=None)
def cli_case():
    """-> (reference, GFF rows, records): 100-base reads at about 60x over 1 200 columns.  A base other than the reference's sits on a
    third of the reads at LOWQ_AT with quality 9, at LOWMQ_AT on the reads of MAPQ 3 (a third of all), at END_AT on the reads that start
    or end within two bases of it; a third of the reads over DEL_AT delete two bases there, a third of those over INS_AT insert two"""
    rng = np.random.default_rng(78)
    ref, orfs = syn.make_reference(seed=3, L=CL, cds=[(100, 900)])
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}
    specs = []
    for k in range(720):
        pos = int(rng.integers(0, CL - 100 + 1))
        if k % 12 == 0:                                                         # reads that end or start right at END_AT
            pos = END_AT - 99 + int(rng.integers(0, 3)) if k % 24 else END_AT - int(rng.integers(0, 3))
        mapq = 3 if k % 3 == 1 else 60
        seq, qual, cig = list(ref[pos:pos + 100].upper()), [int(x) for x in rng.integers(25, 41, 100)], "100M"
        inside = lambda c: pos + 3 <= c < pos + 97
        if pos <= LOWQ_AT < pos + 100 and rng.random() < 0.33:
            seq[LOWQ_AT - pos], qual[LOWQ_AT - pos] = other[seq[LOWQ_AT - pos]], 9
        if pos <= LOWMQ_AT < pos + 100 and mapq == 3:
            seq[LOWMQ_AT - pos] = other[seq[LOWMQ_AT - pos]]
        if pos <= END_AT < pos + 100 and min(END_AT - pos, pos + 99 - END_AT) <= 2:
            seq[END_AT - pos] = other[seq[END_AT - pos]]
        if inside(DEL_AT) and rng.random() < 0.33:
            a = DEL_AT - pos
            seq, qual, cig = seq[:a] + seq[a + 2:] + ["A", "C"], qual, "%dM2D%dM" % (a, 100 - a)
        elif inside(INS_AT) and rng.random() < 0.33:
            a = INS_AT - pos + 1
            seq, cig = seq[:a] + ["G", "T"] + seq[a:98], "%dM2I%dM" % (a, 98 - a)
        specs.append({"pos": pos, "flag": 16 if k % 2 else 0, "cigar": cig, "seq": "".join(seq), "name": "r%d" % k, "tid": 0, "qual": qual, "mapq": mapq})
    specs.sort(key=lambda r: r["pos"])
    return ref, orfs, specs


def cli_yardstick(specs, ref, rule=(20, 20, 5), n_pos=CL):
    """-> (the records, the evidence array, the text) of the yardsticks at the command line's default thresholds"""
    rd = rsp.arrays(specs)
    sums, _ = ey.whole(rd, n_pos)
    recs = vy.records(sums[0], ref.encode(), 3, 100, 1, 10)
    cols = sorted({p for p, *_ in recs})
    at = take(sums, cols)
    return recs, ey.records(cols, at), ey.text(recs, ey.as_dict(cols, at), "ref", ref.encode(), *rule)


def test_cli_single_sample_per_contig_and_the_other_tables(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ref, orfs, specs = cli_case()
    recs, ev, want = cli_yardstick(specs, ref)
    assert engine.variants_evidence_text(vy.as_array(recs), ev, "ref", ref) == want
    word_at = {(int(ln.split("\t")[1]) - 1, ln.split("\t")[3]): ln.split("\t")[-1] for ln in want.splitlines()}
    alt_at = lambda c: next(w for (p, a), w in word_at.items() if p == c and a in "ACGT")
    assert (alt_at(LOWQ_AT), alt_at(LOWMQ_AT), alt_at(END_AT)) == ("LOWQ", "LOWMQ", "END"), word_at
    assert word_at[(DEL_AT, "*")] == "PASS" and word_at[(INS_AT, "+")] == "PASS"
    bamwriter.write_bam("A.bam", rsp.arrays(specs), ref_len=CL, block=4096)
    common = cr.setup_cli(ref, orfs)
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + cr.out_args("a") + ["--variant-table", "a.var", "--variant-evidence", "a.ev", "--stats", "a.json"])
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + cr.out_args("b") + ["--variant-table", "b.var", "--stats", "b.json"])
    got, plain = open("a.ev").read(), open("b.var").read()
    assert got == engine.VARIANTS_EVIDENCE_HEADER + want
    assert open("a.var").read() == plain and [ln.split("\t")[:7] for ln in got.splitlines()] == [ln.split("\t") for ln in plain.splitlines()]
    assert cr.outputs("a") == cr.outputs("b")
    sa, sb = json.load(open("a.json")), json.load(open("b.json"))
    tally = cli.evidence_stats(want)
    assert {k: sa[k] for k in tally} == tally and all(tally.values()) and {k: sb[k] for k in tally} == dict.fromkeys(tally, 0)
    assert sa["variant_records"] == sb["variant_records"] == len(recs)
    # other thresholds; together with the strand columns, the links and the indel table
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + ["-o", "c.fa", "--variant-table", "c.var", "--variant-evidence", "c.ev", "--evidence-min-qual", "0",
                                                                      "--evidence-min-mapq", "61", "--evidence-min-enddist", "40", "--variant-strand", "--variant-links", "c.lnk",
                                                                      "--indel-table", "c.ind"])
    other = cli_yardstick(specs, ref, (0, 61, 40))[2]
    assert open("c.ev").read() == engine.VARIANTS_EVIDENCE_HEADER + other and other != want and "LOWQ" not in other and "LOWMQ,END" in other
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + ["-o", "d.fa", "--variant-table", "d.var", "--variant-strand", "--variant-links", "d.lnk", "--indel-table", "d.ind"])
    assert all(open("c" + x).read() == open("d" + x).read() for x in (".var", ".lnk", ".ind", ".fa")) and open("c.var").read().startswith(engine.VARIANTS_STRAND_HEADER)
    assert open("c.ind").read().count("\n") >= 3

    # --per-contig: the same records on two references of the same sequence: the same rows per region
    two = sorted([dict(r, tid=t, name="%s_%d" % (r["name"], t)) for t in (0, 1) for r in specs], key=lambda r: (r["tid"], r["pos"]))
    bamwriter.write_bam("P.bam", rsp.arrays(two), refs=[("c0", CL), ("c1", CL)], block=4096)
    with open("p.fa", "w") as fh:
        fh.write(">c0\n%s\n>c1\n%s\n" % (ref, ref))
    with open("p.gff", "w") as fh:
        fh.write("##gff-version 3\n" + syn.gff_text(orfs, seqid="c0")[1] + syn.gff_text(orfs, seqid="c1")[1])
    cr.run_cli(monkeypatch, ["-i", "P.bam", "-ref", "p.fa", "-gff", "p.gff", "-cov", "10", "-name", "S", "--per-contig", "-o", "p.fa.out", "--variant-table", "p.var",
                             "--variant-evidence", "p.ev", "--stats", "p.json"])
    assert open("p.ev").read() == engine.VARIANTS_EVIDENCE_HEADER + want.replace("ref\t", "c0\t") + want.replace("ref\t", "c1\t")
    sp = json.load(open("p.json"))
    assert {k: sp[k] for k in tally} == {k: 2 * v for k, v in tally.items()} and sp["variant_records"] == 2 * len(recs)


def test_cli_refuses_a_file_the_host_reads(tmp_path, monkeypatch):
    """a file that leaves the device path (the device decoder is made to decline it) is refused by the flag's name, never counted another
    way, and nothing is written"""
    monkeypatch.chdir(tmp_path)
    ref, orfs, specs = cli_case()
    bamwriter.write_bam("A.bam", rsp.arrays(specs), ref_len=CL, block=4096)
    common = cr.setup_cli(ref, orfs)

    def declined(self, dbam, blocks=None):
        raise _ffi.TcmiError(_ffi.E_UNSUPPORTED, "forced")
    before = sorted(os.listdir(tmp_path))
    with monkeypatch.context() as m:
        m.setattr(engine.Context, "upload_bamfile", declined)
        with pytest.raises(_ffi.TcmiError) as e:
            cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + ["-o", "x.fa", "--variant-table", "x.var", "--variant-evidence", "x.ev"])
        assert e.value.code == _ffi.E_UNSUPPORTED and "--variant-evidence needs the device path" in str(e.value) and "forced" in str(e.value)
        cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + ["-o", "y.fa", "--variant-table", "y.var"])     # without the flag the host reader takes it
    assert sorted(os.listdir(tmp_path)) == sorted(before + ["y.fa", "y.var"])


# ---- 9. a read set of sub-ranges (last: it leaves helper contexts on the module's context) ---------------------------------------------
def test_sub_ranges_answer_with_the_sum_of_their_parts(ctx, tmp_path):
    """a read set of two sub-ranges (tcmi_split_step, "split_sub") is counted part by part, each part staged by its own records and
    grid: the file's counts, staged and in memory"""
    import torch
    seed = SEEDS[0]
    tabled, slack, q, f = fm.MODES["floor"]
    sums, marks, n_pos = sums_of(seed, "floor")
    path = fm.write(tmp_path, fm.fuzz(seed), block=1024)                         # (sub-ranges want at least 64 blocks a piece)
    d = engine.DeviceBam(path)
    assert d.n_blocks >= 256 and not tabled and f == fm.NONE
    try:
        ctx.set_option("split_sub", 2)
        ctx.set_min_base_quality(q)
        taken = ctx.stat("split_sub_taken")
        ld, n_words = td.split_words(n_pos, 1)
        t = torch.zeros(n_words, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()                                                # torch's stream is not the context's
        hook = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)(lambda user, p, n, stream: 0)
        rc, rs, _ = td._split_step(ctx, d, 0, 1, n_pos, ld, t, 10, True, hook, None)
        assert rc == 0 and ctx.stat("split_sub_taken") == taken + 1
        for cols in (sparse_columns(seed, n_pos), list(range(n_pos))):
            not_vacuous(sums, marks, cols, ("sub-ranges", len(cols)))
            msg = differ(device_counts(ctx, rs, cols), take(sums, cols), cols, ("sub-ranges", len(cols)))
            assert not msg, msg
        rs.free()
    finally:
        ctx.set_option("split_sub", 0)
        ctx.set_min_base_quality()
        d.close()
