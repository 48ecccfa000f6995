"""--indel-table on the GPU (csrc/indel_events.hip; tcmi_readset_indel_events, Context.indel_events): every comparison is exact
equality.  The yardstick is tests/indel_yardstick — the rule of include/tcmi.h restated over the records —, the invariant is that the
insertions anchored on a column add up to the I plane of the matrix the step tallied from the same read set.  The inputs are those of
tests/test_floor_mask_fuzz.py (tests/fuzz_masked.specs: every CIGAR op, SEQ '*', short SEQ, no QUAL, long reads, planted insertion
sites) and a hand-built file with many different events on one column (tests/indel_cases.many_keys).  Every host buffer lies between
guard words that are checked after every call.  The rule, the hash, the writer and the argument handling are checked without a GPU in
tests/test_indel_rule.py."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import cli_run as cr
from tests import fuzz_masked as fm
from tests import indel_yardstick as iy
from tests import read_specs as rsp
from tests import repeat_bam as rb
from tests import variant_yardstick as vy
from tests.device_file import uploaded
from tests.indel_cases import COL, EVERYTHING, LDS, N_SHARED, OTHERS, SHARED, TENTH, L, colliding_pair, device_events, differ, fuzz_events, many_keys, \
    not_vacuous, sparse_columns
from trueconsense_amd import _ffi, engine
from trueconsense_amd import distributed as td
from trueconsense_amd.io import bamwriter

pytestmark = pytest.mark.gpu
SC_BLOCK, SC_WG_PER_CU = rb.stream_count_caps()


@pytest.fixture(scope="module")
def ctx():
    with engine.Context(0) as c:
        yield c


def want_of(counts, totals, cols, cov, rule):
    return iy.reported(counts, cols, cov, **rule), iy.totals_at(totals, cols)


# ---- 1. fuzz against the yardstick -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_sync", (1, 0))
@pytest.mark.parametrize("mode", sorted(fm.MODES))
@pytest.mark.parametrize("seed", fm.SEEDS)
def test_fuzz_equals_the_yardstick_and_adds_up_to_the_matrix(ctx, tmp_path, seed, mode, one_sync):
    tabled, slack, q, f = fm.MODES[mode]
    counts, totals, whole = fuzz_events(seed, mode)
    n_pos = len(whole)
    queries = (list(range(n_pos)), sparse_columns(seed, counts, n_pos))
    assert len(queries[1]) <= LDS < len(queries[0])
    for cols in queries:
        not_vacuous(counts, cols, whole[cols, 0], (seed, mode, len(cols)))
    path = fm.write(tmp_path, fm.fuzz(seed))
    with uploaded(ctx, path, fm.table_of(seed) if tabled else (), q, f, slack, one_sync) as rs:
        matrix = ctx.step(rs, n_pos, 0, True)[3]
        assert np.array_equal(matrix, whole)
        for cols in queries:
            cov = matrix[cols, 0]
            for rule in (EVERYTHING, TENTH):
                want, want_tot = want_of(counts, totals, cols, cov, rule)
                got, got_tot = device_events(ctx, rs, cols, cov, **rule)
                msg = differ(got, want, (seed, mode, one_sync, len(cols), rule["num"]))
                assert not msg, msg
                assert np.array_equal(got_tot, want_tot), (seed, mode, len(cols))
                assert np.array_equal(got_tot["ins_total"], matrix[cols, 6]), "the insertions do not add up to the I plane"
                assert (got_tot["del_total"] <= cov).all()


# ---- 2.-4. one wave, many keys; growth; collisions -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def keys_file(tmp_path_factory):
    specs, by_hand = many_keys()
    counts, totals = iy.events(specs)
    assert counts == by_hand                                                    # the yardstick reads the file as it was written
    # before the GPU is asked: one insertion on more than 64 consecutive records (several wavefronts, two workgroups), three others of
    # its length, one of another, deletions of 3 and of 9 on the same column, singletons, a record with both kinds
    names = [r["name"] for r in specs]
    first = names.index("shared0")
    assert names[first:first + N_SHARED] == ["shared%d" % k for k in range(N_SHARED)] and N_SHARED > 64 and first // SC_BLOCK != (first + N_SHARED - 1) // SC_BLOCK
    assert counts[(COL, iy.INS, 3, SHARED)] == N_SHARED and all(counts[(COL, iy.INS, 3, s)] > 1 for s in OTHERS)
    assert counts[(COL, iy.INS, 4, "ACGT")] == 8 and counts[(COL, iy.DEL, 3, "")] == 12 and counts[(COL, iy.DEL, 9, "")] == 7 and counts[(COL, iy.DEL, 1, "")] == 1
    assert sum(n == 1 for n in counts.values()) >= 12 and len(counts) > 16 and {ev[0] for ev in counts} == {COL}
    path = fm.write(tmp_path_factory.mktemp("keys"), specs)
    return path, counts, totals


def keys_answer(ctx, path, **options):
    try:
        for k, v in options.items():
            ctx.set_option(k, v)
        with uploaded(ctx, path) as rs:
            cov = ctx.step(rs, L, 0, True)[3][[COL], 0]
            return [device_events(ctx, rs, [COL], cov, **rule) for rule in (EVERYTHING, TENTH)], cov
    finally:
        ctx.set_option("indel_slots", 15)
        ctx.set_option("indel_hash_bits", 34)


def test_one_wave_many_keys(ctx, keys_file):
    path, counts, totals = keys_file
    answers, cov = keys_answer(ctx, path)
    for (got, got_tot), rule in zip(answers, (EVERYTHING, TENTH)):
        want, want_tot = want_of(counts, totals, [COL], cov, rule)
        assert not differ(got, want, ("many keys", rule["num"])), differ(got, want, ("many keys", rule["num"]))
        assert np.array_equal(got_tot, want_tot)
    assert len(answers[0][0]) == len(counts) > len(answers[1][0]) >= 1


def test_a_small_table_grows(ctx, keys_file):
    path, counts, _ = keys_file
    plain, _ = keys_answer(ctx, path)
    grown0 = ctx.stat("indel_table_grown")
    small, _ = keys_answer(ctx, path, indel_slots=4)                            # 16 slots for more than 16 keys
    assert [a[0] for a in small] == [a[0] for a in plain] and all(np.array_equal(a[1], b[1]) for a, b in zip(small, plain))
    assert ctx.stat("indel_table_grown") - grown0 >= 1


def test_a_collision_takes_the_next_seed_and_no_hash_at_all_is_refused(ctx, keys_file):
    path, counts, _ = keys_file
    a, b = colliding_pair()
    assert a != b and counts[(COL, iy.INS, 5, a)] and counts[(COL, iy.INS, 5, b)]
    assert engine.indel_hash(0, [iy.ss.NT16.index(x) for x in a], 8) == engine.indel_hash(0, [iy.ss.NT16.index(x) for x in b], 8)
    every = [[iy.ss.NT16.index(x) for x in ev[3]] for ev in counts if ev[1] == iy.INS]
    assert len({engine.indel_hash(1, nib, 8) for nib in every}) == len(every)   # under seed 1 no two insertions of the file share a hash
    plain, _ = keys_answer(ctx, path)
    retried0 = ctx.stat("indel_hash_retried")
    with uploaded(ctx, path) as rs:
        cov = ctx.step(rs, L, 0, True)[3][[COL], 0]
        try:
            ctx.set_option("indel_hash_bits", 8)
            got = device_events(ctx, rs, [COL], cov, **EVERYTHING)              # (the sizing call and the call: one retry each; the short-buffer call: one more)
            assert got[0] == plain[0][0] and np.array_equal(got[1], plain[0][1])
            assert ctx.stat("indel_hash_retried") - retried0 == 3
            retried0 = ctx.stat("indel_hash_retried")
            ctx.indel_events(rs, [COL], cov, min_af="0", min_depth=0)
            assert ctx.stat("indel_hash_retried") - retried0 == 1
            ctx.set_option("indel_hash_bits", 0)
            with pytest.raises(_ffi.TcmiError) as e:
                ctx.indel_events(rs, [COL], cov, min_af="0", min_depth=0)
            assert e.value.code == _ffi.E_UNSUPPORTED and "seeds" in str(e.value)
        finally:
            ctx.set_option("indel_hash_bits", 34)
        got = device_events(ctx, rs, [COL], cov, **EVERYTHING)                  # a clean error path: the context answers as before
        assert got[0] == plain[0][0]


# ---- 5. past one trip of the grid ------------------------------------------------------------------------------------------------------
def test_more_records_than_one_trip_of_the_grid(ctx, tmp_path):
    seed, mode = 2, "all"
    tabled, slack, q, f = fm.MODES[mode]
    counts, totals, whole = fuzz_events(seed, mode)
    n_pos = len(whole)
    cap = ctx.stat("compute_units") * SC_WG_PER_CU * SC_BLOCK
    specs = fm.fuzz(seed)
    r = cap // len(specs) + 1
    r += r % 2 == 0
    src = fm.write(tmp_path, specs)
    dst = str(tmp_path / "R.bam")
    n = rb.repeat_records(src, dst, r)
    assert n == r * len(specs) > cap
    last = max(i for i, x in enumerate(specs) if iy.kept(x, f) and iy.record_events(x, fm.table_of(seed), q, slack))
    assert last * r >= cap, "no record of the second trip has an event"
    cols = list(range(n_pos))
    with uploaded(ctx, dst, fm.table_of(seed), q, f, slack) as rs:
        assert rs.n_reads == n
        matrix = ctx.step(rs, n_pos, 0, True)[3]
        assert np.array_equal(matrix, r * whole)
        cov = matrix[cols, 0]
        for rule in (EVERYTHING, TENTH):
            want = iy.reported({ev: r * k for ev, k in counts.items()}, cols, cov, **rule)
            got, got_tot = device_events(ctx, rs, cols, cov, **rule)
            assert not differ(got, want, ("repeated", r, rule["num"])), differ(got, want, ("repeated", r, rule["num"]))
            assert np.array_equal(got_tot["ins_total"], matrix[cols, 6]) and np.array_equal(got_tot["ins_total"], r * iy.totals_at(totals, cols)["ins_total"])


# ---- 6. sub-ranges ---------------------------------------------------------------------------------------------------------------------
def test_sub_ranges_merge_to_the_single_context_answer(ctx, tmp_path):
    import torch
    seed = fm.SEEDS[3]
    tabled, slack, q, f = fm.MODES["all"]
    table = fm.table_of(seed)
    counts, totals, whole = fuzz_events(seed, "all")
    n_pos = len(whole)
    # (sub-ranges want at least 64 blocks a piece: the same records four times over in 1 024-byte blocks, four times the counts)
    big = sorted([dict(x, name="%s_%d" % (x["name"], k)) for k in range(4) for x in fm.fuzz(seed)], key=lambda x: x["pos"])
    path4 = str(tmp_path / "A4.bam")
    bamwriter.write_bam(path4, rsp.arrays(big), ref_len=L, block=1024)
    cols = list(range(n_pos))
    cov = 4 * whole[cols, 0]
    with uploaded(ctx, path4, table, q, f, slack) as rs:
        single = [device_events(ctx, rs, cols, cov, **rule) for rule in (EVERYTHING, TENTH)]
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
        for rule, (want, want_tot) in zip((EVERYTHING, TENTH), single):
            got, got_tot = device_events(c, rs, cols, cov, **rule)
            assert not differ(got, want, ("sub-ranges", rule["num"])), differ(got, want, ("sub-ranges", rule["num"]))
            assert np.array_equal(got_tot, want_tot)
            assert got == iy.reported({ev: 4 * k for ev, k in counts.items()}, cols, cov, **rule)
        rs.free()
    finally:
        d.close()
        c.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_empty_read_set(ctx, tmp_path):
    specs = fm.fuzz(fm.SEEDS[0])
    pa = fm.write(tmp_path, specs[:400])
    pb_ = str(tmp_path / "B.bam")
    bamwriter.write_bam(pb_, rsp.arrays(specs[400:700]), ref_len=L, block=4096)
    da, db = engine.DeviceBam(pa), engine.DeviceBam(pb_)
    cols, cov = [10, 500, 1500], [5, 5, 5]
    try:
        ra = ctx.upload_bamfile(da)
        ctx.indel_events(ra, cols, cov)
        for bad, word in (([5, 5], "strictly ascending"), ([3, 1 << 29], "2^29"), ([-1, 4], "2^29")):
            with pytest.raises(_ffi.TcmiError) as e:
                ctx.indel_events(ra, bad, [1] * len(bad))
            assert e.value.code == _ffi.E_ARG and word in str(e.value), (bad, str(e.value))
        for kw, word in ((dict(min_alt_depth=0), "min_alt_depth"), (dict(min_depth=-1), "min_depth")):
            with pytest.raises(_ffi.TcmiError) as e:
                ctx.indel_events(ra, cols, cov, **kw)
            assert e.value.code == _ffi.E_ARG and word in str(e.value), (kw, str(e.value))
        with pytest.raises(_ffi.TcmiError) as e:
            ctx.indel_events(ra, cols, [5, -1, 5])
        assert e.value.code == _ffi.E_ARG and "negative" in str(e.value)
        rb_ = ctx.upload_bamfile(db)                                            # another upload on the context: ra's stream is displaced
        with pytest.raises(_ffi.TcmiError) as e:
            ctx.indel_events(ra, cols, cov)
        assert e.value.code == _ffi.E_UNSUPPORTED and "no longer resident" in str(e.value)
        ctx.indel_events(rb_, cols, cov)                                        # the newer one answers
        ra.free()
        rb_.free()
    finally:
        da.close()
        db.close()
    bam = engine.BamFile(pa)
    flat = ctx.upload(bam)                                                      # flat arrays: packed, but no record stream
    with pytest.raises(_ffi.TcmiError) as e:
        ctx.indel_events(flat, cols, cov)
    assert e.value.code == _ffi.E_UNSUPPORTED and "not decoded on the device" in str(e.value)
    flat.free()
    bam.close()
    with uploaded(ctx, pa, (), 13, (0, 0x1000, 0)) as rs:                       # a FLAG bit no record has is required: every record fails
        assert rs.n_piled == 0
        ev, text, tot = ctx.indel_events(rs, cols, cov)
        assert len(ev) == 0 and text == b"" and tot["pos"].tolist() == cols and not tot["ins_total"].any() and not tot["del_total"].any()


def test_the_launches_are_profiled_and_nothing_runs_without_the_call(ctx, tmp_path):
    path = fm.write(tmp_path, fm.fuzz(fm.SEEDS[0])[:500])
    try:
        ctx.profile(True)
        with uploaded(ctx, path) as rs:
            ctx.step(rs, L, 10, True)
            assert ctx.profile_get(_ffi.K_INDEL_EVENTS)[1] == 0
            ctx.indel_events(rs, [100, 900], [9, 9])
            ms, n = ctx.profile_get(_ffi.K_INDEL_EVENTS)
            assert n == 1 and ms > 0
    finally:
        ctx.profile(False)


# ---- 8. the command line ---------------------------------------------------------------------------------------------------------------
RULE = dict(num=1, den=20, min_alt_depth=2, min_depth=10)
RULE_FLAGS = ["--min-af", "1/20", "--min-alt-depth", "2", "--variant-min-depth", "10", "--min-baseq", "13"]


def table_of_yardstick(specs, ref, region, n_ref, least=3):
    """the records on one reference -> (the variant table's records, --indel-table's rows) from the yardsticks alone, floor 13"""
    from tests import primer_yardstick as py
    kept = [dict(x, tid=0) for x in specs]
    matrix = py.counts(rsp.arrays(kept), n_ref, (), 13)[0]
    recs = vy.records(matrix, ref.encode(), RULE["num"], RULE["den"], RULE["min_alt_depth"], RULE["min_depth"])
    cols = sorted({p for p, a, *_ in recs if a in (5, 6)})
    cov = [int(matrix[c, 0]) for c in cols]
    counts, totals = iy.events(kept, (), 13)
    rep = iy.reported(counts, cols, cov, **RULE)
    rows = iy.text(rep, region, ref.encode())
    assert engine.indels_text(*iy.arrays(rep), iy.totals_at(totals, cols), vy.as_array(recs), region, ref) == rows
    kinds = [t[1] for t in rep]
    assert kinds.count(iy.INS) >= least and kinds.count(iy.DEL) >= least and len(rep) < len([ev for ev in counts if ev[0] in cols]), (region, len(rep))
    return recs, rows


def test_cli_single_sample_and_per_contig(tmp_path, monkeypatch):
    from trueconsense_amd import synthetic as syn
    monkeypatch.chdir(tmp_path)
    ref = syn.make_reference(seed=3, L=L, cds=[])[0]
    orfs = syn.make_reference(seed=3, L=L, cds=[(100, 900)])[1]
    specs = fm.fuzz(1)
    recs, rows = table_of_yardstick(specs, ref, "ref", L)
    bamwriter.write_bam("A.bam", rsp.arrays(specs), ref_len=L, block=4096)
    common = cr.setup_cli(ref, orfs) + RULE_FLAGS
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + cr.out_args("a") + ["--variant-table", "a.var", "--indel-table", "a.ind", "--stats", "a.json"])
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + cr.out_args("b") + ["--variant-table", "b.var", "--stats", "b.json"])
    assert open("a.ind").read() == engine.INDELS_HEADER + rows and not os.path.exists("b.ind")
    assert open("a.var").read() == open("b.var").read() == engine.VARIANTS_HEADER + vy.text(recs, "ref", ref.encode())
    assert cr.outputs("a") == cr.outputs("b")                                   # every other output byte for byte
    import json
    sa, sb = json.load(open("a.json")), json.load(open("b.json"))
    assert sorted(sa) == sorted(sb) and {k: v for k, v in sa.items() if k != "seconds"} == {k: v for k, v in sb.items() if k != "seconds"}

    # --per-contig: each contig's rows on its own positions
    parts, every = fm.contig_case()
    refs = [(name, ln) for name, ln, _ in fm.CONTIGS]
    seqs = [(name, syn.make_reference(seed=3, L=ln, cds=[])[0]) for name, ln in refs]
    bamwriter.write_bam("P.bam", rsp.arrays(every), refs=refs, block=4096)
    cr.setup_contigs(seqs, [(name, syn.make_reference(seed=3, L=ln, cds=[(100, 700)])[1]) for name, ln in refs])
    want_var, want_ind = "", ""
    for (name, ln, _, part), (_, seq) in zip(parts, seqs):
        r, rows_t = table_of_yardstick(part, seq, name, ln, least=1)
        want_var += vy.text(r, name, seq.encode())
        want_ind += rows_t
    flags = ["-i", "P.bam", "-ref", "r.fa", "-gff", "g.gff", "-cov", "10", "-name", "S", "--per-contig"] + RULE_FLAGS
    cr.run_cli(monkeypatch, flags + ["-o", "p.fa", "--variant-table", "p.var", "--indel-table", "p.ind"])
    cr.run_cli(monkeypatch, flags + ["-o", "q.fa", "--variant-table", "q.var"])
    assert open("p.ind").read() == engine.INDELS_HEADER + want_ind
    assert open("p.var").read() == open("q.var").read() == engine.VARIANTS_HEADER + want_var and open("p.fa").read() == open("q.fa").read()
