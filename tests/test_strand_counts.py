"""--variant-strand on the GPU (csrc/strand_counts.hip; tcmi_readset_strand_counts, Context.strand_counts): every comparison is exact
equality.  The yardstick is tests/strand_yardstick.counts — tests/primer_yardstick.counts applied to the FLAG-0x10-clear records and to
the FLAG-0x10-set records —, the invariant is fwd + rev == the matrix the step tallied from the same read set, and the independent
device route is the matrix of the same file uploaded under exclude_flags | 0x10 and require_flags | 0x10.  The inputs are those of
tests/test_floor_mask_fuzz.py (tests/fuzz_masked.specs: every CIGAR op, SEQ '*', short SEQ, no QUAL, long reads, planted insertion
sites, FLAG 16 on a third of the records).  The host record buffer lies between guard words that are checked after every call.  The
rule, the writer and the argument handling are checked without a GPU in tests/test_strand_rule.py."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from tests import cli_run as cr
from tests import device_file as dvf
from tests import fuzz_masked as fm
from tests import primer_yardstick as py
from tests import read_specs as rsp
from tests import strand_yardstick as sy
from tests import variant_yardstick as vy
from tests.device_file import uploaded
from tests.strand_cases import LDS, G, L, device_counts, differ, halves, not_vacuous, one_column_a_record, sparse_columns
from trueconsense_amd import TrueConsense as cli
from trueconsense_amd import _ffi, contigs, engine
from trueconsense_amd import distributed as td
from trueconsense_amd import synthetic as syn
from trueconsense_amd.io import bamwriter
from trueconsense_amd.io import primers as pbed

pytestmark = pytest.mark.gpu
assert fm.FLAGS.count(16) == 2 and len(fm.FLAGS) == 6


@pytest.fixture(scope="module")
def ctx():
    with engine.Context(0) as c:
        yield c


# ---- 1. both routes, three modes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_sync", (1, 0))
@pytest.mark.parametrize("mode", sorted(fm.MODES))
@pytest.mark.parametrize("seed", fm.SEEDS)
def test_both_routes_equal_the_yardstick_and_add_up_to_the_matrix(ctx, tmp_path, seed, mode, one_sync):
    tabled, slack, q, f = fm.MODES[mode]
    specs, _ = fm.passing(seed, None, None, f)
    fwd, rev, n_pos = halves(seed, mode)
    sparse, dense = sparse_columns(seed, n_pos), list(range(n_pos))
    assert len(sparse) <= LDS < len(dense)
    for cols in (sparse, dense):
        not_vacuous(specs, fwd[cols], rev[cols], cols, (seed, mode))
    path = fm.write(tmp_path, fm.fuzz(seed))
    with uploaded(ctx, path, fm.table_of(seed) if tabled else (), q, f, slack, one_sync) as rs:
        matrix = ctx.step(rs, n_pos, 0, True)[3]
        for route, cols in (("LDS", sparse), ("memory", dense)):
            got = device_counts(ctx, rs, cols)
            msg = differ(got, (fwd[cols], rev[cols]), cols, (seed, mode, one_sync, route))
            assert not msg, msg
            assert np.array_equal(got[0] + got[1], matrix[cols]), (seed, mode, one_sync, route, "the invariant")


# ---- 2. the independent device route -------------------------------------------------------------------------------------------------
def test_each_strand_equals_the_matrix_of_the_file_filtered_by_flag_0x10(ctx, tmp_path):
    seed = fm.SEEDS[0]
    tabled, slack, q, f = fm.MODES["all"]
    specs, _ = fm.passing(seed, None, None, f)
    fwd, rev, n_pos = halves(seed, "all")
    cols = list(range(n_pos))
    not_vacuous(specs, fwd, rev, cols, seed)
    path = fm.write(tmp_path, fm.fuzz(seed))
    table = fm.table_of(seed)
    only_fwd = dvf.through(ctx, "one_sync", path, table, n_pos, q, (f[0], f[1], f[2] | 0x10), slack)[0]
    only_rev = dvf.through(ctx, "one_sync", path, table, n_pos, q, (f[0], f[1] | 0x10, f[2]), slack)[0]
    assert only_fwd.any() and only_rev.any() and not np.array_equal(only_fwd, only_rev)
    with uploaded(ctx, path, table, q, f, slack) as rs:
        got = device_counts(ctx, rs, cols)
    msg = differ(got, (only_fwd, only_rev), cols, "against the device's own matrices")
    assert not msg, msg


# ---- 3. the staging edge -------------------------------------------------------------------------------------------------------------
def test_the_largest_staged_query_and_the_smallest_in_memory(ctx, tmp_path):
    seed = fm.SEEDS[1]
    specs, _ = fm.passing(seed)
    fwd, rev, n_pos = halves(seed, "floor")
    cols = sorted(int(c) for c in np.random.default_rng(9).choice(n_pos, LDS + 1, replace=False))
    not_vacuous(specs, fwd[cols[:LDS]], rev[cols[:LDS]], cols[:LDS], seed)
    path = fm.write(tmp_path, fm.fuzz(seed))
    with uploaded(ctx, path, (), 13) as rs:
        staged, memory = device_counts(ctx, rs, cols[:LDS]), device_counts(ctx, rs, cols)
    assert not differ(staged, (fwd[cols[:LDS]], rev[cols[:LDS]]), cols, "staged")
    assert not differ(memory, (fwd[cols], rev[cols]), cols, "memory")
    assert np.array_equal(staged[0], memory[0][:LDS]) and np.array_equal(staged[1], memory[1][:LDS])


# ---- 4. small and ragged -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rec", (1, 63, 65, 257))
def test_small_files(ctx, tmp_path, n_rec):
    """1, 63, 65 and 257 records (fewer than a wavefront, one more, one more than a workgroup); a column nobody covers, a column beyond
    every read; the same records under a filter that all of them fail: zeros, and TCMI_OK"""
    every = [r for r in fm.fuzz(fm.SEEDS[2]) if fm._piles_up(r)]
    step = len(every) // n_rec
    specs = every[::step][:n_rec] if n_rec > 1 else [next(r for r in every if r["flag"] & 16 and fm._span(r) > 20)]
    assert len(specs) == n_rec
    rd = rsp.arrays(specs)
    whole = py.counts(rd, L, (), 13)[0]
    n_pos = len(whole)
    beyond = n_pos + 700
    bare = [c for c in range(n_pos) if not whole[c].any()]
    assert bare and whole[:, 0].any()
    dense = list(range(n_pos)) + [beyond]
    sparse = sorted(set(int(c) for c in np.random.default_rng(n_rec).choice(n_pos, 60, replace=False)) | {bare[0], int(np.argmax(whole[:, 0])), beyond})
    want = sy.counts(rd, dense, L, (), 13)
    path = fm.write(tmp_path, specs)
    with uploaded(ctx, path, (), 13) as rs:
        assert rs.n_reads == n_rec
        matrix = ctx.step(rs, n_pos, 0, True)[3]
        for cols in (sparse, dense):
            idx = [dense.index(c) for c in cols]
            got = device_counts(ctx, rs, cols)
            msg = differ(got, (want[0][idx], want[1][idx]), cols, (n_rec, len(cols)))
            assert not msg, msg
            assert np.array_equal((got[0] + got[1])[:-1], matrix[cols[:-1]]) and not got[0][-1].any() and not got[1][-1].any()
            k = cols.index(bare[0])
            assert not got[0][k].any() and not got[1][k].any()
    with uploaded(ctx, path, (), 13, (0, 0x1000, 0)) as rs:                     # a FLAG bit no record has is required: every record fails
        assert rs.n_reads == n_rec and rs.n_piled == 0 and rs.filtered == n_rec
        got = device_counts(ctx, rs, sparse)
        assert not got[0].any() and not got[1].any()


# ---- 5. depth ------------------------------------------------------------------------------------------------------------------------
def test_many_lanes_on_one_counter(ctx, tmp_path):
    """every random read starts inside a window of 50 columns: depth past 255 on one column, the sums stay exact"""
    seed, window = fm.DEEP_SEED, fm.DEEP_WINDOW
    tabled, slack, q, f = fm.MODES["all"]
    specs, _ = fm.passing(seed, None, window, f)
    fwd, rev, n_pos = halves(seed, "all", window)
    sparse = sorted(set(range(window[0] - 20, window[1] + 60, 3)) | set(sparse_columns(seed, n_pos, 20)))[:LDS]
    dense = list(range(n_pos))
    assert (fwd[sparse, 0] + rev[sparse, 0]).max() >= 256 and min(fwd[sparse, 0].max(), rev[sparse, 0].max()) >= 64
    not_vacuous(specs, fwd[sparse], rev[sparse], sparse, "deep")
    path = fm.write(tmp_path, fm.fuzz(seed, None, window))
    with uploaded(ctx, path, fm.table_of(seed), q, f, slack) as rs:
        matrix = ctx.step(rs, n_pos, 0, True)[3]
        for cols in (sparse, dense):
            got = device_counts(ctx, rs, cols)
            msg = differ(got, (fwd[cols], rev[cols]), cols, ("deep", len(cols)))
            assert not msg, msg
            assert np.array_equal(got[0] + got[1], matrix[cols])


# ---- 5b. the join's worst case ---------------------------------------------------------------------------------------------------------


def test_a_wavefront_on_64_columns_and_a_ragged_one_behind_it(ctx, tmp_path):
    """the records of one_column_a_record at one column per record, staged; and the same query padded past the LDS capacity with
    columns beyond every read, counted in memory"""
    specs, cols = one_column_a_record()
    rd = rsp.arrays(specs)
    n_pos = len(py.counts(rd, L)[0])
    padded = cols + [n_pos + 700 + j for j in range(LDS + 1 - len(cols))]
    assert len(specs) == 65 and len(cols) == 64 <= LDS < len(padded) and cols[-1] < n_pos
    want = sy.counts(rd, padded, L)
    cov = (want[0] + want[1])[:, 0].tolist()
    assert cov == [2] + [1] * 63 + [0] * (len(padded) - 64) and want[0][0, 0] == 1 and want[1][0, 0] == 1, cov
    path = fm.write(tmp_path, specs)
    with uploaded(ctx, path) as rs:
        assert rs.n_reads == 65 and rs.n_piled == 65
        matrix = ctx.step(rs, n_pos, 0, True)[3]
        for route, q in (("LDS", cols), ("memory", padded)):
            got = device_counts(ctx, rs, q)
            msg = differ(got, (want[0][:len(q)], want[1][:len(q)]), q, ("one column a record", route))
            assert not msg, msg
            assert np.array_equal((got[0] + got[1])[:64], matrix[cols]) and not got[0][64:].any() and not got[1][64:].any()


# ---- 6. a contig layout ----------------------------------------------------------------------------------------------------------------
def test_two_contigs_under_a_layout(ctx, tmp_path):
    """columns in both slots and one in the guard between them; each contig under its own table, floor 13 and the read filter"""
    parts, specs = fm.contig_case()
    refs = [(name, ln) for name, ln, _ in fm.CONTIGS]
    names = [n for n, _ in refs]
    path = str(tmp_path / "A.bam")
    bamwriter.write_bam(path, rsp.arrays(specs), refs=refs, block=4096)
    recs = [(name, syn.make_reference(seed=3, L=ln, cds=[])[0]) for name, ln in refs]
    shift, slot, axis = contigs.layout_for(recs, names, [ln for _, ln in refs])
    rows = pbed.rows_for_layout([(name, s, e, rev) for name, _, table, _ in parts for s, e, rev in table], names, shift)
    guard = int(shift[1]) - 1
    assert guard >= int(shift[0]) + refs[0][1]
    cols, want_f, want_r = [], [], []
    for t, (name, ln, table, part) in enumerate(parts):
        kept = [dict(r, tid=0) for r in rsp.kept(part, fm.F)[0]]
        own = list(range(ln))
        fwd, rev = sy.counts(rsp.arrays(kept), own, ln, table, 13)
        not_vacuous(kept, fwd, rev, own, name)
        cols += [c + int(shift[t]) for c in own] + ([guard] if t == 0 else [])
        want_f += [fwd] + ([np.zeros((1, 7), np.int32)] if t == 0 else [])
        want_r += [rev] + ([np.zeros((1, 7), np.int32)] if t == 0 else [])
    assert cols == sorted(cols) and len(cols) > LDS
    want = (np.concatenate(want_f), np.concatenate(want_r))
    try:
        ctx.set_layout(shift, slot)
        with uploaded(ctx, path, rows, 13, fm.F) as rs:
            matrix = ctx.step(rs, axis, 0, True)[3]
            at = cols.index(guard)
            for use in (cols, cols[at - 100:at + 100]):                         # (the memory route, and a staged query that holds the guard column)
                k0 = cols.index(use[0])
                got = device_counts(ctx, rs, use)
                msg = differ(got, (want[0][k0:k0 + len(use)], want[1][k0:k0 + len(use)]), use, ("layout", len(use)))
                assert not msg, msg
                assert np.array_equal(got[0] + got[1], matrix[use]) and guard in use
            ctx.set_layout()                                                    # cleared: the read set still answers
            assert not differ(device_counts(ctx, rs, cols), want, cols, "layout cleared")
            ctx.set_layout(shift, slot)                                         # set once more: another generation
            with pytest.raises(_ffi.TcmiError) as e:
                ctx.strand_counts(rs, cols)
            assert e.value.code == _ffi.E_UNSUPPORTED and "layout" in str(e.value)
    finally:
        ctx.set_layout()


# ---- 7. block ranges -------------------------------------------------------------------------------------------------------------------
def test_block_ranges_and_sub_ranges_add_up_to_the_file(ctx, tmp_path):
    """records that straddle 4 096-byte BGZF blocks: three block ranges taken in turn add up to the whole file's counts, and a read set
    of two sub-ranges (tcmi_split_step, "split_sub") answers with the same"""
    import torch
    seed = fm.SEEDS[3]
    tabled, slack, q, f = fm.MODES["all"]
    specs, _ = fm.passing(seed, None, None, f)
    fwd, rev, n_pos = halves(seed, "all")
    table = fm.table_of(seed)
    path = fm.write(tmp_path, fm.fuzz(seed), block=4096, split_records=True)
    for cols in (sparse_columns(seed, n_pos), list(range(n_pos))):
        not_vacuous(specs, fwd[cols], rev[cols], cols, seed)
        with uploaded(ctx, path, table, q, f, slack) as rs:
            whole = device_counts(ctx, rs, cols)
        assert not differ(whole, (fwd[cols], rev[cols]), cols, "straddled")
        d = engine.DeviceBam(path)
        n_blocks = d.n_blocks
        d.close()
        assert n_blocks > 60
        total, n_reads = [np.zeros_like(whole[0]), np.zeros_like(whole[1])], 0
        for rank in range(3):
            with uploaded(ctx, path, table, q, f, slack, blocks=td.block_range(n_blocks, rank, 3)) as rs:
                got = device_counts(ctx, rs, cols)
                total[0] += got[0]
                total[1] += got[1]
                n_reads += rs.n_reads
        assert n_reads == len(fm.fuzz(seed)) and not differ(total, whole, cols, "three ranges")
    # (sub-ranges want at least 64 blocks a piece: the same records four times over in 1 024-byte blocks, four times the counts)
    big = sorted([dict(r, name="%s_%d" % (r["name"], k)) for k in range(4) for r in fm.fuzz(seed)], key=lambda r: r["pos"])
    path4 = str(tmp_path / "A4.bam")
    bamwriter.write_bam(path4, rsp.arrays(big), ref_len=L, block=1024)
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
        for cols in (sparse_columns(seed, n_pos), list(range(n_pos))):
            assert not differ(device_counts(c, rs, cols), (4 * fwd[cols], 4 * rev[cols]), cols, "sub-ranges")
        rs.free()
    finally:
        d.close()
        c.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, tmp_path):
    specs = fm.fuzz(fm.SEEDS[0])
    pa = fm.write(tmp_path, specs[:400])
    pb_ = str(tmp_path / "B.bam")
    bamwriter.write_bam(pb_, rsp.arrays(specs[400:700]), ref_len=L, block=4096)
    da, db = engine.DeviceBam(pa), engine.DeviceBam(pb_)
    try:
        ra = ctx.upload_bamfile(da)
        ok = ctx.strand_counts(ra, [10, 500, 1500])
        assert ok["fwd"][:, 0].any() and ok["rev"][:, 0].any()
        guarded = dvf.sentinel(2 * G + 16 * 4, np.int32, salt=3).copy()
        for bad, word in (([5, 5], "strictly ascending"), ([7, 5], "strictly ascending"), ([1, 2, 2, 9], "strictly ascending"), ([], "1..1048576"),
                          (np.arange((1 << 20) + 1), "1..1048576"), ([3, 1 << 29], "2^29"), ([-1, 4], "2^29")):
            with pytest.raises(_ffi.TcmiError) as e:
                ctx.strand_counts(ra, bad)
            assert e.value.code == _ffi.E_ARG and word in str(e.value), (bad[:4], str(e.value))
            if 0 < len(bad) <= 4:                                               # ... and nothing is written when the call refuses
                before = guarded.copy()
                rc = _ffi.lib().tcmi_readset_strand_counts(ctx.handle, ra.handle, len(bad), _ffi.ptr(np.ascontiguousarray(bad, np.int64)),
                                                           C.c_void_p(guarded.ctypes.data + 4 * G))
                assert rc == _ffi.E_ARG and np.array_equal(guarded, before)
        rb = ctx.upload_bamfile(db)                                             # another upload on the context: ra's stream is displaced
        with pytest.raises(_ffi.TcmiError) as e:
            ctx.strand_counts(ra, [10, 500])
        assert e.value.code == _ffi.E_UNSUPPORTED and "no longer resident" in str(e.value)
        assert ctx.strand_counts(rb, [10, 500, 1500])["fwd"].any()              # the newer one answers
        ra.free()
        rb.free()
    finally:
        da.close()
        db.close()
    bam = engine.BamFile(pa)
    flat = ctx.upload(bam)                                                      # flat arrays: packed, but no record stream
    with pytest.raises(_ffi.TcmiError) as e:
        ctx.strand_counts(flat, [10, 500])
    assert e.value.code == _ffi.E_UNSUPPORTED and "not decoded on the device" in str(e.value)
    flat.free()
    bam.close()


def test_the_launch_is_profiled_and_nothing_runs_without_the_call(ctx, tmp_path):
    path = fm.write(tmp_path, fm.fuzz(fm.SEEDS[0])[:500])
    try:
        ctx.profile(True)
        with uploaded(ctx, path) as rs:
            ctx.step(rs, L, 10, True)
            assert ctx.profile_get(_ffi.K_STRAND_COUNTS)[1] == 0
            ctx.strand_counts(rs, [100, 900])
            ctx.strand_counts(rs, np.arange(LDS + 1))
            ms, n = ctx.profile_get(_ffi.K_STRAND_COUNTS)
            assert n == 2 and ms > 0
    finally:
        ctx.profile(False)


# ---- 9. the command line ---------------------------------------------------------------------------------------------------------------
CL = 1200
BOTH, FWD_ONLY, LOW_AT = 300, 600, 1100            # the planted alleles' 0-based columns


@functools.lru_cache(maxsize=None)
def cli_case():
    """-> (reference, GFF rows, records): 100-base reads at about 60x over 1 200 columns, the strands in turn up to column 1 000 and
    forward reads only behind it; a base other than the reference's on a third of both strands' reads at BOTH, on half of the forward
    reads at FWD_ONLY, on 40 % of the reads at LOW_AT"""
    rng = np.random.default_rng(77)
    ref, orfs = syn.make_reference(seed=3, L=CL, cds=[(100, 900)])
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}
    specs = []
    for k in range(720):
        pos = int(rng.integers(0, CL - 100 + 1))
        rev = k % 2 == 1 and pos + 100 <= 1000
        seq = list(ref[pos:pos + 100])
        for col, hit in ((BOTH, rng.random() < 0.33), (FWD_ONLY, not rev and rng.random() < 0.5), (LOW_AT, rng.random() < 0.4)):
            if hit and pos <= col < pos + 100:
                seq[col - pos] = other[ref[col].upper()]
        specs.append({"pos": pos, "flag": 16 if rev else 0, "cigar": "100M", "seq": "".join(seq), "name": "r%d" % k, "tid": 0, "qual": 30, "mapq": 60})
    specs.sort(key=lambda r: r["pos"])
    return ref, orfs, specs


def cli_yardstick(specs, ref, rule=(10, 1, 10)):
    """-> (the records, {pos: (fwd, rev)}, the strand array) of the yardsticks at the command line's default thresholds"""
    rd = rsp.arrays(specs)
    whole = py.counts(rd, CL)[0]
    recs = vy.records(whole, ref.encode(), 3, 100, 1, 10)
    cols = sorted({p for p, *_ in recs})
    fwd, rev = sy.counts(rd, cols, CL)
    assert np.array_equal(fwd + rev, whole[cols])
    return recs, {c: (fwd[k], rev[k]) for k, c in enumerate(cols)}, sy.records(cols, fwd, rev)


def test_cli_single_sample_per_contig_and_split(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ref, orfs, specs = cli_case()
    recs, strand, strand_arr = cli_yardstick(specs, ref)
    want = engine.variants_strand_text(vy.as_array(recs), strand_arr, "ref", ref)
    assert want == sy.text(recs, strand, "ref", ref.encode(), 10, 1, 10)
    verdict_at = {int(ln.split("\t")[1]) - 1: ln.split("\t")[-1] for ln in want.splitlines()}
    assert (verdict_at[BOTH], verdict_at[FWD_ONLY], verdict_at[LOW_AT]) == ("PASS", "BIAS", "LOW"), verdict_at
    bamwriter.write_bam("A.bam", rsp.arrays(specs), ref_len=CL, block=4096)
    common = cr.setup_cli(ref, orfs)
    out = lambda t: ["-o", t + ".fa", "-vcf", t + ".vcf", "-ogff", t + ".gff", "-doc", t + ".tsv"]
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + out("a") + ["--variant-table", "a.var", "--variant-strand", "--stats", "a.json"])
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + out("b") + ["--variant-table", "b.var", "--stats", "b.json"])
    got, plain = open("a.var").read(), open("b.var").read()
    assert got == engine.VARIANTS_STRAND_HEADER + want
    assert [ln.split("\t")[:7] for ln in got.splitlines()] == [ln.split("\t") for ln in plain.splitlines()] and plain.startswith(engine.VARIANTS_HEADER)
    assert cr.outputs("a") == cr.outputs("b")
    sa, sb = json.load(open("a.json")), json.load(open("b.json"))
    n_bias, n_low = (sum(v == w for v in (ln.split("\t")[-1] for ln in want.splitlines())) for w in ("BIAS", "LOW"))
    assert (sa["variant_strand_bias"], sa["variant_strand_low"]) == (n_bias, n_low) and n_bias > 0 and n_low > 0
    assert (sb["variant_strand_bias"], sb["variant_strand_low"]) == (0, 0) and sa["variant_records"] == sb["variant_records"] == len(recs)
    # other thresholds
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + ["-o", "c.fa", "--variant-table", "c.var", "--variant-strand", "--strand-min-depth", "35",
                                                                      "--strand-ratio", "0.9"])
    assert open("c.var").read() == engine.VARIANTS_STRAND_HEADER + sy.text(recs, strand, "ref", ref.encode(), 35, 9, 10)
    assert [ln.split("\t")[-1] for ln in open("c.var").read().splitlines()[1:]] == ["BIAS", "LOW", "LOW"]

    # --per-contig: the same records on two references of the same sequence: the same rows per region
    two = sorted([dict(r, tid=t, name="%s_%d" % (r["name"], t)) for t in (0, 1) for r in specs], key=lambda r: (r["tid"], r["pos"]))
    bamwriter.write_bam("P.bam", rsp.arrays(two), refs=[("c0", CL), ("c1", CL)], block=4096)
    with open("p.fa", "w") as fh:
        fh.write(">c0\n%s\n>c1\n%s\n" % (ref, ref))
    with open("p.gff", "w") as fh:
        fh.write("##gff-version 3\n" + syn.gff_text(orfs, seqid="c0")[1] + syn.gff_text(orfs, seqid="c1")[1])
    cr.run_cli(monkeypatch, ["-i", "P.bam", "-ref", "p.fa", "-gff", "p.gff", "-cov", "10", "-name", "S", "--per-contig", "-o", "p.fa.out", "--variant-table", "p.var",
                             "--variant-strand", "--stats", "p.json"])
    assert open("p.var").read() == engine.VARIANTS_STRAND_HEADER + want.replace("ref\t", "c0\t") + want.replace("ref\t", "c1\t")
    sp = json.load(open("p.json"))
    assert (sp["variant_strand_bias"], sp["variant_strand_low"], sp["variant_records"]) == (2 * n_bias, 2 * n_low, 2 * len(recs))

    # one file through consensus_split_bamfile at world 1
    parts = td.consensus_split_bamfile("A.bam", CL, cr.gff_rows(orfs), 10, True, "S", 0, 1, return_parts=True,
                                       variant_strand=dict(ref=ref, min_af="0.03", min_alt_depth=1, min_depth=10))
    vrecs, vstrand = parts[-1]
    assert engine.variants_strand_text(vrecs, vstrand, "ref", ref) == want and len(parts) == 4

    # refused: exit 1, nothing written
    man = tmp_path / "m.tsv"
    man.write_text("A.bam\tS0\to0.fa\t-\t-\t-\tt0.var\n")
    cr.write_override("o.csv.gz", py.counts(rsp.arrays(specs), CL)[0])
    before = sorted(os.listdir(tmp_path))
    for argv in (["--batch", str(man)] + common + ["--variant-strand"],
                 ["-i", "A.bam", "-name", "S"] + common + ["-o", "x.fa", "--variant-table", "x.var", "--variant-strand", "--index-override", "o.csv.gz"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 1
    assert sorted(os.listdir(tmp_path)) == before


def test_cli_one_file_over_two_gpus(tmp_path, monkeypatch):
    """--gpus 2 (two ranks rehearsed on this one GPU, gloo for the exchange): rank 0 lists the records and broadcasts their columns, every
    rank counts its own records, rank 0 writes the sum: the rows of the single-GPU run"""
    monkeypatch.chdir(tmp_path)
    ref, orfs, specs = cli_case()
    recs, strand, strand_arr = cli_yardstick(specs, ref)
    bamwriter.write_bam("A.bam", rsp.arrays(specs), ref_len=CL, block=4096, split_records=True)
    common = cr.setup_cli(ref, orfs)
    cr.run_two_ranks(["-i", "A.bam", "-name", "S"] + common + ["-o", "a.fa", "--variant-table", "a.var", "--variant-strand", "--strand-min-depth", "12", "--gpus", "2"])
    assert open("a.var").read() == engine.VARIANTS_STRAND_HEADER + engine.variants_strand_text(vy.as_array(recs), strand_arr, "ref", ref, min_strand_depth=12)
