"""The base-quality floor, the primer mask and the read filter together, on fuzzed inputs (tests/fuzz_masked.py): random CIGARs of
all nine ops (leading D / N / I / P, D D, I behind D through P, = / X, hard clips, SEQ '*', SEQ shorter than the CIGAR, no QUAL),
random long reads (the by_token branch of tally_stream_kernel), random primer tables (overlapping, nested, alternative, with
slack), tables of more than 256 segments (the packer kernels then search the table in global memory, not their LDS copy), depth
past 255 with a different drop word per read, records that straddle BGZF blocks, block ranges, a contig layout.  The yardstick
everywhere is tests/primer_yardstick.counts on the records that pass the read filter; the device is driven through
tests/device_file.through (both packers).  The constructed edges live in test_base_quality.py and test_primer_mask.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import c_oracle
from tests import cli_run as cr
from tests import device_file as dvf
from tests import fuzz_masked as fm
from tests import primer_yardstick as py
from tests import read_specs as rsp
from tests import schemes as sch
from tests.fuzz_masked import CONTIGS, DEEP_SEED, DEEP_WINDOW, MODES, SEEDS, F, L, NONE, contig_case, differ, fuzz, n_long, passing, profile, table_of, write, yardstick
from trueconsense_amd import _ffi, contigs, distributed, engine
from trueconsense_amd import synthetic as sy
from trueconsense_amd.io import bamwriter
from trueconsense_amd.io import primers as pbed


# ------------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("seed", SEEDS)
def test_the_yardsticks_agree_on_the_fuzz(seed):
    """the read-major yardstick (read_tokens with qualities) against the column-major pileup_columns(min_base_quality=q), and at
    q = 0 against the C oracle, on CIGARs neither has seen with per-base qualities"""
    specs, rd = passing(seed)
    n_pos = c_oracle.extent(rd, L)
    for q in (1, 13, 42, 255):
        msg = differ(py.counts(rd, L, (), q)[0], rsp.oracle_counts(rd, q, n_pos), specs, (seed, "q", q))
        assert not msg, msg
    msg = differ(yardstick(seed)[0], c_oracle.tally(rd, n_pos), specs, (seed, "q", 0))
    assert not msg, msg


@pytest.mark.parametrize("seed", SEEDS)
def test_the_inputs_are_not_vacuous(seed):
    """conditions on the generator, per seed, on the records that pass the filter, under the seed's table with slack 3 and floor 13"""
    specs, rd = passing(seed, f=F)                                              # (read_specs.kept: 20 - 60 % of the records fail)
    table = table_of(seed)
    got = profile(specs, table, 3)
    assert got["ops"] == set("MIDNSHP=X"), got
    assert min(got["lead"].values()) >= 30, got
    assert got["long"] >= 15 and got["long_masked"] >= 5, got
    assert got["crossing"] >= 30, got
    assert min(got["star"], got["short"], got["noqual"]) >= 10, got
    want, base = yardstick(seed, f=F, table=True, q=13, slack=3), yardstick(seed, f=F, q=13)
    assert want[1] == got["masked"], (want[1], got)
    assert 0.2 <= want[2] / want[3] <= 0.9, want[2:]
    assert want[0][:, 5].sum() != base[0][:, 5].sum() and want[0][:, 6].sum() != base[0][:, 6].sum()


def test_dense_tables_compile_to_the_segment_counts_the_device_tests_rely_on():
    for n, plus_only, want in ((256, False, 256), (257, False, 257), (300, False, 300)):
        rc, head, tail, msg = sch.compile_primers(fm.dense_table(n, plus_only), 0)
        assert rc == 0 and len(head) + len(tail) == want and len(head) == (n + 1) // 2, (n, msg)
    rc, head, tail, msg = sch.compile_primers(fm.dense_table(257, plus_only=True), 0)
    assert rc == 0 and (len(head), len(tail)) == (257, 0), msg


# ------------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    with engine.Context(0) as c:
        yield c


def check(ctx, path, specs, want, label, primers=(), q=0, f=NONE, slack=0):
    """test_primer_mask.check_file with a message a failure is analysed from: both packers equal the yardstick `want` (on `specs`, the
    records that pass f); the piled-up count and the extent are those of the same file without a table"""
    n_pos = len(want[0])
    for how in dvf.PACKERS:
        got, piled, end, n_prim, n_masked = dvf.through(ctx, how, path, primers, n_pos, q, f, slack)
        _, piled0, end0, n_prim0, n_masked0 = dvf.through(ctx, how, path, (), n_pos, q, f)
        msg = differ(got, want[0], specs, label + (how,))
        assert not msg, msg
        assert (piled, end, n_prim, n_masked, n_prim0, n_masked0) == (piled0, end0, len(primers), want[1], 0, 0), label + (how,)


def check_mode(ctx, path, seed, mode, key=None, window=None, q=None):
    tabled, slack, q0, f = MODES[mode]
    q = q0 if q is None else q
    specs, _ = passing(seed, key, window, f)
    want = yardstick(seed, key, window, f, tabled, q, slack)
    check(ctx, path, specs, want, (seed, mode, q), table_of(seed if key is None else key) if tabled else (), q, f, slack)
    return specs, want


def check_routing(ctx, path, seed, specs, want):
    """the combined mode: every piled-up read of more than 512 columns is left out of the packed set and walked by tally_stream_kernel,
    one launch in the general-tally bracket and one of the plane kernel per step (as test_primer_mask.test_long_reads asserts it)"""
    for how in dvf.PACKERS:
        try:
            ctx.set_option("one_sync", int(how == "one_sync"))
            ctx.set_read_filter(*F)
            ctx.set_min_base_quality(13)
            ctx.set_primers(table_of(seed), 3)
            d = engine.DeviceBam(path)
            try:
                rs = ctx.upload_bamfile(d)
                aligned, chunks, general = (C.c_int64(0) for _ in range(3))
                _ffi.check(_ffi.lib().tcmi_readset_sets(rs.handle, C.byref(aligned), C.byref(chunks), C.byref(general)))
                assert (rs.n_piled - aligned.value, general.value) == (n_long(specs), 0), (seed, how)
                ctx.profile(True)
                got = ctx.step(rs, len(want[0]), 0, True)[3]
                n_stream, n_planes = ctx.profile_get(_ffi.K_TALLY_GENERAL)[1], ctx.profile_get(_ffi.K_TALLY)[1]
                ctx.profile(False)
                msg = differ(got, want[0], specs, (seed, "all", "profiled", how))
                assert (n_stream, n_planes) == (1, 1) and not msg, (seed, how, n_stream, n_planes, msg)
                rs.free()
            finally:
                d.close()
        finally:
            ctx.profile(False)
            ctx.set_option("one_sync", 1)
            ctx.set_read_filter()
            ctx.set_min_base_quality()
            ctx.set_primers()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("seed", SEEDS)
def test_seeds_and_modes(ctx, tmp_path, seed, mode):
    path = write(tmp_path, fuzz(seed))
    specs, want = check_mode(ctx, path, seed, mode)
    if mode == "all":
        assert n_long(specs) >= 15
        check_routing(ctx, path, seed, specs, want)


@pytest.mark.gpu
def test_records_that_straddle_blocks(ctx, tmp_path):
    """512-byte blocks filled to the brim: the packers' reads of QUAL and of the CIGAR across block boundaries.  The long reads'
    records (1 - 2.3 KB) are larger than a block, so some blocks lie wholly inside one record: such a block holds no record start
    (test_bam_device.py constructs the case that the decoder's rec_vouch is for)."""
    path = write(tmp_path, fuzz(SEEDS[1]), block=512, split_records=True)
    check_mode(ctx, path, SEEDS[1], "all")


@pytest.mark.gpu
def test_long_records_that_straddle_blocks_larger_than_they_are(ctx, tmp_path):
    """the same records in 4 096-byte blocks filled to the brim: every long record straddles, none covers a whole block"""
    path = write(tmp_path, fuzz(SEEDS[1]), block=4096, split_records=True)
    check_mode(ctx, path, SEEDS[1], "all")


@pytest.mark.gpu
def test_short_records_that_straddle_small_blocks(ctx, tmp_path):
    """the seed without its long reads in 512-byte blocks filled to the brim: the packers' reads of QUAL and of the CIGAR across
    block boundaries, on random CIGARs"""
    seed, (_, slack, q, f) = SEEDS[1], MODES["all"]
    table = table_of(seed)
    kept = rsp.kept(fm.specs(seed, n_long=0, table=table), f)[0]
    assert n_long(kept) == 0 and profile(kept, table, slack)["masked"] >= 100
    path = write(tmp_path, fm.specs(seed, n_long=0, table=table), block=512, split_records=True)
    check(ctx, path, kept, py.counts(rsp.arrays(kept), L, table, q, slack), (seed, "all, short reads", q), table, q, f, slack)


@pytest.mark.gpu
@pytest.mark.parametrize("q", (1, 42, 255))
def test_other_floors(ctx, tmp_path, q):
    """under the table; at 255 only the reads without QUAL contribute"""
    seed = SEEDS[2]
    _, want = check_mode(ctx, write(tmp_path, fuzz(seed)), seed, "table", q=q)
    assert want[0][:, 0].any() and want[2] < yardstick(seed, table=True)[2]


@pytest.mark.gpu
def test_depth_with_irregular_drops(ctx, tmp_path):
    """every random read starts inside a window of 50 columns: the fourth bit-sliced counter of tally_planes_drop_kernel past eight
    bits, with a different drop word per read"""
    base = yardstick(DEEP_SEED, None, DEEP_WINDOW, F, False, 13)[0]
    want = yardstick(DEEP_SEED, None, DEEP_WINDOW, F, True, 13, 3)[0]
    assert base[:, 0].max() >= 256 and (want[:, 0] < base[:, 0]).sum() >= 100, (base[:, 0].max(), (want[:, 0] < base[:, 0]).sum())
    check_mode(ctx, write(tmp_path, fuzz(DEEP_SEED, None, DEEP_WINDOW)), DEEP_SEED, "all", window=DEEP_WINDOW)


@pytest.mark.gpu
@pytest.mark.parametrize("n,plus_only", ((256, False), (257, False), (300, False), (257, True)))
def test_tables_around_and_beyond_the_lds_stage(ctx, tmp_path, n, plus_only):
    """256 segments are the most a workgroup stages in LDS; from 257 on pk_planes_bq and place_body<true> search global memory"""
    seed, key = SEEDS[3], ("dense", n, plus_only)
    specs, _ = passing(seed, key)
    got = profile(specs, table_of(key), 0)
    assert got["masked"] >= 100 and got["long_masked"] >= 1, got
    path = write(tmp_path, fuzz(seed, key))
    for q in (0, 13):
        check_mode(ctx, path, seed, "table", key=key, q=q)


@pytest.mark.gpu
@pytest.mark.parametrize("split_sub", (1, 2))
def test_block_ranges_over_three_ranks(tmp_path, split_sub):
    """split_ranks_in_turn(world = 3) in the combined mode: the ranges in one piece, and as two sub-ranges each (that file holds every
    record four times: four times the yardstick).
    The 1 024-byte blocks of the sub-range file are smaller than the long reads' records: a range then holds blocks that lie wholly
    inside one record."""
    seed = SEEDS[0]
    _, orfs = sy.make_reference(seed=3, L=L, cds=[(100, 900), (1100, 1900)])
    specs, table = fuzz(seed), table_of(seed)
    kept, _ = passing(seed, f=F)
    want = yardstick(seed, f=F, table=True, q=13, slack=3)[0]
    n_pos = len(want)
    times = 1 if split_sub == 1 else 4
    big = specs if times == 1 else sorted([dict(r, name="%s_%d" % (r["name"], k)) for k in range(4) for r in specs], key=lambda r: r["pos"])
    path = write(tmp_path, big, block=1024 if split_sub == 2 else 4096)
    tm = {}
    kw = dict(return_parts=True, rules=engine.ReadRules(primers=(table, 3), min_baseq=13, read_filter=F))
    ta = distributed.split_ranks_in_turn(path, n_pos, cr.gff_rows(orfs), 10, 3, split_sub=split_sub, timings=tm, **kw)
    tb = distributed.split_ranks_in_turn(path, n_pos, cr.gff_rows(orfs), 10, 1, split_sub=1, **kw)
    msg = differ(ta[1], times * want, kept, (seed, "all", "three ranks", split_sub))
    assert not msg, msg
    msg = differ(ta[1], tb[1], kept, (seed, "all", "three ranks against one", split_sub))
    assert not msg and ta[0] == tb[0] and ta[2] == tb[2], msg
    assert (tm["split_sub_taken"] > 0) == (split_sub == 2)


def test_the_contig_inputs_are_not_vacuous():
    for name, ln, table, part in contig_case()[0]:
        got = profile(rsp.kept(part, F)[0], table, 0)
        assert got["long"] >= 3 and got["long_masked"] >= 1 and got["masked"] >= 30, (name, got)


@pytest.mark.gpu
def test_two_reference_contig_layout(ctx, tmp_path):
    """fuzzed reads on two references under a contig layout (shift_of in tally_stream_kernel and pk_mask_long), floor 13, each
    contig's own table, the read filter: every contig's slice equals the yardstick on that contig's passing reads under its rows"""
    parts, specs = contig_case()
    refs = [(name, ln) for name, ln, _ in CONTIGS]
    names = [n for n, _ in refs]
    path = str(tmp_path / "A.bam")
    bamwriter.write_bam(path, rsp.arrays(specs), refs=refs, block=4096)
    recs = [(name, sy.make_reference(seed=3, L=ln, cds=[])[0]) for name, ln in refs]
    shift, slot, axis = contigs.layout_for(recs, names, [ln for _, ln in refs])
    rows = pbed.rows_for_layout([(name, s, e, rev) for name, _, table, _ in parts for s, e, rev in table], names, shift)
    info = {}
    counts = contigs.step_contigs(ctx, path, shift, slot, axis, 10, True, names, want_counts=True, rules=engine.ReadRules(min_baseq=13, primers=(rows, 0), read_filter=F), info=info)[3]
    assert ctx.primers == 0
    seen = np.zeros(axis, bool)
    n_masked = 0
    for t, (name, ln, table, part) in enumerate(parts):
        kept = [dict(r, tid=0) for r in rsp.kept(part, F)[0]]
        assert n_long(kept) >= 3
        want = py.counts(rsp.arrays(kept), ln, table, 13)
        n_pos = len(want[0])
        n_masked += want[1]
        msg = differ(counts[int(shift[t]):int(shift[t]) + n_pos], want[0], kept, (name, "contig layout"))
        assert not msg, msg
        seen[int(shift[t]):int(shift[t]) + n_pos] = True
    assert not counts[~seen].any() and info["reads_primer_masked"] == n_masked
