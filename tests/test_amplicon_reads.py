"""--amplicon-reads on the GPU (csrc/amplicon_reads.hip; tcmi_readset_amplicon_reads, Context.amplicon_reads): every comparison is
exact equality with the yardstick (tests/amplicon_reads_yardstick.py: per record a loop over all amplicons) applied to the SAME BAM
parsed on the host (engine.BamFile).  The host record buffer lies between guards (tests/device_file.py's sentinel words) and the
invariant — the reads add up to the kept records — is checked on every call.  Every case runs through both staging routes: the scheme
as it is (table and counters in LDS) and padded with far-away amplicons to TCMI_AMPLICON_READS_LDS + 1 (table and counters in
memory).  The rule, the scheme and the argument handling are checked without a GPU in tests/test_amplicon_reads_rule.py."""
import contextlib
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from tests import amplicon_reads_yardstick as ry
from tests import cli_run as cr
from tests import fuzz_reads as fz
from tests import read_specs as rsp
from tests import schemes as sch
from tests import synth_small as ss
from tests.amplicon_reads_cases import LDS, device_counts, host_columns, padded, scheme_rows_for, tiled, want_text
from trueconsense_amd import _ffi, contigs, engine
from trueconsense_amd import distributed as td
from trueconsense_amd.io import bamwriter

pytestmark = pytest.mark.gpu
L = 2400


@pytest.fixture(scope="module")
def ctx():
    with engine.Context(0) as c:
        yield c


@contextlib.contextmanager
def packer(ctx, one_sync):
    """1: the one-sync packer (the default) builds the read set; 0: the several-kernel packer"""
    ctx.set_option("one_sync", one_sync)
    try:
        yield
    finally:
        ctx.set_option("one_sync", 1)


def specs_for(seed, n, length=L, unmapped=0.02):
    """n reads of 40 - 380 reference columns with assorted CIGARs (every op), sorted by position, MAPQ and FLAG bits to filter by"""
    rng = np.random.default_rng(seed)
    ref = ss._rand_seq(rng, length)
    specs = []
    for k in range(n):
        ln = int(rng.integers(40, 380))
        pos = int(rng.integers(0, length - ln - 30))
        a = int(rng.integers(5, ln - 10))
        cig = ([(ln, "M")], [(3, "H"), (4, "S"), (ln, "M"), (2, "S"), (1, "H")], [(a, "M"), (3, "I"), (ln - a, "M")], [(a, "M"), (7, "D"), (ln - a, "M")],
               [(a, "="), (20, "N"), (ln - a, "X")], [(a, "M"), (2, "P"), (1, "I"), (ln - a, "M")], [(ln, "M")], [(2, "S"), (ln, "M")])[int(rng.integers(0, 8))]
        flag = (16 if rng.random() < 0.5 else 0) | (4 if rng.random() < unmapped else 0) | (0x400 if rng.random() < 0.2 else 0)
        r = fz._read(rng, ref, pos, cig, flag, "r%d" % k)
        r["mapq"] = int(rng.choice((0, 19, 20, 60)))
        specs.append(r)
    specs.sort(key=lambda r: r["pos"])
    return specs


def write(path, specs, **kw):
    kw.setdefault("block", 4096)
    kw.setdefault("ref_len", L)
    bamwriter.write_bam(str(path), rsp.arrays(specs), **kw)
    return str(path)


def check(ctx, rs, columns, amps4, slack, what=(), routes=True):
    """the read set's counts == the yardstick's over `columns`, on the scheme as it is and — the other staging route — padded"""
    want = ry.counts(columns, amps4, slack)
    n = len(amps4)
    assert want[:, 0].sum() == len(columns) and (want[:, 1] <= want[:, 0]).all() and not want[n:, 1].any()
    assert not routes or n <= LDS
    for use in [list(amps4)] + ([padded(amps4, LDS + 1)] if routes else []):
        got = device_counts(ctx, rs, use, slack)
        m = len(use)
        assert got[:, 0].sum() == len(columns), (what, m, "the invariant")
        assert np.array_equal(got[:n], want[:n]) and np.array_equal(got[m:], want[n:]) and not got[n:m].any(), (
            what, m, got[:n][got[:n] != want[:n]][:8].tolist(), got[m:].tolist(), want[n:].tolist())
    return want


@functools.lru_cache(maxsize=None)
def big_specs():
    return specs_for(11, 3000)


@pytest.mark.parametrize("one_sync", (1, 0))
@pytest.mark.parametrize("n_rec", (1, 63, 64, 65, 256, 257, 3000))
def test_record_counts_on_both_packers(ctx, tmp_path, n_rec, one_sync):
    specs = big_specs()[::3000 // n_rec][:n_rec] if n_rec < 3000 else big_specs()
    path = write(tmp_path / "A.bam", specs)
    cols = host_columns(path)
    with packer(ctx, one_sync):
        rs = ctx.upload_bamfile(engine.DeviceBam(path))
    try:
        assert rs.n_reads == n_rec and len(cols) == rs.n_piled
        for slack in (0, 5):
            want = check(ctx, rs, cols, tiled(7), slack, (n_rec, one_sync, slack))
        if n_rec == 3000:
            assert (want[:7, 0] > 20).all() and (want[:7, 1] > 0).any() and want[7, 0] > 20 and want[8, 0] > 50     # every class is there
    finally:
        rs.free()


def scheme_of(n):
    """n amplicons on the axis: up to seven tiled ones that hold reads, spread among decoys every four columns that are too short
    (36 columns with slack 3; the shortest read has 40) to hold any — they sit between the real ones in the sorted table, so the
    search, the prefix's largest end and the second largest all have to be right"""
    real = tiled(min(n, 7))
    decoys = [(4 * k + 1, 4 * k + 3, 4 * k + 20, 4 * k + 31) for k in range(n - len(real))]
    every = max(1, len(decoys) // len(real))
    out = []
    for k, a in enumerate(real):
        out += decoys[k * every:(k + 1) * every if k + 1 < len(real) else len(decoys)] + [a]
    return out, [i for i, a in enumerate(out) if a in real]


@pytest.mark.parametrize("n", (1, 2, LDS, LDS + 1))
def test_table_sizes(ctx, tmp_path, n):
    """n = 1, 2, the largest table staged in LDS and the smallest searched in memory, on the same reads"""
    path = write(tmp_path / "A.bam", big_specs())
    cols = host_columns(path)
    amps, real = scheme_of(n)
    assert len(amps) == n and len(real) == min(n, 7)
    rs = ctx.upload_bamfile(engine.DeviceBam(path))
    try:
        want = check(ctx, rs, cols, amps, 3, ("table", n), routes=n <= 2)
        assert (want[real, 0] > 100).all() and want[:n, 0].sum() == want[real, 0].sum() and want[n + 1, 0] > 0
        if n > 2:                                           # the decoys change nothing: the seven real amplicons count what they count alone
            alone = ry.counts(cols, tiled(7), 3)
            assert np.array_equal(want[real], alone[:7]) and np.array_equal(want[n:], alone[7:])
    finally:
        rs.free()


def test_a_wavefront_in_one_amplicon_and_one_in_64(ctx, tmp_path):
    """records 0..63 (one wavefront) all lie in amplicon 0; records 64..127 lie in 64 different amplicons"""
    rng = np.random.default_rng(3)
    ref = ss._rand_seq(rng, 6000)
    amps = [(100, 110, 290, 300)] + [(400 + 80 * k, 405 + 80 * k, 465 + 80 * k, 470 + 80 * k) for k in range(64)]
    specs = [fz._read(rng, ref, 100 + k, [(120, "M")], 0, "a%d" % k) for k in range(64)]
    specs[5] = fz._read(rng, ref, 105, [(195, "M")], 0, "full")                           # ... one of them full length: p < 110, q = 299 >= 290
    specs += [fz._read(rng, ref, 402 + 80 * k, [(66, "M")], 16, "b%d" % k) for k in range(64)]
    for r in specs:
        r["mapq"] = 60
    path = write(tmp_path / "A.bam", specs, ref_len=6000)
    cols = host_columns(path)
    rs = ctx.upload_bamfile(engine.DeviceBam(path))
    try:
        want = check(ctx, rs, cols, amps, 0, "wavefronts")
        assert want[0].tolist() == [64, 1] and want[1:65].tolist() == [[1, 1]] * 64 and want[65:].tolist() == [[0, 0], [0, 0]]
    finally:
        rs.free()


def edge_specs():
    """every CIGAR op, leading and trailing S / H, D at an edge, N, no CIGAR at all, reads that touch an amplicon's widened extent
    [a, b) = [95, 305) exactly, unmapped records in the middle and at the end"""
    rng = np.random.default_rng(9)
    ref = ss._rand_seq(rng, L)
    rows = [(94, [(100, "M")], 0),                                                       # p == a - 1: outside
            (95, [(100, "M")], 0), (95, [(210, "M")], 16),                                 # p == a exactly; q == b - 1 exactly: full length
            (96, [(210, "M")], 0),                                                       # q == b: outside
            (100, [(5, "H"), (6, "S"), (50, "M"), (4, "S"), (2, "H")], 0), (100, [(3, "D"), (50, "M")], 0), (100, [(50, "M"), (155, "D")], 0),   # q = 304 by a trailing D
            (100, [(50, "M"), (156, "D")], 0),                                           # ... and 305: outside
            (101, [(20, "="), (100, "N"), (30, "X"), (2, "P"), (3, "I"), (40, "M")], 16),
            (102, [], 0),                                                                # n_cigar = 0: no span, not kept
            (102, [(30, "S")], 0), (103, [(12, "I")], 0),                                # no reference span either
            (104, [(60, "M")], 4),                                                       # unmapped with a position
            (120, [(185, "M")], 0), (130, [(10, "M"), (165, "N")], 0)]                  # q = 304: inside; N reaches 304
    specs = []
    for k, (pos, cig, flag) in enumerate(rows):
        r = fz._read(rng, ref, pos, cig, flag, "e%d" % k, seq=None if cig else "ACGT")
        if not cig:
            r["cigar"] = ""
        r["mapq"] = 60
        specs.append(r)
    for k in range(3):                                                                   # unmapped, unplaced: tid -1, pos -1, at the end of the file
        r = fz._read(rng, ref, 0, [], 4, "u%d" % k, tid=-1, seq="ACGTAC")
        r.update(pos=-1, cigar="", mapq=0)
        specs.append(r)
    return specs


@pytest.mark.parametrize("one_sync", (1, 0))
def test_cigar_ops_and_exact_edges(ctx, tmp_path, one_sync):
    specs = edge_specs()
    path = write(tmp_path / "A.bam", specs)
    cols = host_columns(path)
    assert cols == [(94, 193), (95, 194), (95, 304), (96, 305), (100, 149), (100, 152), (100, 304), (100, 305), (101, 290), (120, 304), (130, 304)]
    with packer(ctx, one_sync):
        rs = ctx.upload_bamfile(engine.DeviceBam(path))
    try:
        assert rs.n_reads == len(specs) and rs.n_piled == len(cols)
        want = check(ctx, rs, cols, [(100, 125, 280, 300)], 5, ("edges", one_sync))
        assert want.tolist() == [[8, 4], [0, 0], [3, 0]]
        check(ctx, rs, cols, [(100, 125, 280, 300), (100, 125, 280, 300)], 5, ("twins", one_sync))          # identical amplicons: all ambiguous
        check(ctx, rs, cols, [(0, 10, 20, 30)], 1000, ("slack 1000", one_sync))                            # a = -1000: no clamp at 0
    finally:
        rs.free()


@pytest.mark.parametrize("one_sync", (1, 0))
def test_the_read_sets_own_filter(ctx, tmp_path, one_sync):
    """records failing --min-mapq / --exclude-flags are not counted, and the counts follow the filter the read set was BUILT under
    after the context's filter has changed"""
    path = write(tmp_path / "A.bam", big_specs()[:1200])
    f = (20, 0, 0x400)
    cols, everything = host_columns(path, read_filter=f), host_columns(path)
    assert 0.3 < len(cols) / len(everything) < 0.7
    try:
        ctx.set_read_filter(*f)
        with packer(ctx, one_sync):
            rs = ctx.upload_bamfile(engine.DeviceBam(path))
        assert rs.filtered > 0 and rs.n_piled == len(cols)
        ctx.set_read_filter()                               # the context moves on; the read set remembers
        check(ctx, rs, cols, tiled(7), 5, ("filter", one_sync))
        rs.free()
        # ... and the other way round: built under no filter, counted while the context has one
        with packer(ctx, one_sync):
            rs = ctx.upload_bamfile(engine.DeviceBam(path))
        ctx.set_read_filter(*f)
        check(ctx, rs, everything, tiled(7), 5, ("no filter", one_sync), routes=False)
        rs.free()
    finally:
        ctx.set_read_filter()


def test_two_contigs_under_a_layout(ctx, tmp_path):
    """amplicons shifted by their contig's slot; reads on a reference without a slot are not kept; another layout: refused"""
    rng = np.random.default_rng(21)
    recs, _, specs = rsp.two_contigs()
    extra = [fz._read(rng, recs[0][1], 20 * k, [(50, "M")], 0, "x%d" % k, 2) for k in range(30)]           # a reference the layout gives no slot
    for r in extra:
        r["mapq"] = 60
    refs = [("c0", 1500), ("c1", 1200), ("X", 900)]
    path = write(tmp_path / "A.bam", specs + extra, refs=refs, ref_len=0)
    shift, slot, axis = contigs.layout_for(recs, [n for n, _ in refs], [ln for _, ln in refs])
    assert shift[2] == -1 and shift[1] > 1500
    cols = host_columns(path, shift=shift)
    own = tiled(4, 20, 300, 400)
    amps = [tuple(v + int(shift[t]) for v in a) for t in (0, 1) for a in own]
    try:
        ctx.set_layout(shift, slot)
        rs = ctx.upload_bamfile(engine.DeviceBam(path))
        assert rs.dropped() == 30 and rs.n_piled == len(cols)
        want = check(ctx, rs, cols, amps, 5, "layout")
        assert (want[:8, 0] > 10).all() and not np.array_equal(want[:4], want[4:8])
        ctx.set_layout()                                    # cleared: the device table stays, the read set still answers
        check(ctx, rs, cols, amps, 5, "layout cleared", routes=False)
        ctx.set_layout(shift, slot)                         # set once more: the device table was rewritten
        with pytest.raises(_ffi.TcmiError) as e:
            ctx.amplicon_reads(rs, amps, 5)
        assert e.value.code == _ffi.E_UNSUPPORTED and "layout" in str(e.value)
        rs.free()
    finally:
        ctx.set_layout()


@pytest.mark.parametrize("one_sync", (1, 0))
def test_long_reads_count_once(ctx, tmp_path, one_sync):
    """reads longer than the packed set takes (512 columns): they are tallied from the stream, and counted from it, once each"""
    rng = np.random.default_rng(5)
    ref = ss._rand_seq(rng, 6000)
    specs = []
    for k in range(90):
        ln = int(rng.integers(600, 1900)) if k % 3 else int(rng.integers(50, 300))
        a = ln // 2
        cig = [(ln, "M")] if k % 2 else [(a, "M"), (40, "D"), (ln - a, "M")]
        r = fz._read(rng, ref, int(rng.integers(0, 6000 - ln - 60)), cig, 0, "l%d" % k)
        r["mapq"] = 60
        specs.append(r)
    specs.sort(key=lambda r: r["pos"])
    path = write(tmp_path / "A.bam", specs, ref_len=6000)
    cols = host_columns(path)
    assert sum(1 for p, q in cols if q - p + 1 > 512) == 60
    with packer(ctx, one_sync):
        rs = ctx.upload_bamfile(engine.DeviceBam(path))
    try:
        assert rs.n_piled == 90
        want = check(ctx, rs, cols, tiled(3, 100, 1800, 2000, 200), 5, ("long", one_sync))
        assert want[:3, 0].sum() > 30
    finally:
        rs.free()


def test_straddled_blocks_and_block_ranges(ctx, tmp_path):
    """records that straddle BGZF blocks; the block ranges of a file, taken in turn on one context, add up to the whole file"""
    path = write(tmp_path / "A.bam", big_specs(), split_records=True, block=3000)
    cols = host_columns(path)
    amps = tiled(7)
    d = engine.DeviceBam(path)
    assert d.n_blocks > 60
    rs = ctx.upload_bamfile(d)
    whole = check(ctx, rs, cols, amps, 5, "straddled")
    rs.free()
    for world in (2, 5):
        total = np.zeros_like(whole)
        n_reads = 0
        for rank in range(world):
            rs = ctx.upload_bamfile(d, td.block_range(d.n_blocks, rank, world))
            total += device_counts(ctx, rs, amps, 5)
            n_reads += rs.n_reads
            rs.free()
        assert n_reads == 3000 and np.array_equal(total, whole), world
    d.close()


def test_sub_ranges_answer_with_the_sum_of_their_parts(tmp_path):
    """tcmi_split_step with two sub-ranges: the read set is the sum of its parts, each counted on its own context"""
    import torch
    path = write(tmp_path / "A.bam", big_specs(), split_records=True, block=3000)
    cols = host_columns(path)
    c = engine.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    d = engine.DeviceBam(path)
    try:
        c.set_option("split_sub", 2)
        ld, n_words = td.split_words(L, 1)
        t = torch.zeros(n_words, dtype=torch.int32, device="cuda")
        hook = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)(lambda user, p, n, stream: 0)
        rc, rs, _ = td._split_step(c, d, 0, 1, L, ld, t, 10, True, hook, None)
        assert rc == 0 and c.stat("split_sub_taken") == 1
        check(c, rs, cols, tiled(7), 5, "sub-ranges")
        rs.free()
    finally:
        d.close()
        c.close()


def test_refusals(ctx, tmp_path):
    """after another upload on the context the stream is gone: TCMI_E_UNSUPPORTED, in words; a read set from flat arrays has none; the
    scheme's argument errors; nothing is written when the call refuses"""
    pa, pb_ = write(tmp_path / "A.bam", big_specs()[:300]), write(tmp_path / "B.bam", big_specs()[300:500])
    amps = tiled(7)
    ra = ctx.upload_bamfile(engine.DeviceBam(pa))
    assert ctx.amplicon_reads(ra, amps, 5)["reads"].sum() == ra.n_piled
    rb = ctx.upload_bamfile(engine.DeviceBam(pb_))
    with pytest.raises(_ffi.TcmiError) as e:
        ctx.amplicon_reads(ra, amps, 5)
    assert e.value.code == _ffi.E_UNSUPPORTED and "no longer resident" in str(e.value)
    assert ctx.amplicon_reads(rb, amps, 5)["reads"].sum() == rb.n_piled                   # the newer one answers
    for bad, slack, word in (([], 0, "1..65536"), ([(10, 5, 80, 100)], 0, "fs < le"), (amps, 1001, "slack"), ([(0, 5, 8, (1 << 29) + 1)], 0, "2^29")):
        with pytest.raises(_ffi.TcmiError) as e:
            ctx.amplicon_reads(rb, bad, slack)
        assert e.value.code == _ffi.E_ARG and word in str(e.value), bad
    ra.free()
    rb.free()
    bam = engine.BamFile(pa)
    flat = ctx.upload(bam)                                  # flat arrays: packed, but no record stream
    with pytest.raises(_ffi.TcmiError) as e:
        ctx.amplicon_reads(flat, amps, 5)
    assert e.value.code == _ffi.E_UNSUPPORTED and "not decoded on the device" in str(e.value)
    flat.free()
    bam.close()
    path = write(tmp_path / "U.bam", [dict(r, flag=r["flag"] | 4) for r in big_specs()[:40]])    # a file of unmapped records only: all zero
    ru = ctx.upload_bamfile(engine.DeviceBam(path))
    assert ru.n_piled == 0 and not device_counts(ctx, ru, amps, 5).any()
    ru.free()


def test_the_launch_is_profiled_and_nothing_runs_without_the_call(ctx, tmp_path):
    path = write(tmp_path / "A.bam", big_specs()[:500])
    try:
        ctx.profile(True)
        rs = ctx.upload_bamfile(engine.DeviceBam(path))
        ctx.step(rs, L, 10, True)
        assert ctx.profile_get(_ffi.K_AMPLICON_READS)[1] == 0
        ctx.amplicon_reads(rs, tiled(7), 5)
        ctx.amplicon_reads(rs, padded(tiled(7), LDS + 1), 5)
        ms, n = ctx.profile_get(_ffi.K_AMPLICON_READS)
        assert n == 2 and ms > 0
        rs.free()
    finally:
        ctx.profile(False)


# ---- command line ---------------------------------------------------------------------------------------------------------------


def test_cli_single_sample(tmp_path, monkeypatch):
    """-i with --amplicon-reads: the file is the writer's text over the yardstick's counts; FASTA, VCF, GFF, TSV and --amplicon-table
    are byte-identical with and without the flag; the read filter is followed; --stats has the two counts"""
    monkeypatch.chdir(tmp_path)
    ref, orfs, specs = rsp.mixed()
    bamwriter.write_bam("A.bam", rsp.arrays(specs), ref_len=rsp.L, block=4096)
    common = cr.setup_cli(ref, orfs)
    amps = tiled(6, 30, 300, 400)
    sch.write_scheme("s.bed", scheme_rows_for("ref", amps) + scheme_rows_for("elsewhere", amps[:1]))
    table = ["--amplicon-table", "a.amp", "--amplicon-scheme", "s.bed"]
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + cr.out_args("a") + table + ["--amplicon-reads", "a.reads", "--stats", "a.json"])
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + cr.out_args("b") + ["--amplicon-table", "b.amp", "--amplicon-scheme", "s.bed", "--stats", "b.json"])
    cols = host_columns("A.bam")
    want = want_text("S", cols, [("ref", amps)], 5)
    assert open("a.reads").read() == want and want.count("\n") == 9 and "elsewhere" not in want
    assert cr.outputs("a") == cr.outputs("b") and open("a.amp").read() == open("b.amp").read() and not os.path.exists("b.reads")
    sa, sb = json.load(open("a.json")), json.load(open("b.json"))
    cnt = ry.counts(cols, amps, 5)
    assert (sa["amplicon_reads_ambiguous"], sa["amplicon_reads_unassigned"]) == (int(cnt[6, 0]), int(cnt[7, 0])) and cnt[6, 0] > 0 and cnt[7, 0] > 0
    assert (sb["amplicon_reads_ambiguous"], sb["amplicon_reads_unassigned"]) == (0, 0)
    # slack 0 under a read filter, the scheme from --primers' file... which also masks: the counts do not change with the mask
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + ["-o", "c.fa", "--amplicon-reads", "c.reads", "--amplicon-reads-slack", "0", "--primers", "s.bed"] + rsp.FLAGS)
    want0 = want_text("S", host_columns("A.bam", read_filter=rsp.FILTERS["all"]), [("ref", amps)], 0)
    assert open("c.reads").read() == want0 != want


def test_cli_per_contig(tmp_path, monkeypatch):
    """--per-contig on a two-contig file: one file, REGION per contig, amplicons shifted by their slots; the other outputs unchanged"""
    monkeypatch.chdir(tmp_path)
    recs, rows, specs = rsp.two_contigs()
    refs = [("c0", 1500), ("c1", 1200)]
    bamwriter.write_bam("A.bam", rsp.arrays(specs), refs=refs, block=4096)
    cr.setup_contigs(recs, rows)
    own = {"c1": tiled(3, 40, 300, 420), "c0": tiled(4, 20, 300, 400)}
    sch.write_scheme("s.bed", scheme_rows_for("c1", own["c1"]) + scheme_rows_for("c0", own["c0"]) + scheme_rows_for("c9", own["c0"][:1]))
    args = ["-i", "A.bam", "-ref", "r.fa", "-gff", "g.gff", "-cov", "10", "-name", "S", "--per-contig"]
    cr.run_cli(monkeypatch, args + ["-o", "a.fa", "-doc", "a.tsv", "--amplicon-reads", "a.reads", "--amplicon-scheme", "s.bed", "--stats", "a.json"])
    cr.run_cli(monkeypatch, args + ["-o", "b.fa", "-doc", "b.tsv"])
    shift, slot, axis = contigs.layout_for(recs, [n for n, _ in refs], [ln for _, ln in refs])
    at_ = {"c0": int(shift[0]), "c1": int(shift[1])}
    cols = host_columns("A.bam", shift=shift)
    chrom_amps = [(c, [tuple(v + at_[c] for v in a) for a in own[c]]) for c in ("c1", "c0")]      # chroms in the order of the scheme's file
    want = want_text("S", cols, chrom_amps, 5)
    got = open("a.reads").read()
    assert got == want and "c9" not in got and got.count("\n") == 10
    assert open("a.fa").read() == open("b.fa").read() and open("a.tsv").read() == open("b.tsv").read()
    st = json.load(open("a.json"))
    cnt = ry.counts(cols, [a for _, amps in chrom_amps for a in amps], 5)
    assert (st["amplicon_reads_ambiguous"], st["amplicon_reads_unassigned"]) == (int(cnt[7, 0]), int(cnt[8, 0]))


def test_cli_one_file_over_two_gpus(tmp_path, monkeypatch):
    """--gpus 2 (two ranks rehearsed on this one GPU, gloo for the exchange): every rank counts its own records, rank 0 writes the sum;
    the other outputs are those of the run without the flag"""
    monkeypatch.chdir(tmp_path)
    ref, orfs, specs = rsp.mixed()
    bamwriter.write_bam("A.bam", rsp.arrays(specs), ref_len=rsp.L, block=4096, split_records=True)
    common = cr.setup_cli(ref, orfs)
    amps = tiled(6, 30, 300, 400)
    sch.write_scheme("s.bed", scheme_rows_for("ref", amps))
    for tag, extra in (("a", ["--amplicon-reads", "a.reads", "--amplicon-scheme", "s.bed", "--amplicon-reads-slack", "3", "--gpus", "2"]), ("b", ["--gpus", "2"])):
        cr.run_two_ranks(["-i", "A.bam", "-name", "S"] + common + cr.out_args(tag) + extra)
    assert open("a.reads").read() == want_text("S", host_columns("A.bam"), [("ref", amps)], 3)
    assert cr.outputs("a") == cr.outputs("b") and not os.path.exists("b.reads")
