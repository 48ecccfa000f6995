"""The amplicon table on the GPU (csrc/intervals.hip; tcmi_interval_stats_dev, tcmi_interval_stats, tcmi_ctx_set_intervals,
tcmi_step_intervals, tcmi_filerunner_run_files_stats, --amplicon-table): every comparison is exact equality of record arrays, or of the
table's text, with the yardstick (tests/amplicon_yardstick.py, plain Python integers).  The matrix, the interval arrays and the record
buffer lie between guards (tests/device_file.py) and are read back whole.  The scheme rule, the row writer and the argument
handling are checked without a GPU in tests/test_amplicon_scheme.py."""
import functools
import json
import os

import numpy as np
import pytest

from oracle import c_oracle
from tests import amplicon_yardstick as ay
from tests import cli_run as cr
from tests import device_file as dvf
from tests import primer_yardstick as py
from tests import read_specs as rsp
from tests import variant_yardstick as vy
from tests.schemes import write_scheme
from trueconsense_amd import TrueConsense as cli
from trueconsense_amd import _ffi, engine
from trueconsense_amd.io import bamwriter
from trueconsense_amd.io import primers as pb

pytestmark = pytest.mark.gpu
CAP = engine.INTERVAL_STAGE             # columns of an interval the kernel stages in LDS; a longer one is selected from memory
LENS = (0, 1, 2, 63, 64, 65, 255, 256, 257, CAP, CAP + 1, 2 * CAP + 1)
END = 1 << 29
TOP = (1 << 31) - 1


@pytest.fixture(scope="module")
def ctx():
    with engine.Context(0) as c:
        yield c


def test_the_capacity_is_the_headers():
    text = open(os.path.join(cr.ROOT, "include", "tcmi.h")).read()
    assert "#define TCMI_INTERVAL_STAGE %d\n" % CAP in text and CAP >= 512


def on_device(ctx, cov, intervals, min_depth, ld=None, off=0, rec_lead=0, seed=5):
    """tcmi_interval_stats_dev on a matrix between guards whose other planes and padding [L, ld) hold garbage (off: words past an 8-byte
    boundary), guarded interval arrays and a guarded record buffer (rec_lead: words past a 16-byte boundary) -> the records; the
    matrix and the intervals must be bit-identical afterwards, the guards around the records too"""
    L = len(cov)
    ld = L if ld is None else ld
    body = np.random.default_rng(seed).integers(-(1 << 31), 1 << 31, (7, ld), dtype=np.int64).astype(np.int32)
    body[0, :L] = cov
    m = dvf.Matrix(L, ld, off, body)
    n = len(intervals)
    iv = np.asarray(intervals, np.int64).reshape(-1, 2)
    st = dvf.Guarded(2 * n, np.int32, 0, np.ascontiguousarray(iv[:, 0]).view(np.int32))
    en = dvf.Guarded(2 * n, np.int32, 0, np.ascontiguousarray(iv[:, 1]).view(np.int32), salt=3)
    out = dvf.Guarded(8 * n, np.int32, rec_lead, salt=77)
    assert out.ptr % 16 == 4 * rec_lead
    ctx.interval_stats_dev(m.ptr, L, ld, n, st.ptr, en.ptr, min_depth, out.ptr)
    assert m.untouched(), "the matrix was written"
    assert st.untouched() and en.untouched(), "the intervals were written"
    return out.read().view(ay.DTYPE).copy()             # (read() checks both guards)


def rows_of(cov):
    """a coverage plane -> rows [L, 7] for the host entry point; the other columns hold something else"""
    c = np.full((len(cov), 7), 7, np.int32)
    c[:, 0] = cov
    return c


def check(ctx, cov, intervals, min_depth, geometry=((None, 0, 0),), host=True, what=()):
    want = ay.as_array(ay.records(cov, intervals, min_depth))
    L = len(cov)
    for ld, off, lead in geometry:
        got = on_device(ctx, cov, intervals, min_depth, ld, off, lead)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (what, L, ld, off, lead, min_depth, [(intervals[i], got[i].tolist(), want[i].tolist()) for i in bad[:4]])
    if host:
        assert np.array_equal(ctx.interval_stats(rows_of(cov), intervals, min_depth), want), (what, "tcmi_interval_stats")
    return want


def geometries(L):
    """ld = L on a matrix 4 bytes past an 8-byte boundary; an odd ld with the records off a 16-byte boundary; ld rounded up to 256"""
    up = (L + 255) // 256 * 256
    return ((L, 1, 0), (L + 1 + L % 2, 0, 1), (up, 1, 1), (up, 0, 0))


def depths(L, seed):
    """depths around a few levels with negatives, zeros and repeats: ties for the minimum and around the median"""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([-7, -1, 0, 0, 1, 2, 30, 30, 31, 1000, 1 << 20, TOP - 1], np.int64), L).astype(np.int32)


BIG = 2 * CAP + 1 + 70                  # a matrix just large enough for the longest interval at its off-boundary start


@pytest.mark.parametrize("L", (1, 255, 256, 257, 1000, BIG))
def test_lengths_starts_and_extents(ctx, L):
    """every length of LENS at starts on and off 64-column boundaries, in front of L, across it and wholly beyond it (depth 0,
    min_pos = start), intervals that end at 2^29; min_depth 0, 1 and one above every depth"""
    cov = depths(L, L)
    iv = []
    for n in LENS:
        for s in sorted({0, 64, 37, 69, max(L - 1, 0), L, L + 5, max(L - n // 2, 0), max(L - n, 0)}):
            iv.append((s, s + n))
    iv += [(0, END), (L // 2, END), (L, END), (END - 5, END), (END, END), (max(L - 1, 0), L), (0, L)]
    assert len(iv) <= 65536
    for md, geo in ((0, geometries(L)[:2]), (1, geometries(L)[2:]), (TOP, geometries(L)[1:2])):
        want = check(ctx, cov, iv, md, geo, host=md == 1, what="lengths")
        beyond = [k for k, (s, e) in enumerate(iv) if s >= L and e > s]
        assert beyond and all(want[k]["min_pos"] == iv[k][0] and want[k]["sum"] == 0 for k in beyond)
    if L == BIG:
        assert any(e <= L and e - s == 2 * CAP + 1 and s % 64 for s, e in iv)      # the longest one lies inside the matrix


def pattern_intervals(L):
    """short (staged in LDS) and long (selected from memory) intervals, even and odd n, starts on and off a boundary"""
    return [(0, 300), (5, 306), (64, 64 + 256), (1, 1 + 512), (0, CAP), (3, 3 + CAP + 1), (70, 70 + CAP + 300), (0, L), (1, L)]


@pytest.mark.parametrize("name", ("equal", "zero", "top", "top_byte", "bottom_byte", "negative", "last_lane", "twice"))
def test_depth_patterns(ctx, name):
    L = 2 * CAP + 500
    rng = np.random.default_rng(len(name))
    iv = pattern_intervals(L)
    if name == "equal":                 # median and minimum tie everywhere: the first position wins
        cov = np.full(L, 41, np.int64)
    elif name == "zero":
        cov = np.zeros(L, np.int64)
    elif name == "top":                 # 2^31 - 1 everywhere: the sums pass 2^32 (and 2^43 on the long ones)
        cov = np.full(L, TOP, np.int64)
    elif name == "top_byte":            # values that differ only in their top byte (the sign bit among them)
        cov = (rng.integers(0, 256, L) << 24) - (1 << 31) + 0x00ABCDEF
    elif name == "bottom_byte":
        cov = 0x12345600 + rng.integers(0, 256, L)
    elif name == "negative":
        cov = rng.integers(-(1 << 31), 0, L)
    elif name == "last_lane":           # the minimum in the last lane of the last wavefront: column 255 of a 256-column interval, the last column of others
        cov = rng.integers(10, 1000, L)
        cov[64 + 255] = 3
        cov[CAP - 1] = 2
        cov[L - 1] = 1
    else:                               # the minimum twice: its first position
        cov = rng.integers(10, 1000, L)
        for p in (100, 299, 310, CAP + 5, L - 2):
            cov[p] = 4
    cov = cov.astype(np.int32)
    for md in (0, 1, min(max(int(cov.max()) + 1, 0), TOP)):                         # the last: one above every depth, where int32 has one
        want = check(ctx, cov, iv, md, ((L, 0, 0), (L + 1, 1, 1)), host=md == 1, what=name)
    if name == "top":
        assert want[0]["sum"] == 300 * TOP > 1 << 32 and want[-2]["sum"] == L * TOP and want["median"].tolist() == [TOP] * len(iv)
    if name == "equal":
        assert want["min_pos"].tolist() == [s for s, _ in iv] and (want["median"] == 41).all() and (want["below"] == want["n"]).all()
    if name == "last_lane":
        assert (want[2]["min"], want[2]["min_pos"]) == (3, 64 + 255) and (want[4]["min"], want[4]["min_pos"]) == (2, CAP - 1)
        assert (want[-1]["min"], want[-1]["min_pos"]) == (1, L - 1)
    if name == "twice":
        assert (want[0]["min"], want[0]["min_pos"]) == (4, 100) and (want[1]["min_pos"], want[-1]["min_pos"]) == (100, 100)


@pytest.mark.parametrize("n", (1, 2, 255, 256, 257))
def test_interval_counts_and_their_order(ctx, n):
    """n intervals that are identical, nested, overlapping and in descending order"""
    L = 700
    cov = depths(L, 77 + n)
    rng = np.random.default_rng(n)
    iv = [(300, 420), (300, 420), (310, 400), (250, 350), (690, 720)][:n]                       # identical, nested, overlapping, across L
    while len(iv) < n:
        s = int(rng.integers(0, L + 20))
        iv.append((s, s + int(rng.integers(0, 400))))
    iv = iv[:5] + sorted(iv[5:], reverse=True)                                                  # descending starts
    want = check(ctx, cov, iv, 2, ((L, 0, 0), (L + 1, 1, 1)), what="counts")
    if n >= 2:
        assert want[0] == want[1]


def test_the_most_intervals_one_call_takes(ctx):
    L = 1000
    cov = depths(L, 4)
    iv = [(p % (L + 24), p % (L + 24) + 1) for p in range(65536)]
    want = check(ctx, cov, iv, 1, ((1024, 0, 0),), what="65536")
    assert want["n"].tolist() == [1] * 65536 and np.array_equal(want["median"][:L], cov) and np.array_equal(want["min"], want["median"])


def test_argument_errors(ctx):
    lib, h = _ffi.lib(), ctx.handle
    counts = rows_of(depths(64, 1))
    out = np.zeros(4, ay.DTYPE)
    good_s, good_e = np.array([0, 5, 9], np.int64), np.array([0, 9, END], np.int64)
    assert lib.tcmi_interval_stats(h, _ffi.ptr(counts), 64, 3, _ffi.ptr(good_s), _ffi.ptr(good_e), 0, _ffi.ptr(out)) == 0
    cases = [(np.array([0, -1, 9], np.int64), good_e, 0), (np.array([0, 10, 9], np.int64), good_e, 0), (good_s, np.array([0, 9, END + 1], np.int64), 0),
             (good_s, good_e, -1)]
    for s, e, md in cases:
        assert lib.tcmi_interval_stats(h, _ffi.ptr(counts), 64, 3, _ffi.ptr(s), _ffi.ptr(e), md, _ffi.ptr(out)) == _ffi.E_ARG
        assert lib.tcmi_ctx_set_intervals(h, 3, _ffi.ptr(s), _ffi.ptr(e), md) == _ffi.E_ARG
    for n in (-1, 65537):
        assert lib.tcmi_interval_stats(h, _ffi.ptr(counts), 64, n, _ffi.ptr(good_s), _ffi.ptr(good_e), 0, _ffi.ptr(out)) == _ffi.E_ARG
        assert lib.tcmi_ctx_set_intervals(h, n, _ffi.ptr(good_s), _ffi.ptr(good_e), 0) == _ffi.E_ARG
    assert lib.tcmi_interval_stats(h, _ffi.ptr(counts), -1, 3, _ffi.ptr(good_s), _ffi.ptr(good_e), 0, _ffi.ptr(out)) == _ffi.E_ARG
    assert lib.tcmi_interval_stats(h, _ffi.ptr(counts), 64, 3, None, _ffi.ptr(good_e), 0, _ffi.ptr(out)) == _ffi.E_ARG
    with pytest.raises(_ffi.TcmiError):                                             # none of them left a setting behind
        ctx.step_intervals()
    # the device entry point looks at the intervals it is given, and writes nothing when it refuses
    m = dvf.Matrix(64, 64, 0, np.ones((7, 64), np.int32))
    for s, e, _ in cases[:3]:
        st = dvf.Guarded(6, np.int32, 0, s.view(np.int32))
        en = dvf.Guarded(6, np.int32, 0, e.view(np.int32))
        rec = dvf.Guarded(24, np.int32, 0, salt=9)
        with pytest.raises(_ffi.TcmiError) as err:
            ctx.interval_stats_dev(m.ptr, 64, 64, 3, st.ptr, en.ptr, 0, rec.ptr)
        assert err.value.code == _ffi.E_ARG and rec.untouched() and m.untouched()
    with pytest.raises(_ffi.TcmiError):
        ctx.interval_stats_dev(m.ptr, 64, 63, 3, st.ptr, en.ptr, 0, rec.ptr)                  # ld < L
    ctx.interval_stats_dev(m.ptr, 64, 64, 0, 0, 0, 0, 0)                                        # n = 0: nothing to do


# ---- the step path --------------------------------------------------------------------------------------------------------------
L = rsp.L
PRIMERS = py.scheme()                   # '+' [s, s + 24), '-' [s + 376, s + 400), s = 30, 330, ...: 6 amplicons that overlap by 100 columns


def scheme_rows(chrom="ref", primers=PRIMERS):
    """the primer yardstick's scheme as BED rows named amp_K_LEFT / amp_K_RIGHT, pools 1 and 2 in turn, plus an alternate left primer
    of amplicon 2 that ends 6 columns further in"""
    rows = [(chrom, s, e, "amp_%d_%s" % (k // 2 + 1, "RIGHT" if rev else "LEFT"), str(1 + (k // 2) % 2), "-" if rev else "+") for k, (s, e, rev) in enumerate(primers)]
    s, e, _ = primers[2]
    return rows + [(chrom, s + 6, e + 6, "amp_2_LEFT_alt1", "2", "+")]


def amps_of(region="insert", rows=None):
    return ay.scheme(scheme_rows() if rows is None else rows, region)


@functools.lru_cache(maxsize=None)
def mixed_files():
    """-> (reads A, reads B = every second record of A) of read_specs.mixed()"""
    specs = rsp.mixed()[2]
    return rsp.arrays(specs), rsp.arrays(specs[::2])


@pytest.mark.parametrize("one_sync", (1, 0))
def test_step_path(ctx, tmp_path, one_sync):
    """set_intervals + tcmi_bamfile_step on both routes: the records are the yardstick's over the oracle's matrix, without and with
    --min-baseq 20 --primers, beside the variant setting, and none once the setting is cleared (no launch either)"""
    ra, rb = mixed_files()
    ref = rsp.mixed()[0]
    paths = [str(tmp_path / "A.bam"), str(tmp_path / "B.bam")]
    for p, rd in zip(paths, (ra, rb)):
        bamwriter.write_bam(p, rd, ref_len=L, block=4096)
    amps = amps_of()
    iv = [(a[3], a[4]) for a in amps] + [(1990, 2100), (5, 5)]                      # ... one across the reference's end, one empty
    assert len(amps) == 6 and amps[1][3] == PRIMERS[2][1] + 6                       # the alternate primer moved amplicon 2's insert
    plain = {k: c_oracle.tally(rd, c_oracle.extent(rd, L)) for k, rd in enumerate((ra, rb))}
    masked = {k: py.counts(rd, L, PRIMERS, 20)[0] for k, rd in enumerate((ra, rb))}
    try:
        ctx.set_option("one_sync", one_sync)
        with pytest.raises(_ffi.TcmiError):
            ctx.step_intervals()                                                    # no step has computed records yet
        ctx.set_intervals(iv, 30)
        for floor, mats in ((False, plain), (True, masked)):
            ctx.set_min_base_quality(20 if floor else 0)
            ctx.set_primers(*((PRIMERS, 0) if floor else ()))
            for want_counts in (False, True):
                for k in (0, 1, 0):
                    want = ay.as_array(ay.records(mats[k][:, 0], iv, 30))
                    d = engine.DeviceBam(paths[k])
                    before = (ctx.stat("one_sync_taken"), ctx.stat("one_sync_declined"))
                    rs, pl, al, fl, counts = ctx.bamfile_step(d, L, 30, True, want_counts=want_counts)
                    assert (ctx.stat("one_sync_taken"), ctx.stat("one_sync_declined")) == (before[0] + one_sync, before[1]), (one_sync, k)
                    got = ctx.step_intervals()
                    rs.free()
                    d.close()
                    assert np.array_equal(got, want), (one_sync, floor, want_counts, k, got.tolist(), want.tolist())
                    assert (counts is None) if not want_counts else np.array_equal(counts[:len(mats[k])], mats[k])
            assert want[6]["n"] == 110 and want[6]["below"] >= 100 and want[7].tolist() == ay.EMPTY
        assert not np.array_equal(ay.as_array(ay.records(plain[0][:, 0], iv, 30)), ay.as_array(ay.records(masked[0][:, 0], iv, 30)))
        ctx.set_min_base_quality(0)
        ctx.set_primers()
        # beside the variant table: both sets of records are those of the settings alone
        ctx.set_variants(ref, min_af="1/20", min_alt_depth=1, min_depth=1)
        d = engine.DeviceBam(paths[0])
        rs = ctx.bamfile_step(d, L, 30, True, want_counts=False)[0]
        rs.free()
        d.close()
        assert np.array_equal(ctx.step_intervals(), ay.as_array(ay.records(plain[0][:, 0], iv, 30)))
        assert np.array_equal(ctx.step_variants(), vy.as_array(vy.records(plain[0], ref.encode(), 1, 20, 1, 1))) and len(ctx.step_variants()) > 0
        ctx.set_variants(None)
        # the setting cleared: the next step launches nothing and has no records
        ctx.profile(True)
        launches = ctx.profile_get(_ffi.K_INTERVALS)[1]
        ctx.set_intervals(iv[:2], 5)
        rs = ctx.upload(ra)
        ctx.step(rs, len(plain[0]), 30, True, want_counts=False)                    # ... and through tcmi_step from flat arrays
        assert np.array_equal(ctx.step_intervals(), ay.as_array(ay.records(plain[0][:, 0], iv[:2], 5)))
        assert ctx.profile_get(_ffi.K_INTERVALS)[1] == launches + 1
        ctx.set_intervals(None)
        with pytest.raises(_ffi.TcmiError) as e:
            ctx.step_intervals()
        assert e.value.code == _ffi.E_ARG
        assert np.array_equal(ctx.step(rs, len(plain[0]), 30, True)[3], plain[0])
        assert ctx.profile_get(_ffi.K_INTERVALS)[1] == launches + 1
        with pytest.raises(_ffi.TcmiError):
            ctx.step_intervals()
        rs.free()
    finally:
        ctx.profile(False)
        ctx.set_option("one_sync", 1)
        ctx.set_intervals(None)
        ctx.set_variants(None)
        ctx.set_min_base_quality(0)
        ctx.set_primers()


def test_array_pipeline_refuses(ctx):
    ra, _ = mixed_files()
    n_pos = c_oracle.extent(ra, L)
    p = engine.Pipeline(device=0, slots=2, walkers=1)
    try:
        rs = p.ctx.upload(ra)
        for k in range(2):
            p.slot_context(k).set_intervals([(0, 10)], 1)
        with pytest.raises(_ffi.TcmiError) as e:
            p.run([rs], n_pos, 10, True)
        assert e.value.code == _ffi.E_UNSUPPORTED and "--amplicon-table" in str(e.value)
        for k in range(2):
            p.slot_context(k).set_intervals(None)
        assert np.array_equal(p.ctx.step(rs, n_pos, 0, True)[3], c_oracle.tally(ra, n_pos))    # usable afterwards
        rs.free()
    finally:
        p.close()


def test_file_runner_records_and_the_host_reader_fallback(tmp_path):
    ra, rb = mixed_files()
    ref = rsp.mixed()[0]
    paths = []
    for tag, rd in (("A", ra), ("B", rb), ("C", ra)):
        paths.append(str(tmp_path / (tag + ".bam")))
        bamwriter.write_bam(paths[-1], rd, ref_len=L, block=4096)
    iv = [(a[3], a[4]) for a in amps_of("full")] + [(1990, 2100)]
    want = [ay.records(c_oracle.tally(rd, c_oracle.extent(rd, L))[:, 0], iv, 30) for rd in (ra, rb, ra)]
    for device_decode in (True, False):                                             # False: every sample through the host reader
        runner = engine.FileRunner(0, [], 30, gpu_streams=2, intervals=(iv, 30))
        runner.device_decode = device_decode
        runner.set_outputs("ref", ref, "##vcf\n", "##gff\n", [])
        fasta = [str(tmp_path / ("%d%d.fa" % (k, device_decode))) for k in range(3)]
        got = runner.run_files(paths, ["S"] * 3, fasta, ref_len=L, stats=True)
        assert runner.decoded_on == ({"device": 3, "host": 0} if device_decode else {"device": 0, "host": 3})
        assert got.shape == (3, len(iv)) and all(np.array_equal(got[k], ay.as_array(want[k])) for k in range(3))
        assert runner.run_files(paths[:1], ["S"], fasta[:1], ref_len=L) is None     # without stats: as before
        runner.close()
    bare = engine.FileRunner(0, [], 30, gpu_streams=1)
    with pytest.raises(ValueError):
        bare.run_files(paths[:1], ["S"], [str(tmp_path / "x.fa")], ref_len=L, stats=True)
    out = np.zeros(2, ay.DTYPE)                                                     # the ABI itself: records without the setting are refused
    rc = _ffi.lib().tcmi_filerunner_run_files_stats(bare.handle, 0, None, None, (_ffi.C.c_char_p * 1)(), None, None, None, None, L, 30, 1, 1,
                                                    None, None, None, None, 2, _ffi.ptr(out))
    assert rc == _ffi.E_ARG
    bare.close()


# ---- command line ---------------------------------------------------------------------------------------------------------------


def table_text(counts, amps, sample="S", region="ref", min_depth=30, header=True):
    recs = ay.records(counts[:, 0], [(a[3], a[4]) for a in amps], min_depth)
    return (ay.HEADER if header else "") + ay.text(recs, sample, region, [a[1] for a in amps], [a[2] for a in amps], [a[3] for a in amps])


def test_cli_single_sample_and_batch(tmp_path, monkeypatch):
    """-i with --amplicon-table: the table is the yardstick's over the oracle's matrix, the four other outputs are those of the run
    without the flag; --amplicon-region unique; with --min-baseq 20 --primers (the scheme defaults to that file) it follows the masked
    matrix, with --index-override the overridden one; --batch writes one file with every sample's rows in manifest order"""
    monkeypatch.chdir(tmp_path)
    ref, orfs, specs = rsp.mixed()
    rd, rd3 = mixed_files()
    bamwriter.write_bam("A.bam", rd, ref_len=L, block=4096)
    bamwriter.write_bam("A2.bam", rd, ref_len=L, block=4096, split_records=True)
    bamwriter.write_bam("A3.bam", rd3, ref_len=L, block=4096)
    common = cr.setup_cli(ref, orfs)
    write_scheme("s.bed", scheme_rows() + [("elsewhere", 5, 25, "x_LEFT", "1", "+"), ("elsewhere", 300, 320, "x_RIGHT", "1", "-")])
    counts, counts3 = (c_oracle.tally(r, c_oracle.extent(r, L)) for r in (rd, rd3))
    cov = int(common[common.index("-cov") + 1])
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + cr.out_args("a") + ["--amplicon-table", "a.amp", "--amplicon-scheme", "s.bed", "--stats", "a.json"])
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + cr.out_args("b") + ["--stats", "b.json"])
    want = table_text(counts, amps_of(), min_depth=cov)
    assert open("a.amp").read() == want and want.count("\n") == 7 and "elsewhere" not in want
    assert cr.outputs("a") == cr.outputs("b") and not os.path.exists("b.amp")
    below = sum(1 for ln in want.split("\n")[1:] if ln and ln.split("\t")[-1] != "0")
    sa, sb = json.load(open("a.json")), json.load(open("b.json"))
    assert (sa["amplicons"], sa["amplicons_below"], sb["amplicons"], sb["amplicons_below"]) == (6, below, 0, 0)
    for region in ("unique", "full"):
        cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + cr.out_args("u") + ["--amplicon-table", "u.amp", "--amplicon-scheme", "s.bed",
                                                                          "--amplicon-region", region])
        got = open("u.amp").read()
        assert got == table_text(counts, amps_of(region), min_depth=cov) != want
        assert cr.outputs("u") == cr.outputs("b"), region
    # the floor and the primer mask: the table follows the masked matrix; the scheme is the file of --primers
    masked = py.counts(rd, L, [(s, e, st == "-") for _, s, e, _, _, st in scheme_rows()], 20)[0]
    write_scheme("p.bed", scheme_rows())
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + ["-o", "q.fa", "--amplicon-table", "q.amp", "--min-baseq", "20", "--primers", "p.bed"])
    assert open("q.amp").read() == table_text(masked, amps_of(), min_depth=cov) != want
    # --index-override: the table is taken behind the override
    over = counts.copy()
    over[700:760] = (3, 3, 0, 0, 0, 0, 0)
    cr.write_override("o.csv.gz", over)
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + cr.out_args("o") + ["--amplicon-table", "o.amp", "--amplicon-scheme", "s.bed", "--index-override", "o.csv.gz"])
    cr.run_cli(monkeypatch, ["-i", "A.bam", "-name", "S"] + common + cr.out_args("o2") + ["--index-override", "o.csv.gz"])
    assert open("o.amp").read() == table_text(over, amps_of(), min_depth=cov) != want
    assert cr.outputs("o") == cr.outputs("o2") != cr.outputs("b")
    # --batch: three samples, one file, manifest order
    for name, tail in (("m", ["--amplicon-table", "m.amp", "--amplicon-scheme", "s.bed", "--stats", "m.json"]), ("n", [])):
        with open(name + ".tsv", "w") as fh:
            for k, bam in enumerate(("A.bam", "A2.bam", "A3.bam")):
                fh.write("\t".join([bam, "S%d" % k] + ["%s%d.%s" % (name, k, e) for e in ("fa", "vcf", "gff", "tsv")]) + "\n")
        cr.run_cli(monkeypatch, ["--batch", name + ".tsv"] + common + tail)
    assert open("m.amp").read() == ay.HEADER + "".join(table_text(c, amps_of(), "S%d" % k, min_depth=cov, header=False) for k, c in enumerate((counts, counts, counts3)))
    for k in range(3):
        assert cr.outputs("m%d" % k) == cr.outputs("n%d" % k), k
    assert not os.path.exists("n.amp") and json.load(open("m.json"))["amplicons"] == 6


def test_cli_per_contig(tmp_path, monkeypatch):
    """--per-contig on a two-contig file: one table, REGION the contig, positions the contig's own; rows on a chrom the layout does
    not hold are ignored, a scheme that leaves nothing is an argument error"""
    monkeypatch.chdir(tmp_path)
    recs, rows, specs = rsp.two_contigs()
    refs = [("c0", 1500), ("c1", 1200)]
    bamwriter.write_bam("A.bam", rsp.arrays(specs), refs=refs, block=4096)
    cr.setup_contigs(recs, rows)
    bed = scheme_rows("c1", py.scheme(n=3)) + scheme_rows("c0", py.scheme(first=100, n=4))[:-1] + [("c9", 5, 25, "x_LEFT", "1", "+"), ("c9", 300, 320, "x_RIGHT", "1", "-")]
    bed = [r[:3] + (r[0] + r[3],) + r[4:] for r in bed]                             # (keys are per scheme: the contig's name in front)
    write_scheme("s.bed", bed)
    args = ["-i", "A.bam", "-ref", "r.fa", "-gff", "g.gff", "-cov", "10", "-name", "S", "--per-contig"]
    cr.run_cli(monkeypatch, args + ["-o", "a.fa", "-doc", "a.tsv", "--amplicon-table", "a.amp", "--amplicon-scheme", "s.bed", "--stats", "a.json"])
    cr.run_cli(monkeypatch, args + ["-o", "b.fa", "-doc", "b.tsv"])
    amps = ay.scheme(bed)
    want = ay.HEADER
    for name, ln in (refs[1], refs[0]):                                             # chroms in the order of the scheme's file
        t = [n for n, _ in refs].index(name)
        rd = rsp.arrays([dict(r, tid=0) for r in specs if r["tid"] == t])
        part = table_text(c_oracle.tally(rd, c_oracle.extent(rd, ln)), [a for a in amps if a[0] == name], region=name, min_depth=10, header=False)
        assert part.count("\n") >= 3
        want += part
    got = open("a.amp").read()
    assert got == want and "c9" not in got
    assert open("a.fa").read() == open("b.fa").read() and open("a.tsv").read() == open("b.tsv").read()
    st = json.load(open("a.json"))
    assert st["amplicons"] == 7 and st["amplicons_below"] == sum(1 for ln in got.split("\n")[1:] if ln and ln.split("\t")[-1] != "0")
    write_scheme("none.bed", bed[-2:])
    with pytest.raises(SystemExit) as e:
        cr.run_cli(monkeypatch, args + ["-o", "c.fa", "--amplicon-table", "c.amp", "--amplicon-scheme", "none.bed"])
    assert e.value.code == 1 and not os.path.exists("c.amp") and not os.path.exists("c.fa")


def test_cli_split_worker_at_world_one(tmp_path, monkeypatch):
    """`-i --gpus N`'s worker (trueconsense_amd.split_main) as one rank: rank 0 takes the table from the reduced counts; the other
    four outputs are those of the worker without the flag"""
    monkeypatch.chdir(tmp_path)
    ref, orfs, specs = rsp.mixed()
    rd = mixed_files()[0]
    bamwriter.write_bam("A.bam", rd, ref_len=L, block=4096, split_records=True)
    common = cr.setup_cli(ref, orfs)
    write_scheme("s.bed", scheme_rows())
    worker = ["-i", "A.bam", "-name", "S"] + common
    for args in (worker + cr.out_args("w") + ["--amplicon-table", "w.amp", "--amplicon-scheme", "s.bed", "--amplicon-region", "unique", "--gpus", "1"],
                 worker + cr.out_args("x") + ["--gpus", "1"]):
        cr.run_split_worker(args)
    assert cr.outputs("w") == cr.outputs("x") and not os.path.exists("x.amp")
    cov = int(common[common.index("-cov") + 1])
    assert open("w.amp").read() == table_text(c_oracle.tally(rd, c_oracle.extent(rd, L)), amps_of("unique"), min_depth=cov)
    assert cli.amplicon_intervals([(pb.Amplicon(*a), 0) for a in amps_of("unique")])[0] == (54, 330)
