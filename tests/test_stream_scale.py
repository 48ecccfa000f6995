"""The record-stream counting kernels (csrc/stream_count.h: amplicon_reads_kernel, strand_counts_kernel, link_counts_kernel), pk_mask_long
and the floor / mask / filter variants of the packers on more records than their capped grids take in one trip.  Every comparison is
exact equality.

CAP = compute units * SC_WG_PER_CU * SC_BLOCK (read from csrc/stream_count.h) is what one trip of each_record covers; pk_mask_long's
cap is its 64 workgroups of PB = 256 lanes (pinned in tests/test_repeat_bam.py).
  A  a fuzz file of tests/test_floor_mask_fuzz.py with every record R times in place (tests/repeat_bam.py), R odd with R * records just
     above CAP and a record that counts in the ragged second trip, more than 1 024 BGZF blocks.  Every count is R times the committed
     yardstick of the small file (the additivity is pinned without a GPU in tests/test_repeat_bam.py).  Seeds 1 and 2, seed 1 once
     more with its blocks filled to the brim, and the deep file (every read starts in 50 columns): its deepest column times R passes
     65 535 in every mode (seeds 1 and 2 reach 120 * 305 = 36 600).
  B  the long reads of seed 1 alone, R' times: more than 64 * 256 of them for pk_mask_long; and those of them that have a mask.
  C  fixed 20M reads with per-base qualities, MAPQ and strands (tests/fixed_reads.py) at CAP, CAP + 1 and 2 CAP + 256 + 65 records: a
     trip that ends on the bound, a second with one live lane, three with a full and a ragged workgroup in the last; the yardstick is
     tests/fixed_reads' numpy restatement (pinned to the committed yardsticks in tests/test_repeat_bam.py).  The one-sync packer builds
     these (the files A overflow its event array — that many indels, N and insertions R times over — and fall to the several-kernel
     packer, which the route assertion admits for that one reason only).
The files are written once per module and every read set answers all of its queries from one upload; the tests of a case then look at
different parts of what was measured."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import amplicon_reads_cases as arc
from tests import amplicon_reads_yardstick as ry
from tests import device_file as dvf
from tests import fixed_reads as fx
from tests import fuzz_masked as fm
from tests import link_cases as lkc
from tests import links_yardstick as ly
from tests import primer_yardstick as py
from tests import read_specs as rsp
from tests import repeat_bam as rb
from tests import schemes as sch
from tests import strand_cases as stc
from trueconsense_amd import _ffi, engine

pytestmark = pytest.mark.gpu
L = fm.L
SC_BLOCK, SC_WG_PER_CU = rb.stream_count_caps()
MASK_LONG_CAP = rb.MASK_LONG_GRID * rb.MASK_LONG_BLOCK
KEYS = {"seed1": (1, None, False), "seed2": (2, None, False), "deep": (fm.DEEP_SEED, fm.DEEP_WINDOW, False), "seed1_brim": (1, None, True)}
A_CASES = [(key, mode) for key in ("seed1", "seed2", "deep") for mode in sorted(fm.MODES)] + [("seed1_brim", "all")]
LINK_KS = (1, 7)
AMP_SLACKS = (0, 5)
FULL = arc.tiled(7, primer=190)                                                  # primer zones 20 columns apart: reads do run from one into the other
# mode -> (floor, read filter, primer table, slack)
C_MODES = {"plain": (0, fm.NONE, (), 0), "floor": (13, fm.NONE, (), 0), "floor_mapq": (13, fx.MQ, (), 0), "all": (13, fx.MQ, tuple(sch.PRIMER_SCHEME), 3)}
C_SIZES = ("cap", "cap_plus_1", "three_trips")


@pytest.fixture(scope="module")
def ctx():
    with engine.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def cap(ctx):
    """the records one trip of each_record covers on this device"""
    n = ctx.stat("compute_units") * SC_WG_PER_CU * SC_BLOCK
    assert n > 0
    return n


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    """the module's directory and everything written or measured once: {key: value}"""
    return {"dir": tmp_path_factory.mktemp("scale")}


def once(store, key, make):
    if key not in store:
        store[key] = make()
    return store[key]


def figures(rs):
    return dict(n_reads=rs.n_reads, n_piled=rs.n_piled, filtered=rs.filtered, masked=rs.primer_masked_reads, max_end=rs.max_end)


def counts_under_every_mode(r):
    return fm._piles_up(r) and rsp.passes(r, fm.F)


def tail_from(cap, n, r):
    """the first of n records whose r copies reach beyond the first `cap` records of the repeated file"""
    return cap // r


def times_for(cap, specs):
    """the smallest odd R with R * records > cap (wavefronts then straddle different records) and no multiple of 64 records, for which a
    record that counts under every mode lies in the second trip: an unmapped or filtered tail would leave that trip nothing to count"""
    n = len(specs)
    r = cap // n + 1
    r += r % 2 == 0
    while (r * n) % 64 == 0 or not any(counts_under_every_mode(x) for x in specs[tail_from(cap, n, r):]):
        r += 2
    return r


# ====================================================================================================================== files A
@functools.lru_cache(maxsize=None)
def plan_a(seed, window, mode):
    """what the small file gives on the yardsticks and which queries the repeated file is asked, every case non-vacuous as
    test_strand_counts, test_link_counts and test_amplicon_reads ask it of the yardstick — before any device runs"""
    tabled, slack, q, f = fm.MODES[mode]
    every = fm.fuzz(seed, None, window)
    specs, _ = fm.passing(seed, None, window, f)
    want = fm.yardstick(seed, None, window, f, tabled, q, slack)
    fwd, rev, n_pos = stc.halves(seed, mode, window)
    assert n_pos == len(want[0]) and np.array_equal(fwd + rev, want[0])
    if window is None:
        strand_sparse, link_sparse = stc.sparse_columns(seed, n_pos), lkc.sparse_columns(seed, n_pos, 5, 3)
    else:                                                                       # (the columns the two modules query on the deep file)
        strand_sparse = sorted(set(range(window[0] - 20, window[1] + 60, 3)) | set(stc.sparse_columns(seed, n_pos, 20)))[:stc.LDS]
        link_sparse = list(range(window[0] - 10, window[1] + 50, 5))[:11]
    dense = list(range(n_pos))
    assert len(strand_sparse) <= stc.LDS < len(dense)
    for cols in (strand_sparse, dense):
        stc.not_vacuous(specs, fwd[cols], rev[cols], cols, (seed, mode))
    cls, n_pos2, whole = lkc.classes_of(seed, mode, window)
    assert n_pos2 == n_pos and np.array_equal(whole, want[0])
    link_cases = [(cols, k, ly.joint(cls, cols, k)) for cols in (link_sparse, lkc.window_columns(whole)) for k in LINK_KS]
    for cols, k, j in link_cases:
        lkc.not_vacuous(j, (seed, mode, len(cols), k))
    assert lkc.long_read_over(specs, link_cases[-1][0]) and lkc.long_read_over(specs, link_sparse, 2), (seed, mode)
    assert [len(cols) * k <= lkc.LDS for cols, k, _ in link_cases] == [True, True, False, False]
    rd = rsp.arrays(every)
    columns = ry.kept_columns(rd, None, f, rd["mapq"])
    assert len(columns) == sum(fm._piles_up(r) for r in specs)
    amp_cases = []
    for amps in (arc.tiled(7), arc.padded(arc.tiled(7), arc.LDS + 1), FULL):
        for s in AMP_SLACKS:
            w = ry.counts(columns, amps, s)
            assert w[:, 0].sum() == len(columns) and (w[:, 1] <= w[:, 0]).all() and w[len(amps):, 0].all(), (seed, mode, w[:9].tolist())
            assert w[:7, 0].all() if window is None else (w[:7, 0] > 0).sum() >= 3, (seed, mode, w[:9].tolist())      # (the deep file's reads start in 50 columns)
            assert amps is not FULL or window is not None or (w[:7, 1] > 0).sum() >= 5, (seed, mode, "full-length reads", w[:7].tolist())
            amp_cases.append((amps, s, w))
    assert [len(a) <= arc.LDS for a, _, _ in amp_cases] == [True, True, False, False, True, True]
    return dict(specs=specs, want=want, n_pos=n_pos, fwd=fwd, rev=rev, strand={"LDS": strand_sparse, "memory": dense}, links=link_cases, amps=amp_cases,
                n_small=len(every), n_piled=len(columns), deepest=int(want[0][:, 0].max()))


def tail_links_of(cap, r, seed, window, mode, n_pos):
    """one more link query, on the records of the second trip: up to eleven columns of the first record there that counts under every
    mode and has tokens on them under this one (a primer can mask a record whole) -> [(columns, k, the small file's joint counts)]"""
    every = fm.fuzz(seed, None, window)
    cls = lkc.classes_of(seed, mode, window)[0]
    for x in every[tail_from(cap, len(every), r):]:
        if not counts_under_every_mode(x):
            continue
        cols = sorted(x["pos"] + d for d in (0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89) if d < fm._span(x) and x["pos"] + d < n_pos)
        cases = [(cols, k, ly.joint(cls, cols, k)) for k in LINK_KS]
        if len(cols) >= 2 and all(j.any() for _, _, j in cases):
            assert len(cols) * max(LINK_KS) <= lkc.LDS
            return cases
    raise AssertionError("no record of the second trip has tokens to count: %r" % ((seed, mode, r),))


def file_a(store, cap, key):
    """-> (the small file, the repeated one, R, its records, its BGZF blocks)"""
    def make():
        seed, window, brim = KEYS[key]
        d = store["dir"] / key
        d.mkdir()
        specs = fm.fuzz(seed, None, window)
        src = fm.write(d, specs)
        r = times_for(cap, specs)
        dst = str(d / "R.bam")
        n = rb.repeat_records(src, dst, r, brim=brim)
        return src, dst, r, n, rb.n_blocks(dst)
    return once(store, ("file", key), make)


def measured_a(ctx, store, cap, key, mode, how):
    """the repeated file of `key` under `mode` on the packer `how`: one upload, the step's matrix and every query of plan_a"""
    def make():
        seed, window, _ = KEYS[key]
        p = plan_a(seed, window, mode)
        tabled, slack, q, f = fm.MODES[mode]
        table = fm.table_of(seed) if tabled else ()
        src, dst, r, n, n_blocks = file_a(store, cap, key)
        tail_links = tail_links_of(cap, r, seed, window, mode, p["n_pos"])
        # two trips of each_record, the second ragged; the single-workgroup scans over the blocks go past one chunk of 1 024
        assert n == r * p["n_small"] and r % 2 == 1
        assert n > cap and n % 64 != 0 and n - cap < cap, (n, cap)
        assert n_blocks > 1024, n_blocks
        if window is not None:                                                  # the deep file: a column of the matrix passes 16 bits
            assert p["deepest"] * r > 65535, (p["deepest"], r)
        with dvf.uploaded(ctx, src, table, q, f, slack, how=how) as rs:
            small = figures(rs)
        assert small["n_reads"] == p["n_small"] and small["n_piled"] == p["n_piled"] and small["masked"] == p["want"][1]
        out = dict(r=r, small=small, tail_links=tail_links)
        with dvf.uploaded(ctx, dst, table, q, f, slack, how=how, events_may_overflow=True) as rs:
            out["big"], out["route"] = figures(rs), rs.route
            assert rs.n_reads == n > cap and rs.n_reads % 64 != 0 and rs.n_reads - cap < cap
            out["matrix"] = ctx.step(rs, p["n_pos"], 0, True)[3]
            out["strand"] = {route: stc.device_counts(ctx, rs, cols) for route, cols in p["strand"].items()}
            out["links"] = [lkc.device_links(ctx, rs, cols, k) for cols, k, _ in p["links"] + tail_links]
            out["amps"] = [arc.device_counts(ctx, rs, amps, s) for amps, s, _ in p["amps"]]
        return out
    return once(store, ("A", key, mode, how), make)


def case_a(ctx, store, cap, key, mode, how):
    seed, window, _ = KEYS[key]
    m = measured_a(ctx, store, cap, key, mode, how)
    return plan_a(seed, window, mode), m, (key, mode, how, "built by " + m["route"])


@pytest.mark.parametrize("how", dvf.PACKERS)
@pytest.mark.parametrize("key,mode", A_CASES)
def test_a_the_matrix_and_the_read_sets_figures_are_r_times_the_small_files(ctx, store, cap, key, mode, how):
    """pk_place_bq / pk_planes_bq / tally_planes_drop_kernel and tally_stream_kernel's by_token branch behind more than 1 024 blocks"""
    p, m, label = case_a(ctx, store, cap, key, mode, how)
    r, small, big = m["r"], m["small"], m["big"]
    msg = fm.differ(m["matrix"], r * p["want"][0], p["specs"], label)
    assert not msg, msg
    assert (big["n_piled"], big["filtered"], big["masked"]) == (r * small["n_piled"], r * small["filtered"], r * small["masked"]), (label, big, small)
    assert big["max_end"] == small["max_end"] and big["masked"] == r * p["want"][1]
    if fm.MODES[mode][3] != fm.NONE:
        assert small["filtered"] > 0
    if fm.MODES[mode][0]:
        assert small["masked"] > 0


@pytest.mark.parametrize("how", dvf.PACKERS)
@pytest.mark.parametrize("key,mode", A_CASES)
def test_a_strand_counts(ctx, store, cap, key, mode, how):
    p, m, label = case_a(ctx, store, cap, key, mode, how)
    for route, cols in p["strand"].items():
        got = m["strand"][route]
        msg = stc.differ(got, (m["r"] * p["fwd"][cols], m["r"] * p["rev"][cols]), cols, label + (route,))
        assert not msg, msg
        assert np.array_equal(got[0] + got[1], m["matrix"][cols]), label + (route, "the invariant")


@pytest.mark.parametrize("how", dvf.PACKERS)
@pytest.mark.parametrize("key,mode", A_CASES)
def test_a_link_counts(ctx, store, cap, key, mode, how):
    p, m, label = case_a(ctx, store, cap, key, mode, how)
    assert len(m["links"]) == len(p["links"]) + len(m["tail_links"])
    for (cols, k, want), got in zip(p["links"] + m["tail_links"], m["links"]):
        msg = lkc.differ(got, m["r"] * want, label + (len(cols), k))
        assert not msg, msg
        assert not ly.invariant(got, k, m["matrix"]), label + (len(cols), k, ly.invariant(got, k, m["matrix"]))


@pytest.mark.parametrize("how", dvf.PACKERS)
@pytest.mark.parametrize("key,mode", A_CASES)
def test_a_amplicon_reads(ctx, store, cap, key, mode, how):
    p, m, label = case_a(ctx, store, cap, key, mode, how)
    for (amps, s, want), got in zip(p["amps"], m["amps"]):
        assert got[:, 0].sum() == m["big"]["n_piled"], label + (len(amps), s, "the invariant")
        assert np.array_equal(got, m["r"] * want), label + (len(amps), s, got[:9].tolist(), (m["r"] * want)[:9].tolist())


# ====================================================================================================================== file B
@functools.lru_cache(maxsize=None)
def plan_b(slack):
    seed = 1
    every = fm.fuzz(seed)
    index = [i for i, r in enumerate(every) if fm._piles_up(r) and fm._span(r) > fm.LONG]
    specs = [every[i] for i in index]
    table = fm.table_of(seed)
    want = py.counts(rsp.arrays(specs), L, table, 0, slack)
    n_masked = fm.profile(specs, table, slack)["long_masked"]
    assert len(specs) == fm.n_long(every) >= 15 and n_masked == want[1] >= 5, (len(specs), n_masked, want[1])
    return dict(index=index, specs=specs, table=table, want=want, n_masked=n_masked)


def file_b(store, masked_only=False):
    """the long reads R' times; masked_only: those of them with a mask at slack 0 (and so at slack 3) alone"""
    def make():
        p = plan_b(0)
        index = [i for i, x in zip(p["index"], p["specs"]) if not masked_only or long_is_masked(x, p["table"], 0)]
        src = fm.write(store["dir"], fm.fuzz(1))
        r = MASK_LONG_CAP // len(index) + 2
        dst = str(store["dir"] / ("B%d.bam" % masked_only))
        return dst, r, rb.repeat_records(src, dst, r, keep=index), index
    return once(store, ("file", "B", masked_only), make)


def long_is_masked(x, table, slack):
    return fm.profile([x], table, slack)["long_masked"] == 1


@pytest.mark.parametrize("how", dvf.PACKERS)
@pytest.mark.parametrize("slack", (0, 3))
def test_b_pk_mask_long_past_one_trip_of_its_grid(ctx, store, slack, how):
    """more long reads than pk_mask_long's 64 x 256 lanes under the seed's table: the masked reads it counts for tcmi_readset_primers
    are R' times those of the 37 records, every one of them is left to tally_stream_kernel, and the matrix is R' times the yardstick"""
    p = plan_b(slack)
    path, r, n, _ = file_b(store)
    assert n == r * len(p["specs"]) > MASK_LONG_CAP and n - MASK_LONG_CAP < rb.MASK_LONG_BLOCK and (n - MASK_LONG_CAP) % 64 != 0, (n, r)
    with dvf.uploaded(ctx, path, p["table"], 0, fm.NONE, slack, how=how) as rs:
        aligned, chunks, general = (C.c_int64(0) for _ in range(3))
        _ffi.check(_ffi.lib().tcmi_readset_sets(rs.handle, C.byref(aligned), C.byref(chunks), C.byref(general)))
        assert rs.n_reads == rs.n_piled == n and (rs.n_piled - aligned.value, general.value) == (n, 0), (how, aligned.value, general.value)
        try:
            ctx.profile(True)
            got = ctx.step(rs, len(p["want"][0]), 0, True)[3]
            n_stream = ctx.profile_get(_ffi.K_TALLY_GENERAL)[1]
        finally:
            ctx.profile(False)
        assert n_stream == 1, (how, n_stream)
        assert rs.primer_masked_reads == r * p["n_masked"], (how, slack, rs.primer_masked_reads, r, p["n_masked"])
        msg = fm.differ(got, r * p["want"][0], p["specs"], ("long reads", slack, how))
        assert not msg, msg


@pytest.mark.parametrize("how", dvf.PACKERS)
@pytest.mark.parametrize("slack", (0, 3))
def test_b_every_long_read_masked_whatever_order_the_packer_lists_them_in(ctx, store, slack, how):
    """the packers list the long reads in the order their lanes get to it, so which of file B's reads a second trip of pk_mask_long
    holds is not the test's to choose: here every read has a mask, and the count is the number of records"""
    p = plan_b(slack)
    path, r, n, index = file_b(store, masked_only=True)
    specs = [x for i, x in zip(p["index"], p["specs"]) if i in index]
    assert 5 <= len(specs) == p["n_masked"] or slack, (len(specs), p["n_masked"])
    assert all(long_is_masked(x, p["table"], slack) for x in specs) and n == r * len(specs) > MASK_LONG_CAP
    with dvf.uploaded(ctx, path, p["table"], 0, fm.NONE, slack, how=how) as rs:
        assert rs.n_reads == rs.n_piled == rs.primer_masked_reads == n, (how, slack, rs.n_piled, rs.primer_masked_reads, n)
        want = py.counts(rsp.arrays(specs), L, p["table"], 0, slack)[0]
        msg = fm.differ(ctx.step(rs, len(want), 0, True)[3], r * want, specs, ("masked long reads", slack, how))
        assert not msg, msg


# ====================================================================================================================== files C
def size_c(cap, which):
    return {"cap": cap, "cap_plus_1": cap + 1, "three_trips": 2 * cap + SC_BLOCK + 65}[which]


C_STRAND = sorted(int(c) for c in np.random.default_rng(41).choice(fx.L, 200, replace=False))
C_LINKS = [700, 701, 705, 719, 720, 740, 1500, 1501, 1519, 2379, 2399]         # neighbours a read of 20 reaches both of, and ones it cannot
C_WINDOW = list(range(1000, 1300))


def file_c(store, cap, which):
    def make():
        rd = fx.generate(size_c(cap, which), 100 + C_SIZES.index(which))
        rd["mapq"][-1] = 60                                                     # (the one live lane of cap + 1's second trip holds a record that passes the filter)
        return rd, fx.write(store["dir"] / ("C_%s.bam" % which), rd)
    return once(store, ("file", "C", which), make)


def measured_c(ctx, store, cap, which, mode):
    def make():
        q, f, table, slack = C_MODES[mode]
        rd, path = file_c(store, cap, which)
        n = len(rd["pos"])
        assert which != "three_trips" or rb.n_blocks(path) > 1024               # (the one-sync packer's scans over the blocks go past one chunk too)
        assert n == size_c(cap, which) and len(C_STRAND) <= stc.LDS < fx.L and len(C_LINKS) * max(LINK_KS) <= lkc.LDS < len(C_WINDOW)
        want = dict(matrix=fx.matrix(rd, fx.L, q, f, table, slack), strand={"LDS": C_STRAND, "memory": list(range(fx.L))},
                    links=[(cols, k, fx.links(rd, cols, k, q, f, table, slack)) for cols in (C_LINKS, C_WINDOW) for k in LINK_KS],
                    masked=fx.masked_reads(rd, f, table, slack),
                    amps=[(amps, s, fx.amplicon_reads(rd, amps, s, f)) for amps in (fx.SCHEME, arc.padded(fx.SCHEME, arc.LDS + 1)) for s in AMP_SLACKS],
                    kept=int(fx.kept(rd, f).sum()))
        for _, k, j in want["links"]:
            lkc.not_vacuous(j, (which, mode, k))
        for amps, s, w in want["amps"]:
            assert w[:8, 0].all() and w[7, 1] > 0 and w[len(amps):, 0].all() and w[:, 0].sum() == want["kept"]
        assert want["matrix"][:, 1:5].sum(0).all() and (f == fm.NONE) == (want["kept"] == n) and (want["masked"] > 1000) == bool(table)
        got = {}
        with dvf.uploaded(ctx, path, table, q, f, slack, how="one_sync") as rs:
            got["figures"] = figures(rs)
            assert rs.n_reads == n
            got["matrix"] = ctx.step(rs, fx.L, 0, True)[3]
            got["strand"] = {route: stc.device_counts(ctx, rs, cols) for route, cols in want["strand"].items()}
            got["links"] = [lkc.device_links(ctx, rs, cols, k) for cols, k, _ in want["links"]]
            got["amps"] = [arc.device_counts(ctx, rs, amps, s) for amps, s, _ in want["amps"]]
        return rd, want, got
    return once(store, ("C", which, mode), make)


@pytest.mark.parametrize("mode", sorted(C_MODES))
@pytest.mark.parametrize("which", C_SIZES)
def test_c_the_matrix_and_the_strand_counts_at_the_bounds_of_each_record(ctx, store, cap, which, mode):
    rd, want, got = measured_c(ctx, store, cap, which, mode)
    q, f, table, slack = C_MODES[mode]
    bad = np.unique(np.argwhere(got["matrix"] != want["matrix"])[:, 0])[:6].tolist()
    assert not bad, (which, mode, [(c, got["matrix"][c].tolist(), want["matrix"][c].tolist()) for c in bad])
    assert (got["figures"]["n_piled"], got["figures"]["filtered"], got["figures"]["masked"]) == (want["kept"], len(rd["pos"]) - want["kept"], want["masked"])
    for route, cols in want["strand"].items():
        msg = stc.differ(got["strand"][route], fx.strand(rd, cols, q, f, table, slack), cols, (which, mode, route))
        assert not msg, msg
        assert np.array_equal(got["strand"][route][0] + got["strand"][route][1], got["matrix"][cols]), (which, mode, route, "the invariant")


@pytest.mark.parametrize("mode", sorted(C_MODES))
@pytest.mark.parametrize("which", C_SIZES)
def test_c_link_counts_at_the_bounds_of_each_record(ctx, store, cap, which, mode):
    _, want, got = measured_c(ctx, store, cap, which, mode)
    for (cols, k, j), g in zip(want["links"], got["links"]):
        msg = lkc.differ(g, j, (which, mode, len(cols), k))
        assert not msg, msg
        assert not ly.invariant(g, k, got["matrix"]), (which, mode, len(cols), k, ly.invariant(g, k, got["matrix"]))


@pytest.mark.parametrize("mode", sorted(C_MODES))
@pytest.mark.parametrize("which", C_SIZES)
def test_c_amplicon_reads_at_the_bounds_of_each_record(ctx, store, cap, which, mode):
    _, want, got = measured_c(ctx, store, cap, which, mode)
    for (amps, s, w), g in zip(want["amps"], got["amps"]):
        assert g[:, 0].sum() == got["figures"]["n_piled"], (which, mode, len(amps), s, "the invariant")
        assert np.array_equal(g, w), (which, mode, len(amps), s, g[:10].tolist(), w[:10].tolist())
