"""GPU: the one-sync file path (tcmi_readset_from_bamfile_blocks, tcmi_bamfile_step) on valid files BEYOND each capacity it sizes its
device arrays for before it has seen the file (tests/capacity_files.py; tests/test_capacity_files.py keeps the files beyond them):
the retry sized for the worst case, the declines to the several-kernel path with their flags, the event re-pack of
tcmi_pack_on_device from files and from flat arrays, a context's state after a declined step, block ranges, and the same files under
a base-quality floor and a read filter.  Integer work: counts and call records equal the oracle's bit for bit (c_oracle.tally /
c_oracle.call; under a floor the pileup oracle of tests/read_specs.oracle_counts), and the read sets' figures equal those of the
several-kernel path.  What the reference computes here is indexing.BuildIndex (indexing.py:75-154) and the position-local part of
BuildConsensus (Sequences.py:119-165)."""
import contextlib

import numpy as np
import pytest

from oracle import c_oracle
from tests import capacity_files as cf
from tests import read_specs as rsp
from tests import synth_small as ss
from trueconsense_amd import distributed as td
from trueconsense_amd import engine
from trueconsense_amd import synthetic as sy
from trueconsense_amd.io import bamwriter

pytestmark = pytest.mark.gpu

REF_LEN = cf.REF_LEN
WG_PER_CU = 4                   # the context's default (TCMI_P_WAVES)
STATS = ("one_sync_taken", "one_sync_declined", "one_sync_retried")
# what one decode of the file on the one-sync path must add to STATS, and the bit its decline must carry
DELTAS = {"hint_too_large": (1, 0, 1), "tiny_records": (0, 1, 1), "wide_skips": (0, 1, 0), "sparse_beyond_ref_len": (0, 1, 0), "all_n": (0, 1, 0),
          "stale_hint": (1, 0, 1), "ordinary": (1, 0, 0), "long_only": (1, 0, 0)}
FLAG = {"tiny_records": cf.PKF_REC_OVF, "wide_skips": cf.PKF_WORD_OVF, "sparse_beyond_ref_len": cf.PKF_CHUNK_OVF, "all_n": cf.PKF_EVENT_OVF}
DECLINED = tuple(FLAG)


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


class Lab:
    """the files, written once, and per file what the oracle says of it (computed once, shared, never changed)"""

    def __init__(self, tmp):
        self.tmp, self.paths, self.known = tmp, {}, {}

    def path(self, case):
        if case not in self.paths:
            p = self.tmp / (case + ".bam")
            if case == "ordinary":                                  # 20 000 x 150M, a hint of its own (the header's block holds records)
                ref, _ = sy.make_reference(L=REF_LEN, cds=[(100, 2000)])
                bamwriter.write_bam(str(p), sy.make_reads(ref, 20_000, seed=61), "ref", REF_LEN, level=1, split_records=True)
            else:
                cf.write(p, case)
            self.paths[case] = str(p)
        return self.paths[case]

    def add(self, name, path):
        self.paths[name] = str(path)
        return name

    def oracle(self, case, want=None):
        """-> reads, L = max(ref_len, extent), counts [L, 7], (plain, alt, flags) at mincov 30"""
        if case not in self.known:
            reads = c_oracle.read_bam(self.path(case))
            L = c_oracle.extent(reads, REF_LEN)
            counts = c_oracle.tally(reads, L) if want is None else want
            self.known[case] = (reads, L, counts, c_oracle.call(counts, 30, True))
        return self.known[case]


@pytest.fixture(scope="module")
def lab(tmp_path_factory):
    return Lab(tmp_path_factory.mktemp("capacities"))


def stats(ctx):
    return tuple(ctx.stat(k) for k in STATS)


def delta(ctx, before):
    return tuple(a - b for a, b in zip(stats(ctx), before))


def check_delta(ctx, before, case):
    got = delta(ctx, before)
    why = ctx.stat("one_sync_last_decline_flags")
    assert got == DELTAS[case], "%s: (taken, declined, retried) %s, expected %s; last decline flags 0x%x" % (case, got, DELTAS[case], why)
    if case in FLAG:
        assert why & FLAG[case], "%s declined with flags 0x%x, expected bit 0x%x" % (case, why, FLAG[case])


def figures(rs):
    return rs.n_reads, rs.n_piled, rs.algorithmic_bytes, rs.max_end


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@contextlib.contextmanager
def prepared(ctx, lab, case):
    """what a case needs of the context around ONE decode of its file: sparse_beyond_ref_len a packer grid of one workgroup per CU
    (4 * n_wg + 615 chunks is then fewer than its reads), stale_hint the mean record size of the helper file decoded just before"""
    try:
        if case == "sparse_beyond_ref_len":
            n_cu = ctx.stat("compute_units")
            assert n_cu <= cf.SPARSE_MAX_SLOTS, "a GPU of %d CUs: the file needs more reads to overflow the chunk capacity" % n_cu
            ctx.set_option("wg_per_cu", 1)
        if case == "stale_hint":
            d = engine.DeviceBam(lab.path("long_only"))
            before = stats(ctx)
            rs = ctx.upload_bamfile(d)
            check_delta(ctx, before, "long_only")
            assert rs.n_reads == 80
            rs.free()
            d.close()
        yield
    finally:
        ctx.set_option("wg_per_cu", WG_PER_CU)


def several_kernel_figures(ctx, path, blocks=None):
    d = engine.DeviceBam(path)
    try:
        ctx.set_option("one_sync", 0)
        before = stats(ctx)
        rs = ctx.upload_bamfile(d, blocks=blocks)
        assert delta(ctx, before) == (0, 0, 0)
        out = figures(rs)
        rs.free()
        return out
    finally:
        ctx.set_option("one_sync", 1)
        d.close()


def upload_and_step(ctx, lab, case, figs0=None, filtered=None):
    """ctx.upload_bamfile + ctx.step: stats, the read set's figures, counts and records against the oracle"""
    reads, L, want, (wp, wa, wf) = lab.oracle(case)
    d = engine.DeviceBam(lab.path(case))
    try:
        with prepared(ctx, lab, case):
            before = stats(ctx)
            rs = ctx.upload_bamfile(d)
            check_delta(ctx, before, case.split("+")[0])
        assert max(REF_LEN, rs.max_end) == L
        if figs0 is not None:
            assert figures(rs) == figs0, (case, figures(rs), figs0)
        if filtered is not None:
            assert rs.filtered == filtered
        plain, alt, flags, counts = ctx.step(rs, L, 30, True)
        rs.free()
        same(counts, want, case + ": counts")
        same(plain, wp, case + ": plain"), same(alt, wa, case + ": alt"), same(flags, wf, case + ": flags")
    finally:
        d.close()


def bamfile_step(ctx, lab, case, want_counts, figs0=None, filtered=None):
    """ctx.bamfile_step: the same"""
    reads, L, want, (wp, wa, wf) = lab.oracle(case)
    d = engine.DeviceBam(lab.path(case))
    try:
        with prepared(ctx, lab, case):
            before = stats(ctx)
            rs, plain, alt, flags, counts = ctx.bamfile_step(d, REF_LEN, 30, True, want_counts=want_counts)
            check_delta(ctx, before, case.split("+")[0])
        assert len(plain) == L == max(REF_LEN, rs.max_end)
        if figs0 is not None:
            assert figures(rs) == figs0, (case, figures(rs), figs0)
        if filtered is not None:
            assert rs.filtered == filtered
        rs.free()
        if want_counts:
            same(counts, want, case + ": counts")
        else:
            assert counts is None
        same(plain, wp, case + ": plain"), same(alt, wa, case + ": alt"), same(flags, wf, case + ": flags")
    finally:
        d.close()


@pytest.mark.parametrize("case", cf.CASES)
def test_every_file_by_both_entry_points(ctx, lab, case):
    reads, L, want, _ = lab.oracle(case)
    figs0 = several_kernel_figures(ctx, lab.path(case))
    assert figs0[0] == reads["n_reads"] and max(REF_LEN, figs0[3]) == L
    upload_and_step(ctx, lab, case, figs0)
    for want_counts in (True, False):
        bamfile_step(ctx, lab, case, want_counts, figs0)


@pytest.mark.parametrize("case", DECLINED)
def test_a_declined_step_leaves_the_context_as_a_fresh_one(ctx, lab, case):
    """tcmi_bamfile_step has run tally and call on a read set it then declines: the next file's records and counts are the oracle's,
    whichever of the two comes first, also behind two declined files in a row, and the next ordinary file takes the one-sync path."""
    other = DECLINED[(DECLINED.index(case) + 1) % len(DECLINED)]
    for first, second in ((case, "ordinary"), ("ordinary", case), (case, other)):
        bamfile_step(ctx, lab, first, False)
        bamfile_step(ctx, lab, second, False)
        bamfile_step(ctx, lab, second, True)
    bamfile_step(ctx, lab, "ordinary", False)


@pytest.mark.parametrize("case", ("wide_skips", "all_n"))
def test_block_ranges_of_an_overflowing_file_add_up_and_join(ctx, lab, case):
    reads, L, want, _ = lab.oracle(case)
    d = engine.DeviceBam(lab.path(case))
    try:
        nb = d.n_blocks
        assert nb >= 6
        for parts in (2, 3):
            cuts = [nb * k // parts for k in range(parts + 1)]
            acc, ranges, n_reads = np.zeros_like(want), [], 0
            for a, b in zip(cuts[:-1], cuts[1:]):
                rs = ctx.upload_bamfile(d, blocks=(a, b - a))
                assert figures(rs) == several_kernel_figures(ctx, lab.path(case), blocks=(a, b - a))
                ranges.append((a, b - a) + rs.range_anchors)
                n_reads += rs.n_reads
                acc += ctx.step(rs, L, 30, True)[3]
                rs.free()
            same(acc, want, "%s in %d ranges" % (case, parts))
            assert n_reads == reads["n_reads"]
            assert td.check_range_anchors(ranges, d.inflated_bytes) is None, ranges
    finally:
        d.close()


@contextlib.contextmanager
def floor(ctx, q):
    try:
        ctx.set_min_base_quality(q)
        yield
    finally:
        ctx.set_min_base_quality()


def superposed(unit, pos, L):
    """counts of copies of ONE read (unit: its counts from position 0 on) at the starts `pos`: a pileup is a sum over reads"""
    hist = np.bincount(pos, minlength=L)
    return np.stack([np.convolve(hist, unit[:, c])[:L] for c in range(7)], 1).astype(np.int32)


def test_wide_skips_under_a_base_quality_floor(ctx, lab, tmp_path):
    """File c, a quality per read from {12, 13, 30}, floor 13: the reads of quality 12 lose every token (an N token is tested with the
    quality of the next query base).  The words do not depend on the floor: declined with PKF_WORD_OVF as without one."""
    rng = np.random.default_rng(113)
    quals = rng.choice([12, 13, 30], 20000)
    specs = cf.wide_skips_specs(quals)
    reads = ss.reads_from_spec({"reads": specs})
    L = c_oracle.extent(reads, REF_LEN)
    # the pileup oracle walks token by token in Python (10 M tokens here): one read per quality through it, the file by superposition —
    # checked against the oracle itself on the file's first 800 reads
    want = np.zeros((L, 7), np.int32)
    for q in (12, 13, 30):
        unit = rsp.oracle_counts(ss.reads_from_spec({"reads": [dict(specs[0], pos=0, qual=q)]}), 13, 502)
        assert unit[:, 0].sum() == (0 if q < 13 else 502)
        want += superposed(unit, reads["pos"][quals == q], L)
    head = ss.reads_from_spec({"reads": specs[:800]})
    direct = rsp.oracle_counts(head, 13, L)
    part = np.zeros((L, 7), np.int32)
    for q in (12, 13, 30):
        unit = rsp.oracle_counts(ss.reads_from_spec({"reads": [dict(specs[0], pos=0, qual=q)]}), 13, 502)
        part += superposed(unit, head["pos"][quals[:800] == q], L)
    same(part, direct, "superposition against the pileup oracle")
    case = lab.add("wide_skips+floor", cf.write_reads(tmp_path / "c_q.bam", reads, "wide_skips"))
    lab.oracle(case, want)
    figs0 = several_kernel_figures(ctx, lab.path(case))             # (without a floor: the figures do not depend on it)
    with floor(ctx, 13):
        upload_and_step(ctx, lab, case, figs0)
        bamfile_step(ctx, lab, case, True, figs0)
        bamfile_step(ctx, lab, case, False, figs0)


def test_all_n_under_a_base_quality_floor(ctx, lab, tmp_path):
    """File e, every read's first 75 qualities 10 and its last 75 30, floor 20.  A skipped token pushes no event: 7 500 * 75 = 562 500
    events are left, fewer than the capacity of 1 048 576 — the file takes the one-sync path."""
    qual = [10] * 75 + [30] * 75
    specs = cf.all_n_specs(qual)
    reads = ss.reads_from_spec({"reads": specs})
    n_events = len(specs) * sum(q >= 20 for q in qual)
    assert n_events == 562_500
    fits = n_events <= cf.EVENT_FLOOR
    L = c_oracle.extent(reads, REF_LEN)
    want = rsp.oracle_counts(reads, 20, L)
    assert want[:, 0].sum() == n_events and want[:, 1:].sum() == 0
    # (the name's first part says which statistics to expect: those of an ordinary file if the events fit)
    case = lab.add(("ordinary" if fits else "all_n") + "+floor", cf.write_reads(tmp_path / "e_q.bam", reads, "all_n"))
    lab.oracle(case, want)
    figs0 = several_kernel_figures(ctx, lab.path(case))
    with floor(ctx, 20):
        upload_and_step(ctx, lab, case, figs0)
        bamfile_step(ctx, lab, case, True, figs0)
        bamfile_step(ctx, lab, case, False, figs0)


def test_hint_too_large_under_a_read_filter(ctx, lab, tmp_path):
    """File a with every fourth short read flagged 0x400, under exclude_flags = 0x400: the counts of the file written without those
    reads, 5 000 records filtered, and the same retry (a filtered record is still a record of the index)."""
    specs = cf.hint_too_large_specs(flag_quarter=True)
    kept = [r for r in specs if not r["flag"] & 0x400]
    assert len(specs) - len(kept) == 5000
    a = lab.add("hint_too_large+flagged", cf.write_reads(tmp_path / "a_flagged.bam", ss.reads_from_spec({"reads": specs}), "hint_too_large"))
    b = lab.add("hint_too_large+kept", cf.write_reads(tmp_path / "a_kept.bam", ss.reads_from_spec({"reads": kept}), "hint_too_large"))
    _, L, want, _ = lab.oracle(b)
    lab.oracle(a, want)
    assert c_oracle.extent(c_oracle.read_bam(lab.path(a)), REF_LEN) == L
    upload_and_step(ctx, lab, b, filtered=0)                        # the file without them, no filter: the same counts from the device
    try:
        ctx.set_read_filter(0, 0, 0x400)
        ctx.set_option("one_sync", 0)
        d = engine.DeviceBam(lab.path(a))
        rs = ctx.upload_bamfile(d)
        figs0 = figures(rs)
        assert rs.filtered == 5000 and figs0[0] == len(specs)
        rs.free()
        d.close()
        ctx.set_option("one_sync", 1)
        upload_and_step(ctx, lab, a, figs0, filtered=5000)
        bamfile_step(ctx, lab, a, True, figs0, filtered=5000)
        bamfile_step(ctx, lab, a, False, figs0, filtered=5000)
    finally:
        ctx.set_option("one_sync", 1)
        ctx.set_read_filter()


def test_flat_arrays_full_of_n_take_the_event_re_pack(ctx, lab):
    """The reads of file e as flat arrays: 1 125 000 events against the first capacity of 1 048 576 — tcmi_pack_on_device packs once
    more with room for all (a read set that still reports packed_on_device, with every event: the oracle's counts); the host packer
    ("device_pack" 0) gives the same counts and figures."""
    reads = cf.reads_of("all_n")
    L = c_oracle.extent(reads, REF_LEN)
    want = c_oracle.tally(reads, L)
    assert int((want[:, 0] - want[:, 1:5].sum(1)).sum()) == 1_125_000 > cf.EVENT_FLOOR
    got = {}
    try:
        for device_pack in (1, 0):
            ctx.set_option("device_pack", device_pack)
            rs = ctx.upload(reads)
            assert rs.packed_on_device == bool(device_pack)
            got[device_pack] = figures(rs)
            plain, alt, flags, counts = ctx.step(rs, L, 30, True)
            rs.free()
            same(counts, want, "device_pack %d" % device_pack)
    finally:
        ctx.set_option("device_pack", 1)
    assert got[1] == got[0] and got[1][0] == 7500
