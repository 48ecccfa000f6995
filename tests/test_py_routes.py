"""The Python routes from a BAM file to its read set and to its FASTA, where the orchestration paths share one piece:
indexing.device_readset ("the device path, or say why not"), the one token-buffer loop of the three modal-token callers, the
split drivers' shared tail, and the borrowed contexts of the pipeline and the file runner."""
import gc
from collections import Counter

import numpy as np
import pytest

from oracle import c_oracle
from oracle import tc_oracle as orc
from tests import synth_small as ss
from trueconsense_amd import _ffi, _state, contigs, engine, indexing
from trueconsense_amd import synthetic as sy
from trueconsense_amd.io import bamwriter


# ------------------------------------------------------------------------------------------------ device_readset, with stand-ins
class _StubBam:
    made = []

    def __init__(self, path):
        self.path, self.closed = path, 0
        _StubBam.made.append(self)

    def close(self):
        self.closed += 1


class _FakeCtx:
    def __init__(self, result, floor=0):
        self.result, self.read_rules, self.calls = result, engine.ReadRules(min_baseq=floor), []

    def upload_bamfile(self, dbam, blocks=None):
        self.calls.append((dbam, blocks))
        if isinstance(self.result, Exception):
            raise self.result
        return self.result


@pytest.fixture
def stub_bam(monkeypatch):
    _StubBam.made = []
    monkeypatch.setattr(indexing, "DeviceBam", _StubBam)
    return _StubBam


def test_device_readset_returns_the_upload_and_closes_the_file(stub_bam):
    rs = object()
    ctx = _FakeCtx(rs)
    assert indexing.device_readset(ctx, "x.bam") is rs
    assert indexing.device_readset(ctx, "x.bam", blocks=(3, 4)) is rs
    assert [(d.path, b) for d, b in ctx.calls] == [("x.bam", None), ("x.bam", (3, 4))]
    assert [d.closed for d in stub_bam.made] == [1, 1]


def test_device_readset_is_none_when_the_decoder_declines_without_a_floor(stub_bam):
    ctx = _FakeCtx(_ffi.TcmiError(_ffi.E_UNSUPPORTED, "records straddle"))
    assert indexing.device_readset(ctx, "x.bam") is None
    assert [d.closed for d in stub_bam.made] == [1]


def test_device_readset_refuses_under_a_floor_with_the_reason(stub_bam):
    why = _ffi.TcmiError(_ffi.E_UNSUPPORTED, "records straddle")
    with pytest.raises(_ffi.TcmiError) as e:
        indexing.device_readset(_FakeCtx(why, floor=13), "some/x.bam")
    assert e.value.code == _ffi.E_UNSUPPORTED and e.value.__cause__ is why
    assert "--min-baseq 13 needs the device path (the host packer knows no base-quality floor), which some/x.bam left: " in str(e.value)
    assert str(e.value).endswith(str(why))
    assert [d.closed for d in stub_bam.made] == [1]


def test_device_readset_lets_other_errors_through(stub_bam):
    for floor in (0, 13):
        bad = _ffi.TcmiError(_ffi.E_FORMAT, "not a BAM")
        with pytest.raises(_ffi.TcmiError) as e:
            indexing.device_readset(_FakeCtx(bad, floor), "x.bam")
        assert e.value is bad
    assert [d.closed for d in stub_bam.made] == [1, 1]


# ------------------------------------------------------------------------------------------------ the one token-buffer loop
def _seq(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))


def _carriers(rng, n_cols, ins_len, spacing, per_col=3):
    """n_cols candidate columns `spacing` apart, each with per_col reads 5M<ins_len>I5M that carry the same insertion behind it.
    -> (read specs sorted by position, 1-based columns, the columns' tokens)."""
    reads, cols, inss = [], [], []
    for k in range(n_cols):
        p = 10 + spacing * k
        ins = _seq(rng, ins_len)
        left, right = _seq(rng, 5), _seq(rng, 5)
        for j in range(per_col):
            reads.append({"pos": p, "flag": 0, "cigar": "5M%dI5M" % ins_len, "seq": left + ins + right, "qual": 30, "name": "c%d_%d" % (k, j)})
        cols.append(p + 5)
        inss.append(left[-1] + "+%d" % ins_len + ins)
    return reads, cols, inss


def _oracle_modal(rd, cols):
    out = {}
    for c in cols:
        toks = orc.region_tokens(rd, c)
        out[c] = (Counter(t.upper() for t in toks).most_common(1)[0][0] if toks else None, len(toks))
    return out


def test_modal_tokens_grows_its_buffer_for_one_token_beyond_64_kib():
    """Three reads with the same 70 000-base insertion behind one column: the token alone exceeds the first 65 536-byte buffer."""
    reads, cols, inss = _carriers(np.random.default_rng(11), 1, 70_000, 20)
    rd = ss.reads_from_spec({"reads": reads})
    got = engine.modal_tokens(rd, cols + [cols[0] + 1])
    assert got == _oracle_modal(rd, cols + [cols[0] + 1])
    assert got[cols[0]] == (inss[0], 3) and len(got[cols[0]][0]) > (1 << 16)


def test_modal_tokens_grows_its_buffer_for_many_columns_beyond_64_kib():
    """700 candidate columns whose tokens of ~100 bytes each fit the first buffer one by one, but not together (one read a column:
    the oracle walks every read for every column)."""
    reads, cols, inss = _carriers(np.random.default_rng(12), 700, 96, 12, per_col=1)
    rd = ss.reads_from_spec({"reads": reads})
    got = engine.modal_tokens(rd, cols)
    assert sum(len(t) for t, _ in got.values()) > (1 << 16) and max(len(t) for t, _ in got.values()) < 128
    assert got == _oracle_modal(rd, cols)
    assert [got[c] for c in cols] == [(t, 1) for t in inss]


# ------------------------------------------------------------------------------------------------ the split drivers' shared tail
def test_consensus_split_at_world_1_sweeps_the_host_when_the_entries_are_refused(tmp_path):
    """consensus_split_bamfile with no process group: the one rank's entries_fn refuses (E_UNSUPPORTED: a read the entry kernel does not
    take), so the tokens come from the host sweep of the file, and the FASTA is the oracle chain's."""
    from tests.consensus_case import consensus_case, oracle_fasta
    from trueconsense_amd import distributed as td
    ref, orfs, reads = consensus_case()
    L = len(ref)
    want, ins = oracle_fasta(reads, orfs, L, 30)
    assert len(ins) >= 4
    path = str(tmp_path / "one.bam")
    bamwriter.write_bam(path, reads, "r", L, level=1)
    asked = []

    def step_fn(what):
        if what == "n_blocks":
            return 1
        if what[0] == "call":
            return c_oracle.call(what[1], what[2], what[3])
        return c_oracle.tally(reads, L)

    def entries_fn(pos):
        asked.append(list(pos))
        raise _ffi.TcmiError(_ffi.E_UNSUPPORTED, "a read of more than 512 positions")
    rows = [{"start": o["start"], "end": o["end"], "strand": "+"} for o in orfs]
    text, counts, toks = td.consensus_split_bamfile(path, L, rows, 30, True, "S", 0, 1, step_fn=step_fn, entries_fn=entries_fn, return_parts=True)
    assert text == want
    assert len(asked) == 1 and set(ins) <= set(asked[0]) == set(toks)
    assert np.array_equal(counts, c_oracle.tally(reads, L))


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    return _state.default_context()


@pytest.mark.gpu
def test_forced_decline_takes_the_host_leg_or_refuses_under_a_floor(ctx, tmp_path, monkeypatch):
    """The device decoder is made to decline (E_UNSUPPORTED): build_counts and step_contigs take their host legs and give the oracle's
    counts; under a base-quality floor both refuse with the same sentence; afterwards the context carries no floor, filter or layout."""
    L = 1000
    ref, _ = sy.make_reference(L=L, cds=[(100, 900)])
    reads = sy.make_reads(ref, 300, seed=31)
    want = c_oracle.tally(reads, L)
    path = str(tmp_path / "decl.bam")
    bamwriter.write_bam(path, reads, "r", L)
    shift, slot, axis = contigs.layout_for([("r", ref)], ["r"], [L])

    def declined(self, dbam, blocks=None):
        raise _ffi.TcmiError(_ffi.E_UNSUPPORTED, "forced")
    with monkeypatch.context() as m:
        m.setattr(engine.Context, "upload_bamfile", declined)
        assert np.array_equal(indexing.build_counts(path, L, ctx=ctx), want)
        assert indexing.build_counts.last_reads == 300
        info = {}
        out = contigs.step_contigs(ctx, path, shift, slot, axis, 30, True, ["r"], info=info)
        assert np.array_equal(out[3][:L], want) and not out[3][L:].any() and out[5] == 0 and out[6] is not None
        assert info == {"reads": 300, "reads_filtered": 0}
        out[6].close()
        said = []
        ctx.set_min_base_quality(13)
        try:
            with pytest.raises(_ffi.TcmiError) as e:
                indexing.build_counts(path, L, ctx=ctx)
            said.append(e.value)
        finally:
            ctx.set_min_base_quality(0)
        with pytest.raises(_ffi.TcmiError) as e:
            contigs.step_contigs(ctx, path, shift, slot, axis, 30, True, ["r"], rules=engine.ReadRules(min_baseq=13))
        said.append(e.value)
        assert [x.code for x in said] == [_ffi.E_UNSUPPORTED] * 2 and str(said[0]) == str(said[1])
        assert "--min-baseq 13 needs the device path (the host packer knows no base-quality floor), which %s left: " % path in str(said[0])
        assert str(said[0]).endswith("forced")
    assert ctx.min_base_quality == 0 and ctx.read_filter == (0, 0, 0)
    rs = indexing.device_readset(ctx, path)                    # the decoder itself again: no floor, no filter, reference 0 on its own axis
    try:
        assert rs.min_base_quality == 0 and rs.filtered == 0 and rs.n_reads == 300 and rs.dropped() == 0
        assert np.array_equal(ctx.step(rs, L, 30, True)[3], want)
        assert ctx.readset_modal_tokens(rs, [500])[500][1] > 0   # (a read set uploaded under a layout is refused here)
    finally:
        rs.free()


@pytest.mark.gpu
def test_readset_modal_tokens_grows_its_buffer_beyond_64_kib(ctx, tmp_path):
    """Candidate columns of a device-decoded file whose tokens sum to more than 65 536 bytes: 40 columns, each a 2 000-base insertion
    carried by three reads (700 columns of ~100 bytes where the device's own limits refuse insertions that long).  Equal to the host
    sweep.  Before the three callers shared one buffer loop this call allocated 64 KiB once and failed with E_ARG ("token buffer too
    small") on an input that the file runner retries for the same C function."""
    def case(n_cols, ins_len, spacing, seed):
        reads, cols, _ = _carriers(np.random.default_rng(seed), n_cols, ins_len, spacing)
        p = str(tmp_path / ("tok%d.bam" % n_cols))
        bamwriter.write_bam(p, ss.reads_from_spec({"reads": reads}), "r", 10 + spacing * n_cols + 20)
        d = engine.DeviceBam(p)
        rs = ctx.upload_bamfile(d)
        try:
            assert rs.packed_on_device
            return p, cols, ctx.readset_modal_tokens(rs, cols)
        finally:
            rs.free()
            d.close()
    try:
        p, cols, got = case(40, 2000, 20, 21)
    except _ffi.TcmiError as e:
        if e.code != _ffi.E_UNSUPPORTED:
            raise
        p, cols, got = case(700, 96, 12, 22)
    assert sum(len(t) for t, _ in got.values()) > (1 << 16)
    assert all(n == 3 for _, n in got.values())
    bam = engine.BamFile(p)
    try:
        assert got == engine.modal_tokens(bam, cols)
    finally:
        bam.close()


@pytest.mark.gpu
def test_file_runner_refuses_a_file_off_the_device_path_under_a_floor_or_a_mask(ctx, tmp_path):
    """A FileRunner told not to read its files for the device decoder (device_decode = False) hands every file to the host reader,
    whose packer knows neither a base-quality floor nor a primer mask: under either the file is refused with the flag's own
    sentence, the floor's first; without them it is decoded on the host and gives the device path's FASTA."""
    L = 600
    ref, orfs = sy.make_reference(L=L, cds=[(50, 500)])
    path = str(tmp_path / "off.bam")
    bamwriter.write_bam(path, sy.make_reads(ref, 100, read_len=100, seed=77), "r", L)
    rows = [{"start": o["start"], "end": o["end"], "strand": "+"} for o in orfs]
    floor = "--min-baseq 13 needs the device path (the host packer knows no base-quality floor), which this file left: it was not read for the device decoder"
    mask = "--primers needs the device path (the host packer knows no primer mask), which this file left: it was not read for the device decoder"
    primers = ([(60, 80, False), (400, 420, True)], 0)
    for settings, said in ((dict(min_baseq=13), floor), (dict(primers=primers), mask), (dict(min_baseq=13, primers=primers), floor)):
        runner = engine.FileRunner(ctx, rows, 10, gpu_streams=1, rules=engine.ReadRules(**settings))
        try:
            runner.device_decode = False
            with pytest.raises(_ffi.TcmiError) as e:
                runner.run([path], names=["s"], ref_len=L)
            assert e.value.code == _ffi.E_UNSUPPORTED and path in str(e.value) and said in str(e.value), str(e.value)
            assert list(runner.last_status) == [_ffi.E_UNSUPPORTED] and runner.decoded_on == {"device": 0, "host": 0}
        finally:
            runner.close()
    runner = engine.FileRunner(ctx, rows, 10, gpu_streams=1)
    try:
        runner.device_decode = False
        text = runner.run([path], names=["s"], ref_len=L)
        assert runner.decoded_on == {"device": 0, "host": 1} and list(runner.last_status) == [0]
        runner.device_decode = True
        assert runner.run([path], names=["s"], ref_len=L) == text and runner.decoded_on == {"device": 1, "host": 1}
        assert text[0].startswith(">s mincov=10\n") and len(text[0]) > L
    finally:
        runner.close()


@pytest.mark.gpu
def test_a_rules_block_leaves_the_context_under_none_and_set_rules_none_leaves_it_alone(ctx, tmp_path):
    """Context.rules(r) with all four rules set, left by an exception: behind the block the context is under none of them — what it
    reports, and the next upload of the file, which equals a fresh context's exactly.  Context.set_rules(None) keeps a floor that was
    set before.  The file: a pair whose mates share 15 columns, a duplicate, a read of quality 5, a read on its own."""
    L = 80
    seq = _seq(np.random.default_rng(5), 30)
    reads = [{"pos": 10, "flag": 99, "cigar": "30M", "seq": seq, "qual": 30, "name": "p", "mtid": 0, "mpos": 25, "tlen": 45},
             {"pos": 12, "flag": 0x400, "cigar": "30M", "seq": seq, "qual": 30, "name": "dup"},
             {"pos": 15, "flag": 0, "cigar": "30M", "seq": seq, "qual": 5, "name": "low"},
             {"pos": 25, "flag": 147, "cigar": "30M", "seq": seq, "qual": 30, "name": "p", "mtid": 0, "mpos": 10, "tlen": -45},
             {"pos": 40, "flag": 16, "cigar": "30M", "seq": seq, "qual": 30, "name": "own"}]
    path = str(tmp_path / "few.bam")
    bamwriter.write_bam(path, ss.reads_from_spec({"reads": reads}), "r", L)

    def upload(c):
        d = engine.DeviceBam(path)
        try:
            rs = c.upload_bamfile(d)
            try:
                return c.step(rs, L, 0, True)[3], (rs.n_reads, rs.n_piled, rs.filtered, rs.min_base_quality, rs.primers, rs.primer_masked_reads, rs.mate_overlap)
            finally:
                rs.free()
        finally:
            d.close()
    with engine.Context(0) as fresh:
        want = upload(fresh)
    assert want[1] == (5, 5, 0, 0, 0, 0, dict(on=0, pairs=0, clipped_reads=0, clipped_columns=0, ambiguous=0)) and want[0][:, 0].sum() == 150
    r = engine.ReadRules(read_filter=(0, 0, 0x400), min_baseq=13, primers=(((10, 14, False),), 0), mate_overlap=True)
    under = []
    with pytest.raises(ZeroDivisionError):
        with ctx.rules(r):
            assert ctx.read_rules == r
            under.append(upload(ctx))
            1 / 0
    counts, said = under[0]
    # (every rule took tokens away: the duplicate's 30, the low read's 30, the pair's 15 shared columns, the first mate's 4 in the primer)
    assert said == (5, 4, 1, 13, 1, 1, dict(on=1, pairs=1, clipped_reads=1, clipped_columns=15, ambiguous=0)) and counts[:, 0].sum() == 150 - 30 - 30 - 15 - 4
    assert ctx.read_rules == engine.ReadRules()
    assert (ctx.read_filter, ctx.min_base_quality, ctx.primers, ctx.mate_overlap) == ((0, 0, 0), 0, 0, False)
    got = upload(ctx)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    with engine.Context(0) as c:
        c.set_min_base_quality(13)
        c.set_rules(None)
        assert c.min_base_quality == 13 and c.read_rules == engine.ReadRules(min_baseq=13)
        assert upload(c)[1][3] == 13


@pytest.mark.gpu
def test_closing_borrowed_contexts_leaves_their_owner_usable(ctx, tmp_path):
    """FileRunner.contexts and Pipeline.ctx / slot_context(k) are the owner's: close() on them (and dropping them) destroys nothing."""
    ref, orfs = sy.make_reference(L=3000, cds=[(100, 1200), (1500, 2900)])
    L = len(ref)
    rows = [{"start": o["start"], "end": o["end"], "strand": "+"} for o in orfs]
    sets = [sy.make_reads(ref, 2000, seed=40 + k, indel_sites=sy.default_indel_sites(orfs)) for k in range(2)]
    dbams = []
    for k, reads in enumerate(sets):
        p = str(tmp_path / ("f%d.bam" % k))
        bamwriter.write_bam(p, reads, "ref", L)
        dbams.append(engine.DeviceBam(p).to_device(ctx))
    runner = engine.FileRunner(ctx, rows, 30, gpu_streams=2)
    pipe = engine.Pipeline(0, slots=2, walkers=1)
    rss = []
    try:
        before = runner.run_resident(dbams, names=["a", "b"], ref_len=L)
        assert before[0].startswith(">a mincov=30\n") and before[1].startswith(">b mincov=30\n") and before[0] != before[1]
        pipe.set_orfs([o["start"] for o in orfs], [o["end"] for o in orfs], [1] * len(orfs))
        rss = [pipe.ctx.upload(r) for r in sets]
        want, _ = pipe.run(rss, L, 30, True, host_reads=sets)
        borrowed = runner.contexts + [pipe.slot_context(k) for k in range(2)] + [pipe.ctx]
        assert len(borrowed) == 5 and all(c.handle for c in borrowed)
        for c in borrowed:
            c.close()
        del borrowed, c
        gc.collect()
        assert runner.run_resident(dbams, names=["a", "b"], ref_len=L) == before
        again, status = pipe.run(rss, L, 30, True, host_reads=sets)
        assert again == want and not status.any()
    finally:
        for rs in rss:                                          # (before their context goes with the pipeline)
            rs.free()
        pipe.close()
        runner.close()
        for d in dbams:
            d.close()
