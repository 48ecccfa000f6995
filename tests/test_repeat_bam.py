"""What tests/test_stream_scale.py rests on, checked without a GPU: tests/repeat_bam.repeat_records gives the records it says it gives,
every committed yardstick is additive over repeated records (a file with every record three times counts three times as much, under
the primer table, the floor and the read filter), tests/fixed_reads' numpy restatement equals those yardsticks on 2 000 records, and
the two launch caps the scale tests compute still stand in the source where they were read."""
import functools
import os
import re

import numpy as np
import pytest

from oracle import c_oracle
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
from tests import strand_yardstick as sy

L = fm.L
R = 3
SEED = 1
PER_READ = ("pos", "flag", "l_qseq", "tid", "mapq")
RAGGED = (("cigar_off", "cigar"), ("seq_off", "seq"), ("qual_off", "qual"))


# ------------------------------------------------------------------------------------------------------------------------ the caps


def test_the_two_caps_stand_in_the_source_where_the_scale_tests_read_them():
    """a change of either launch moves the record counts at which tests/test_stream_scale.py reaches a second trip: SC_BLOCK and
    SC_WG_PER_CU are read from the header (the test moves with them); pk_mask_long's 64 x 256 is restated there, so it is pinned here"""
    block, per_cu = rb.stream_count_caps()
    assert block > 0 and block % 64 == 0 and per_cu > 0
    text = open(os.path.join(rb.CSRC, "stream_count.h")).read()
    assert re.search(r"std::min<int64_t>\(blocks,\s*\(int64_t\)std::max\(ctx->n_cu,\s*1\)\s*\*\s*SC_WG_PER_CU\)", text), "the counting kernels' grid is no longer capped at compute units * SC_WG_PER_CU"
    assert "base += (int64_t)gridDim.x * SC_BLOCK" in text, "each_record no longer strides by the grid"
    pack = open(os.path.join(rb.CSRC, "pack_device.hip")).read()
    launches = re.findall(r"hipLaunchKernelGGL\(pk_mask_long,\s*dim3\((\w+)\),\s*dim3\((\w+)\)", pack)
    assert launches and set(launches) == {(str(rb.MASK_LONG_GRID), "PB")}, ("pk_mask_long's launch changed: adjust file B of tests/test_stream_scale.py", launches)
    assert re.search(r"\bPKF_EVENT_OVF\s*=\s*%d\s*," % dvf.PKF_EVENT_OVF, open(os.path.join(rb.CSRC, "pack_caps.h")).read()),"dvf.PKF_EVENT_OVF changed: tests/test_stream_scale.py admits that decline by its number"
    pb = re.search(r"constexpr\s+int\s+PB\s*=\s*(\d+)\s*;", pack)
    assert pb and int(pb.group(1)) == rb.MASK_LONG_BLOCK, "PB changed: adjust file B of tests/test_stream_scale.py"


# ------------------------------------------------------------------------------------------------------------------------ the helper
def take(rd, idx):
    """the flat arrays of the records idx (any order, repeats allowed) -> {field: array}, the ragged fields record by record"""
    out = {k: np.asarray(rd[k])[idx] for k in PER_READ}
    for off, data in RAGGED:
        o = np.asarray(rd[off]).astype(np.int64)
        out[data] = [np.asarray(rd[data])[o[i]:o[i + 1]].tobytes() for i in idx]
    return out


def same_records(got, want, label):
    assert sorted(got) == sorted(want)
    for k in want:
        if isinstance(want[k], list):
            assert got[k] == want[k], (label, k)
        else:
            assert np.array_equal(got[k], want[k]), (label, k)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the fuzz's seed 1 as the fuzz tests write it, and the same with every record three times -> (src, dst, their arrays)"""
    d = tmp_path_factory.mktemp("repeat")
    src = fm.write(d, fm.fuzz(SEED))
    dst = str(d / "R.bam")
    n = rb.repeat_records(src, dst, R)
    a, b = c_oracle.read_bam(src), c_oracle.read_bam(dst)
    assert n == R * len(fm.fuzz(SEED)) == int(b["n_reads"]) and int(a["n_reads"]) == len(fm.fuzz(SEED))
    return src, dst, a, b


def test_every_record_three_times_in_place(files):
    src, dst, a, b = files
    n = int(a["n_reads"])
    same_records(take(b, np.arange(R * n)), take(a, np.repeat(np.arange(n), R)), "r0 x 3, r1 x 3, ...")
    spec = rsp.arrays(fm.fuzz(SEED))                                             # ... and the source is what the fuzz wrote
    assert np.array_equal(a["pos"], spec["pos"]) and np.array_equal(a["flag"], spec["flag"]) and np.array_equal(a["mapq"], spec["mapq"])
    header, records = rb.split(rb.inflate(dst))
    assert header == rb.split(rb.inflate(src))[0] and len(records) == R * n
    # cut as write_bam cuts: the header in a block of its own, every other block starts on a record and holds no more than 0xFF00 bytes
    sizes = rb.block_sizes(dst)
    starts = set(np.cumsum([len(header)] + [len(r) for r in records]).tolist())
    assert sizes[0] == len(header) and sizes[-1] == 0 and len(sizes) == rb.n_blocks(dst) > 10 and max(sizes) <= rb.BLOCK
    assert all(int(at) in starts for at in np.cumsum(sizes[:-1]))


def test_the_tally_of_the_repeated_file_is_three_times_the_tally(files):
    _, _, a, b = files
    n_pos = c_oracle.extent(a, L)
    assert c_oracle.extent(b, L) == n_pos
    want = c_oracle.tally(a, n_pos)
    assert want[:, 0].max() > 100 and np.array_equal(c_oracle.tally(b, n_pos), R * want)


def passing(rd, f):
    flag = np.asarray(rd["flag"]).astype(np.int64)
    return sy.subset(rd, (np.asarray(rd["mapq"]) >= f[0]) & ((flag & f[1]) == f[1]) & ((flag & f[2]) == 0))


def test_every_yardstick_is_additive_over_repeated_records(files):
    """under the combined mode (the seed's table with slack 3, floor 13, the read filter): the count matrix with its masked reads and
    token counts, the strand halves, the link counts at one and seven neighbours and the reads per amplicon of the repeated file are
    each three times those of the source — what lets the scale tests multiply the yardstick of the small file"""
    _, _, a, b = files
    tabled, slack, q, f = fm.MODES["all"]
    table = fm.table_of(SEED)
    pa, pb = passing(a, f), passing(b, f)
    assert int(pb["n_reads"]) == R * int(pa["n_reads"]) and 0 < int(pa["n_reads"]) < int(a["n_reads"])
    want, got = py.counts(pa, L, table, q, slack), py.counts(pb, L, table, q, slack)
    assert np.array_equal(want[0], fm.yardstick(SEED, None, None, f, tabled, q, slack)[0])     # (the file read back is the fuzz's records)
    assert np.array_equal(got[0], R * want[0]) and tuple(got[1:]) == tuple(R * v for v in want[1:]) and want[1] > 0
    n_pos = len(want[0])
    cols = list(range(n_pos))
    for w, g in zip(sy.counts(pa, cols, L, table, q, slack), sy.counts(pb, cols, L, table, q, slack)):
        assert w.any() and np.array_equal(g, R * w)
    ca, cb = ly.classes(pa, L, table, q, slack, n_pos=n_pos), ly.classes(pb, L, table, q, slack, n_pos=n_pos)
    for use in (lkc.sparse_columns(SEED, n_pos), lkc.window_columns(want[0])):
        for k in (1, 7):
            w = ly.joint(ca, use, k)
            lkc.not_vacuous(w, (len(use), k))
            assert np.array_equal(ly.joint(cb, use, k), R * w)
    ka, kb = (ry.kept_columns(rd, None, f, rd["mapq"]) for rd in (a, b))
    assert len(kb) == R * len(ka) > 0
    for amps in (arc.tiled(7), arc.padded(arc.tiled(7), arc.LDS + 1)):
        for s in (0, 5):
            w = ry.counts(ka, amps, s)
            assert w[:7, 0].all() and w[len(amps):, 0].all() and np.array_equal(ry.counts(kb, amps, s), R * w)


def test_blocks_filled_to_the_brim_hold_the_same_records(files, tmp_path):
    src, dst, a, b = files
    brim = str(tmp_path / "B.bam")
    assert rb.repeat_records(src, brim, R, brim=True) == int(b["n_reads"])
    assert rb.inflate(brim) == rb.inflate(dst)
    idx = np.arange(int(b["n_reads"]))
    same_records(take(c_oracle.read_bam(brim), idx), take(b, idx), "brim")
    # ... and records do straddle: every block but the last is full, and a block boundary falls inside a record
    sizes = rb.block_sizes(brim)
    assert sizes[-1] == 0 and all(s == rb.BLOCK for s in sizes[:-2]) and len(sizes) > 3
    header, records = rb.split(rb.inflate(brim))
    starts = set(np.cumsum([len(header)] + [len(r) for r in records]).tolist())
    assert any(k * rb.BLOCK not in starts for k in range(1, len(sizes) - 2))


def test_keep_gives_exactly_the_kept_records(files, tmp_path):
    src, _, a, _ = files
    specs = fm.fuzz(SEED)
    long_ones = [i for i, r in enumerate(specs) if fm._piles_up(r) and fm._span(r) > fm.LONG]
    assert len(long_ones) == fm.n_long(specs) >= 15
    want = take(a, np.repeat(long_ones, 5))
    for how, keep in (("indices", long_ones), ("predicate", lambda i, rec: i in set(long_ones))):
        dst = str(tmp_path / (how + ".bam"))
        assert rb.repeat_records(src, dst, 5, keep=keep) == 5 * len(long_ones)
        got = c_oracle.read_bam(dst)
        assert int(got["n_reads"]) == 5 * len(long_ones)
        same_records(take(got, np.arange(int(got["n_reads"]))), want, how)
    # the predicate sees the record: the reverse-strand records alone (FLAG at byte 14 of the record)
    dst = str(tmp_path / "rev.bam")
    minus = np.nonzero(np.asarray(a["flag"]) & 16)[0]
    assert rb.repeat_records(src, dst, 2, keep=lambda i, rec: rec[14] & 16) == 2 * len(minus) > 0
    same_records(take(c_oracle.read_bam(dst), np.arange(2 * len(minus))), take(a, np.repeat(minus, 2)), "by FLAG")
    with pytest.raises(AssertionError):
        rb.repeat_records(src, dst, 2, keep=[int(a["n_reads"])])


# ------------------------------------------------------------------------------------------------------------------------ fixed reads
@functools.lru_cache(maxsize=None)
def fixed_case(which):
    """'spread': 2 000 records over the whole reference; 'head': the first 2 000 records of a 60 000-record set (depth in the hundreds)"""
    return fx.generate(2000, 7) if which == "spread" else fx.head(fx.generate(60000, 8), 2000)


@pytest.mark.parametrize("q", (0, 13))
@pytest.mark.parametrize("which", ("spread", "head"))
def test_the_numpy_restatement_equals_the_committed_yardsticks(tmp_path, which, q):
    """tests/fixed_reads on 2 000 of its records, written by write_bam_fast and read back by the C oracle, without a filter, with the
    MAPQ filter and with the filter under test_primer_mask's scheme with slack 3: the matrix, the masked reads, the strand halves, the link counts and the reads per amplicon are those of the committed yardsticks"""
    rd = fixed_case(which)
    back = c_oracle.read_bam(fx.write(tmp_path / "C.bam", rd))
    assert int(back["n_reads"]) == 2000 and np.array_equal(back["pos"], rd["pos"]) and np.array_equal(back["mapq"], rd["mapq"])
    n_pos = c_oracle.extent(back, fx.L)
    assert n_pos == fx.L
    covered = np.nonzero(c_oracle.tally(back, n_pos)[:, 0])[0]
    window = list(range(int(covered[0]), min(int(covered[0]) + 120, n_pos)))
    sparse = sorted(set(int(c) for c in np.random.default_rng(3).choice(covered, 11, replace=False)))
    for f, table, slack in ((fm.NONE, (), 0), (fx.MQ, (), 0), (fx.MQ, sch.PRIMER_SCHEME, 3)):
        kept = passing(back, f)
        assert (f == fm.NONE) == (int(kept["n_reads"]) == 2000) and int(kept["n_reads"]) > 500
        whole, n_masked = py.counts(kept, fx.L, table, q, slack)[:2]
        assert np.array_equal(fx.matrix(rd, n_pos, q, f, table, slack), whole) and whole[:, 1:5].sum(0).all() and (whole[:, 0] > whole[:, 1:5].sum(1)).any()
        assert fx.masked_reads(rd, f, table, slack) == n_masked and (n_masked > 20) == bool(table)
        assert q == 0 or whole[:, 0].sum() < py.counts(kept, fx.L, table, 0, slack)[0][:, 0].sum()
        assert not table or whole[:, 0].sum() < py.counts(kept, fx.L, (), q)[0][:, 0].sum()
        cols = list(range(n_pos))
        for got, want in zip(fx.strand(rd, cols, q, f, table, slack), sy.counts(kept, cols, fx.L, table, q, slack)):
            assert want.any() and np.array_equal(got, want)
        cls = ly.classes(kept, fx.L, table, q, slack, n_pos=n_pos)
        for use in (window, sparse, sparse[:1] + [n_pos + 5]):
            for k in (1, 7):
                want = ly.joint(cls, use, k)
                assert np.array_equal(fx.links(rd, use, k, q, f, table, slack), want) and (want.any() or len(use) == 2)
        columns = ry.kept_columns(back, None, f, back["mapq"])
        for amps in (fx.SCHEME, arc.padded(fx.SCHEME, arc.LDS + 1)):
            for s in (0, 5):
                want = ry.counts(columns, amps, s)
                assert np.array_equal(fx.amplicon_reads(rd, amps, s, f), want) and want[:, 0].sum() == len(columns)
    assert fx.SCHEME[:7] == arc.tiled(7)
    if which == "spread":
        want = ry.counts(ry.kept_columns(back), fx.SCHEME, 0)
        assert want[:8, 0].all() and want[7, 1] > 0 and want[8, 0] > 0 and want[9, 0] > 0     # reads in every amplicon, full-length ones, ambiguous, unassigned
