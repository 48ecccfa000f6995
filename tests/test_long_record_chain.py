"""GPU: the record chain where records cover dozens of BGZF blocks.  Three pieces of code decide where records start and end across
block boundaries — the host rule (csrc/bgzf_host.cpp: tcmi_bam_chain_check, the several-kernel path), rec_vouch / rec_scan
(csrc/bam_device.hip: one workgroup, a stretch of ceil(blocks / 1024) blocks a lane, joined through LDS, a serial walk when a find
is off) and pk_place's wavefront 0 (csrc/pack_device.hip: a look-back over the blocks' transfer functions, 64 blocks a trip; under
"prefix_kernels" the sums come from pk_prefix) — and here they meet files whose records cover up to 148 blocks of 512 bytes, in more
than 2 048 blocks: whole, as block ranges that begin, end and lie inside long records, as ranks and sub-ranges of the split step,
with a false record start planted above block 1024, and with arbitrary bytes in the long records.  Every expectation comes from the
plain model of tests/long_records.py (zlib + a Python walk; tests/test_long_record_model.py holds the host rule to it on the CPU) and
from the oracle's tally; every route is asserted to be the one meant (device_file.uploaded(how=...))."""
import struct

import numpy as np
import pytest

from oracle import c_oracle
from tests import long_records as lr
from tests.device_file import PACKERS, check_decode, uploaded
from trueconsense_amd import _ffi, _state, distributed

pytestmark = pytest.mark.gpu

KINDS = {"brim512": (512, True, False), "htslib512": (512, False, False), "brim1024": (1024, True, False), "tail512": (512, True, True)}
ROUTES = (("one_sync", 0), ("one_sync", 1), ("several_kernels", 0))               # (packer, "prefix_kernels")


@pytest.fixture(scope="module")
def ctx():
    return _state.default_context()


class File:
    def __init__(self, path, reads, L):
        self.path, self.reads, self.L = path, reads, L
        self.m = lr.Model(path)
        self.want = c_oracle.tally(reads, L)
        assert len(self.m.rec) == reads["n_reads"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("long_record_chain")
    out = {}
    for kind, (block, split, tail) in KINDS.items():
        path, _, reads, L, _ = lr.build(tmp, block, split, tail=tail)
        out[kind] = File(path, reads, L)
    # one long read in the middle of the file: the cut of two sub-ranges of the whole file falls inside it
    specs, which = lr.make_specs(long_reads=((3_000, 49_999),))
    path, _, reads, L, _ = lr.build(tmp, 512, True, name="middle512.bam", specs=specs, which=which)
    out["middle512"] = File(path, reads, L)
    return out


def counts_of(ctx, rs, L):
    return ctx.step(rs, L, 30, True)[3]


def through(ctx, f, how, blocks=None, prefix=0):
    """-> (n_reads, n_piled, anchors, counts) of the file or a block range of it on one packer, the route asserted"""
    try:
        ctx.set_option("prefix_kernels", prefix)
        with uploaded(ctx, f.path, blocks=blocks, how=how) as rs:
            return rs.n_reads, rs.n_piled, rs.range_anchors, counts_of(ctx, rs, f.L).astype(np.int64)
    finally:
        ctx.set_option("prefix_kernels", 0)


def refused(ctx, path, blocks=None):
    """both packers' refusals -> [(code, message)]; an upload that succeeds fails the test"""
    out = []
    for how in PACKERS:
        with pytest.raises(_ffi.TcmiError) as e:
            with uploaded(ctx, path, blocks=blocks, one_sync=int(how == "one_sync")):
                pass
        out.append((e.value.code, str(e.value)))
    return out


# ---- (a) whole files -------------------------------------------------------------------------------------------------------------------------
def test_the_files_are_what_the_paths_need(files):
    lr.check_conditions(files["brim512"].m, files["htslib512"].m, files["brim1024"].m)
    m = files["tail512"].m
    for i in m.long_records():
        assert m.ulen[m.touched(i)[0]] - (m.rec[i] - m.start[m.touched(i)[0]]) == 3


@pytest.mark.parametrize("kind", list(KINDS))
def test_whole_files_on_every_route(ctx, files, kind):
    """stream and record index against zlib (rec_vouch, rec_scan, rec_compact); n_reads, n_piled and the count matrix against the oracle
    through the one-sync packer (pk_place's look-back adds the blocks up itself), under "prefix_kernels" and through the several-kernel
    path (the host rule)"""
    f = files[kind]
    check_decode(ctx, f.path).close()
    orc = c_oracle.read_bam(f.path)
    assert orc["n_reads"] == f.reads["n_reads"]
    for how, prefix in ROUTES:
        n_reads, n_piled, anchors, counts = through(ctx, f, how, prefix=prefix)
        assert (n_reads, n_piled, anchors) == (orc["n_reads"], int(((orc["flag"] & 4) == 0).sum()), (-1, -1)), (how, prefix)
        assert np.array_equal(counts, f.want), (how, prefix, np.argwhere(counts != f.want)[:5])


# ---- (b) block ranges ------------------------------------------------------------------------------------------------------------------------
def ranges_around(m):
    """for every long record over blocks [s, e]: ranges to the file's end from s, s + 1, the middle, e and e + 1; ranges from block 0
    whose last own block is s - 1, s, e - 1 or e; a range wholly inside the record"""
    out = []
    for i in m.long_records():
        s, e = m.touched(i)
        out += [(x, -1) for x in (s, s + 1, (s + e) // 2, e, e + 1)]
        out += [(0, x + 1) for x in (s - 1, s, e - 1, e)]
        out.append((s + 1, max(1, (e - s) // 2)))
    return out


@pytest.mark.parametrize("kind", ("brim512", "htslib512", "brim1024"))
def test_block_ranges_that_begin_end_and_lie_inside_long_records(ctx, files, kind):
    f = files[kind]
    m = f.m
    rg = [m.range(*b) for b in ranges_around(m)]
    seg = lr.SegmentTally(f.reads, f.L, [x for r in rg for x in r["records"]])
    n_refused = n_inside = 0
    for r in rg:
        blocks = (r["first_block"], r["n_own"])
        if r["refused"]:
            for code, msg in refused(ctx, f.path, blocks):
                assert code == _ffi.E_UNSUPPORTED and lr.E_UNSUPPORTED_WORDS in msg, (blocks, msg)
            n_refused += 1
            continue
        i0, i1 = r["records"]
        want = seg.of(i0, i1)
        for how in PACKERS:
            n_reads, _, anchors, counts = through(ctx, f, how, blocks)
            assert n_reads == i1 - i0 and anchors == (r["range_first"], r["range_next"]), (how, blocks, n_reads, anchors, r)
            assert np.array_equal(counts, want), (how, blocks, np.argwhere(counts != want)[:5])
        if i1 == i0:                                                # a range inside one record: no reads, a zero matrix, no anchors
            assert (r["range_first"], r["range_next"]) == (-1, -1) and not want.any()
            n_inside += 1
    assert n_refused >= len(lr.LONG) - 1 and n_inside >= len(lr.LONG) - 1, (n_refused, n_inside)


@pytest.mark.parametrize("kind", ("brim512", "htslib512"))
def test_ranges_of_cut_lists_join_and_add_up(ctx, files, kind):
    """cut lists with cuts at the blocks long records start and end in: the device's anchors join (check_range_anchors) and the parts'
    matrices add up to the file's, on both packers"""
    f = files[kind]
    joined = 0
    for cuts in lr.cut_lists(f.m):
        ranges = f.m.cut(cuts)
        if any(r["refused"] for r in ranges):
            continue
        for how in PACKERS:
            table, acc = [], np.zeros_like(f.want, dtype=np.int64)
            for r in ranges:
                _, _, anchors, counts = through(ctx, f, how, (r["first_block"], r["n_own"]))
                table.append((r["first_block"], r["n_own"]) + anchors)
                acc += counts
            assert table == f.m.anchors(ranges) and distributed.check_range_anchors(table, f.m.inflated) is None, (how, cuts, table)
            assert np.array_equal(acc, f.want), (how, cuts)
        joined += 1
    assert joined >= 4


# ---- (c) ranks and sub-ranges through the product ------------------------------------------------------------------------------------------------
def oracle_fasta(f, mincov):
    from oracle import tc_oracle as orc
    _, orfs = lr.reference()
    has, ins = orc.list_inserts(f.want, mincov, lambda pos1: [])
    cons, _ = orc.build_consensus(mincov, f.want, [dict(o) for o in orfs], True, ins if has else None, True)
    return orc.fasta_text("S", mincov, cons)


def rows():
    return [{"start": o["start"], "end": o["end"], "strand": "+"} for o in lr.reference()[1]]


def test_rank_boundaries_inside_long_records(files):
    """distributed.split_ranks_in_turn at world sizes the model chooses from distributed.block_range.  W1: a rank's range begins inside
    a long record and no range is refused — counts and FASTA equal a world = 1 run's and the oracle's.  W2: some rank's range ends in
    a long record that its extra block does not end — TcmiError, E_UNSUPPORTED, naming the rank: never a wrong matrix."""
    f = files["brim512"]
    m = f.m
    se = [m.touched(i) for i in m.long_records()]
    inside = lambda rk: any(s < r["first_block"] <= e for r in rk for s, e in se)
    w1 = next(w for w in range(2, 17) if inside(m.ranks(w)) and not any(r["refused"] for r in m.ranks(w)))
    w2 = next(w for w in range(2, 17) if any(r["refused"] for r in m.ranks(w)))
    text1, counts1, _ = distributed.split_ranks_in_turn(f.path, f.L, rows(), 10, 1, return_parts=True, split_sub=1)
    assert np.array_equal(counts1, f.want) and text1 == oracle_fasta(f, 10)
    text, counts, _ = distributed.split_ranks_in_turn(f.path, f.L, rows(), 10, w1, return_parts=True, split_sub=1)
    assert np.array_equal(counts, f.want) and text == text1, w1
    bad = [k for k, r in enumerate(m.ranks(w2)) if r["refused"]]
    with pytest.raises(_ffi.TcmiError) as e:
        distributed.split_ranks_in_turn(f.path, f.L, rows(), 10, w2, return_parts=True, split_sub=1)
    # (the ranks play in turn from the last one down: the first refusal met is the highest rank's)
    assert e.value.code == _ffi.E_UNSUPPORTED and "rank %d of %d" % (bad[-1], w2) in str(e.value) and lr.E_UNSUPPORTED_WORDS in str(e.value), str(e.value)


@pytest.mark.parametrize("K", (2, 3))
def test_sub_ranges_cut_inside_long_records(files, K):
    """"split_sub" = K: a rank's range as K sub-ranges side by side.  One layout in which the model says every rank's sub-ranges decode
    and join (split_sub_taken = the ranks), one in which a sub-range's last record overruns its extra block or a sub-range holds no
    record start in every rank that tries (split_sub_taken = 0: each range goes in one piece) — the oracle's counts in both."""
    def layout(f, w):
        rk = f.m.ranks(w)
        if any(r["refused"] for r in rk):
            return None
        subs = [f.m.sub_ranges(r["first_block"], r["n_own"], K) for r in rk]
        return sum(1 for k, _, _ in subs if k > 1), sum(1 for k, _, ok in subs if k > 1 and ok)
    cand = [(f, w) for w in range(1, 9) for f in (files["brim512"], files["htslib512"], files["middle512"]) if layout(f, w)]
    joins = next((f, w) for f, w in cand if w >= 2 and layout(f, w) == (w, w))
    falls = next((f, w) for f, w in cand if layout(f, w)[0] > 0 and layout(f, w)[1] == 0)
    for (f, w), taken in ((joins, joins[1]), (falls, 0)):
        assert f.m.n_blocks // w // 64 >= K
        tm = {}
        _, counts, _ = distributed.split_ranks_in_turn(f.path, f.L, rows(), 10, w, return_parts=True, split_sub=K, timings=tm)
        assert tm["split_sub_taken"] == taken, (w, taken, tm["split_sub_taken"])
        assert np.array_equal(counts, f.want), (w, taken)


# ---- (d) a false start, at scale ---------------------------------------------------------------------------------------------------------------
def planted(tmp_path, fake, at, residue):
    """the recipe's file (512-byte blocks filled to the brim) with `fake` in a block above index 1024 that lies wholly inside the
    longest record's QUAL, at place `residue` of its lane's stretch in rec_vouch (block % ceil(blocks / 1024))
    -> (File, the block, the blocks [s, e] of that record)"""
    specs, which = lr.make_specs()
    path = str(tmp_path / "planted.bam")
    per = []

    def pick(inside):
        n_blocks = len(lr.block_ulens(path))
        per.append((n_blocks + 1023) // 1024)
        return next(b for b in inside if b > 1024 and b % per[0] == residue % per[0])
    reads, b = lr.plant(path, specs, which[2], fake, at, pick, "r", lr.REF_LEN)
    f = File(path, reads, lr.REF_LEN)
    assert per[0] == 3 and b > 1024 and b % per[0] == residue % per[0]
    return f, b, f.m.touched(which[2])


@pytest.mark.parametrize("residue", (0, 1, -1))
def test_a_false_start_above_block_1024_is_withdrawn(ctx, tmp_path, residue):
    """struct.pack("<I", 64) in the last four bytes of a block wholly inside a long record, the block first, second and last of its
    lane's stretch: rec_vouch's serial walk withdraws it, both packers take the file, the record list is the true one and the counts
    are the oracle's — whole, and as a range that holds the block behind records that vouch for the chain.  A range that begins inside
    the record, in front of the block, has nothing to vouch for its first find: refused, not wrong."""
    f, b, (s, e) = planted(tmp_path, struct.pack("<I", 64), -4, residue)
    found = lr.block_search(f.m, b)                                # (506: the fake's first two bytes behind two QUAL bytes read as a size too)
    assert s < b < e and f.m.first[b] == lr.NONE and 512 - 40 < found <= 508 and lr.predict(f.m) is None
    check_decode(ctx, f.path).close()
    for how in PACKERS:
        n_reads, _, _, counts = through(ctx, f, how)
        assert n_reads == f.reads["n_reads"] and np.array_equal(counts, f.want), how
    r = f.m.range(s - 3, -1)
    want = lr.SegmentTally(f.reads, f.L, r["records"]).of(*r["records"])
    for how in PACKERS:
        n_reads, _, anchors, counts = through(ctx, f, how, (s - 3, -1))
        assert n_reads == r["records"][1] - r["records"][0] and anchors == (r["range_first"], r["range_next"]), (how, anchors, r)
        assert np.array_equal(counts, want), how
    for code, _ in refused(ctx, f.path, (b - 2, -1)):
        assert code in (_ffi.E_UNSUPPORTED, _ffi.E_FORMAT)


def test_a_false_start_in_the_body_of_a_block_above_1024_is_still_refused(ctx, tmp_path):
    f, b, _ = planted(tmp_path, lr.record_head(2000), 100, 1)
    for code, msg in refused(ctx, f.path):
        assert code == _ffi.E_UNSUPPORTED and "the chain of alignment records does not close at BGZF block %d (found a start at 100," % b in msg, msg


# ---- (e) arbitrary bytes in long records: right or refused, never wrong ------------------------------------------------------------------
SEEDS = tuple(range(8))


def test_arbitrary_bytes_in_long_records_decode_right_or_are_refused(ctx, tmp_path):
    """Eight files of about 260 blocks of 512 bytes whose two long records carry random QUAL bytes (0 .. 93) and SEQ with N and =
    nibbles: plausible heads occur by accident (long_records.false_finds: one to seven blocks a file find a start that is none).  Both
    packers either refuse the file (E_UNSUPPORTED / E_FORMAT) or give exactly the oracle's n_reads and counts, and they do what the
    restated decode (long_records.predict) says; at least half of the seeds must decode.
    Seeds that decode, by the restatement on the CPU and on the first run on an MI355X alike: 0, 1, 2, 3, 4, 5, 6, 7 — every accidental
    find is a tail find in a block inside a record, which rec_vouch withdraws (none of seeds 8 .. 119 is refused either: a refusal
    needs a whole plausible head, and the planted one of the test above pins that side)."""
    decoded = []
    for seed in SEEDS:
        path, reads, L = lr.build_arbitrary(tmp_path, seed)
        want = c_oracle.tally(reads, L)
        ok = 0
        for how in PACKERS:
            try:
                with uploaded(ctx, path, how=how) as rs:
                    n_reads, counts = rs.n_reads, counts_of(ctx, rs, L)
            except _ffi.TcmiError as e:
                assert e.code in (_ffi.E_UNSUPPORTED, _ffi.E_FORMAT), (seed, how, str(e))
                continue
            assert n_reads == reads["n_reads"] and np.array_equal(counts, want), (seed, how)
            ok += 1
        assert ok in (0, len(PACKERS)), (seed, ok)                  # (the packers agree on what they take)
        assert bool(ok) == (lr.predict(lr.Model(path)) is None), (seed, ok)
        if ok:
            decoded.append(seed)
    print("seeds that decode:", decoded)
    assert len(decoded) >= len(SEEDS) // 2, decoded
