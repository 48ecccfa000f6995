"""BAM files whose records cover dozens of BGZF blocks — the shape of long-read files — and a plain model of what a correct decoder
must report for them, block by block and block range by block range: zlib, a Python walk of the block_size chain and the blocks'
ISIZEs, nothing else (device_file.host_stream_and_records, repeat_bam.block_sizes).  Beside them: a false record start planted in a
chosen block of a chosen long record, and the decoder's plausibility test restated, for the tests that ask what a block's own search
finds.  No GPU, no tests in here (tests/test_long_record_model.py, tests/test_long_record_chain.py, tests/test_bam_device.py)."""
import struct

import numpy as np

from tests import synth_small as ss
from tests.device_file import host_stream_and_records
from tests.repeat_bam import block_sizes
from trueconsense_amd import synthetic as sy
from trueconsense_amd.io import bamwriter

REF_LEN = 60_000
N_SHORT, SHORT = 6_500, 60
SHORT_SPAN = 10_000                                                  # the short reads start in [0, SHORT_SPAN - SHORT]: a long read behind any of them ends inside the reference
LONG = ((800, 40_000), (2_500, 23_000), (4_000, 49_999), (5_200, 9_000))        # (behind short read, bases)
NONE = 0xFFFFFFFF                                                    # bgzf_host.h: no record start in the block
E_UNSUPPORTED_WORDS = "a record longer than a BGZF block at the end of a block range"


def record_head(block_size):
    """the fixed fields the search tests, all plausible: refID 0, pos 5, l_read_name 2, one CIGAR op, l_seq 4, no mate (44 bytes needed)"""
    return struct.pack("<IiiIIIii", block_size, 0, 5, 2, 1, 4, -1, -1)


def block_ulens(path):
    """ISIZE of every BGZF block of the file"""
    return block_sizes(path)


def qual_at(rec_start, spec):
    """offset of a record's QUAL in the stream (bamwriter.write_bam: block_size, 32 fixed bytes, name + NUL, CIGAR, SEQ, QUAL)"""
    return int(rec_start) + 36 + len(spec["name"]) + 1 + 4 * len(ss.parse_cigar(spec["cigar"])) + (len(spec["seq"]) + 1) // 2


def plant(path, specs, which, fake, at, pick, ref_name, ref_len, block=512):
    """Write specs to `path` in blocks filled to the brim, with `fake` in the QUAL of read `which` (no floor: the counts do not depend on
    it) at offset `at` (< 0: from the end) of a block of `block` bytes that lies wholly inside that QUAL: pick(those blocks' indices) says
    which.  The record offsets must be what they were without the fake.  -> (reads, that block's index)"""
    bamwriter.write_bam(path, ss.reads_from_spec({"reads": specs}), ref_name, ref_len, block=block, split_records=True)
    rec = host_stream_and_records(path)[1]
    q0, rec_end = qual_at(rec[which], specs[which]), int(rec[which + 1]) if which + 1 < len(rec) else None
    assert rec_end is not None and rec_end - q0 == len(specs[which]["seq"])
    starts = np.concatenate(([0], np.cumsum(block_ulens(path))))
    inside = [k for k in range(len(starts) - 1) if starts[k] >= q0 and starts[k + 1] <= rec_end and starts[k + 1] - starts[k] == block]
    b = pick(inside)
    assert b in inside, (b, inside[:3], inside[-3:])
    where = int(starts[b]) + (at if at >= 0 else block + at) - q0
    assert 0 <= at + (block if at < 0 else 0) <= block - len(fake)
    if isinstance(specs[which]["qual"], int):
        specs[which]["qual"] = [specs[which]["qual"]] * len(specs[which]["seq"])
    specs[which]["qual"][where:where + len(fake)] = list(fake)
    reads = ss.reads_from_spec({"reads": specs})
    bamwriter.write_bam(path, reads, ref_name, ref_len, block=block, split_records=True)
    stream, rec2 = host_stream_and_records(path)
    assert np.array_equal(rec2, rec) and bytes(stream[int(starts[b]) + at % block:][:len(fake)]) == bytes(fake)
    return reads, b


def false_start_inside_a_record(tmp_path, fake, at):
    """One read of 1 500 bases among short ones, in 512-byte blocks filled to the brim: its record of 2.3 KB covers whole blocks.
    `fake` goes into its QUAL (no floor: the counts do not depend on it), at offset `at` (< 0: from the end) of a block that lies
    wholly inside the record.  Every other QUAL byte is 30 and SEQ holds A / C / G / T only: four such bytes never read as
    block_size < 2^24, so `fake` is the only place in the long record where the decoder's search for a record start can say yes.
    -> (path, reads, L, that block's index, the read's index)"""
    ref, _ = sy.make_reference(L=3000, cds=[(10, 600)])
    mk = lambda pos, n, name: {"pos": pos, "flag": 0, "cigar": "%dM" % n, "seq": ref[pos:pos + n], "qual": [30] * n, "name": name}
    specs = [mk(20 + 7 * k, 60, "a%d" % k) for k in range(8)] + [mk(100, 1500, "long")] + [mk(120 + 9 * k, 60, "b%d" % k) for k in range(12)]
    which = 8
    path = str(tmp_path / "inside.bam")
    reads, b = plant(path, specs, which, fake, at, lambda inside: inside[0], "r", len(ref))
    return path, reads, len(ref), b, which


# ---- the files -----------------------------------------------------------------------------------------------------------------------------
_REF = {}


def reference():
    if "ref" not in _REF:
        _REF["ref"] = sy.make_reference(L=REF_LEN, cds=[(10, 600)])
    return _REF["ref"]


def make_specs(seed=7, n_short=N_SHORT, long_reads=LONG, rng_long=None):
    """n_short reads of 60 bases, constant quality 30, A / C / G / T only, sorted; the long reads behind the short reads LONG names, each
    at its predecessor's position.  rng_long: the long reads carry random QUAL bytes (0 .. 93) and SEQ with N and = nibbles instead —
    accidental plausible record heads can occur.  -> (specs, the long reads' indices)"""
    ref, _ = reference()
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.integers(0, SHORT_SPAN - SHORT + 1, n_short))
    specs, which = [], []
    behind = {k: n for k, n in long_reads}
    for k in range(n_short):
        p = int(pos[k])
        specs.append({"pos": p, "flag": 0, "cigar": "%dM" % SHORT, "seq": ref[p:p + SHORT], "qual": 30, "name": "a%d" % k})
        if k in behind:
            n = behind[k]
            assert p + n <= REF_LEN
            seq, qual = ref[p:p + n], 30
            if rng_long is not None:
                seq = "".join("ACGTN="[int(x)] for x in rng_long.choice(6, n, p=[0.22, 0.22, 0.22, 0.22, 0.06, 0.06]))
                qual = [int(x) for x in rng_long.integers(0, 94, n)]
            which.append(len(specs))
            specs.append({"pos": p, "flag": 0, "cigar": "%dM" % n, "seq": seq, "qual": qual, "name": "long%d" % len(which)})
    return specs, which


def build(tmp, block, split_records, tail=False, seed=7, name=None, specs=None, which=None):
    """The recipe's file in `tmp` -> (path, specs, reads, L, the long reads' indices).
    tail: (files filled to the brim) the names of the records in front of every long record are lengthened until that long record
    starts in the last three bytes of a block — its size field straddles the block's end."""
    if specs is None:
        specs, which = make_specs(seed)
    path = str(tmp / (name or "long_%d_%s%s.bam" % (block, "brim" if split_records else "htslib", "_tail" if tail else "")))
    write = lambda: bamwriter.write_bam(path, ss.reads_from_spec({"reads": specs}), "r", REF_LEN, block=block, split_records=split_records)
    write()
    if tail:
        assert split_records, "htslib cuts start a record larger than a block on a block of its own: offset 0"
        for w in which:
            at = int(host_stream_and_records(path)[1][w]) % block   # (blocks filled to the brim: block b starts at b * block)
            d = (block - 3 - at) % block
            for k in range(w - 1, w - 4, -1):                       # (a name holds 254 characters; the record in front stays short enough to start in the same block)
                add = min(d, 170)
                specs[k]["name"] += "x" * add
                d -= add
            assert d == 0
            write()
            assert int(host_stream_and_records(path)[1][w]) % block == block - 3
    reads = ss.reads_from_spec({"reads": specs})
    return path, specs, reads, REF_LEN, which


def slice_reads(reads, a, b):
    """records [a, b) of flat read arrays, for c_oracle.tally (the offset arrays keep pointing into the whole CIGAR / SEQ arrays)"""
    out = {"n_reads": b - a}
    for k in ("pos", "flag", "l_qseq", "tid"):
        out[k] = np.ascontiguousarray(reads[k][a:b])
    for k in ("cigar_off", "seq_off"):
        out[k] = np.ascontiguousarray(reads[k][a:b + 1])
    out["cigar"], out["seq"] = reads["cigar"], reads["seq"]
    return out


class SegmentTally:
    """c_oracle.tally of any run of records [a, b) with a and b among `cuts`: every stretch between two neighbouring cuts is tallied
    once, a run's matrix is the sum of its stretches (a tally is additive over records)."""

    def __init__(self, reads, L, cuts):
        from oracle import c_oracle
        self.cuts = sorted(set(int(c) for c in cuts) | {0, int(reads["n_reads"])})
        self.L = L
        self.seg = [c_oracle.tally(slice_reads(reads, a, b), L).astype(np.int64) for a, b in zip(self.cuts[:-1], self.cuts[1:])]

    def of(self, a, b):
        i, j = self.cuts.index(int(a)), self.cuts.index(int(b))
        out = np.zeros((self.L, 7), np.int64)
        for s in self.seg[i:j]:
            out += s
        return out


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
class Model:
    """What a correct decoder must report for the file, with the meanings csrc/bgzf_host.h gives the words.
    Per block: entry (-1 header only, >= 0 the first record where the header says, -2 the block finds it), first (offset of the first
    record start in the block, NONE: none), over (bytes the block's last record runs past the block, 0 without a start).
    Per block range: range(first_block, n_blocks)."""

    def __init__(self, path):
        self.path = path
        self.stream, rec = host_stream_and_records(path)
        self.rec = rec.astype(np.int64)
        self.ulen = np.array(block_sizes(path), np.int64)
        self.n_blocks = len(self.ulen)
        self.start = np.concatenate(([0], np.cumsum(self.ulen)))    # block b holds stream bytes [start[b], start[b + 1])
        self.inflated = int(self.start[-1])
        assert self.inflated == len(self.stream) and len(self.rec)
        self.end = np.concatenate((self.rec[1:], [self.inflated]))  # where record i ends: the next one's start
        # the records that start in block b: [lo[b], lo[b + 1])
        self.lo = np.searchsorted(self.rec, self.start, "left")
        nb = self.n_blocks
        has = self.lo[1:] > self.lo[:-1]
        self.entry = np.full(nb, -2, np.int64)
        rec0 = int(self.rec[0])
        for b in range(nb):
            if rec0 >= self.start[b + 1]:
                self.entry[b] = -1
            else:
                self.entry[b] = rec0 - self.start[b]
                break
        self.first = np.where(has, self.rec[np.minimum(self.lo[:-1], len(self.rec) - 1)] - self.start[:-1], NONE)
        self.over = np.where(has, self.end[np.maximum(self.lo[1:] - 1, 0)] - self.start[1:], 0)
        assert (self.over >= 0).all()
        # the block a record starts in / the block that holds its last byte
        self.rec_block = np.searchsorted(self.start, self.rec, "right") - 1
        self.end_block = np.searchsorted(self.start, self.end - 1, "right") - 1

    def touched(self, i):
        """blocks [s, e] of record i: where it starts, where its last byte lies"""
        return int(self.rec_block[i]), int(self.end_block[i])

    def range(self, first_block, n_blocks=-1):
        """-> dict(first_block, n_own, n, records=(i0, i1), range_first, range_next, refused) for blocks [first_block, first_block +
        n_blocks) (n_blocks < 0: to the end): the records that START in them; the anchors in offsets of the file's stream (-1 where the
        rule gives none: the first record is the file's first — the header says where it starts —, a range without a record start);
        refused: its last record runs beyond the one block taken along.  n: the blocks decoded (one more than n_own unless the range
        ends with the file)."""
        nb = self.n_blocks
        fb = int(first_block)
        own = nb - fb if n_blocks < 0 else min(int(n_blocks), nb - fb)
        n = own + (1 if fb + own < nb else 0)
        i0, i1 = int(self.lo[fb]), int(self.lo[fb + own])
        r = dict(first_block=fb, n_own=own, n=n, records=(i0, i1), range_first=-1, range_next=-1, refused=False)
        if i1 > i0:
            if i0 > 0:
                r["range_first"] = int(self.rec[i0])
            r["range_next"] = int(self.end[i1 - 1])
            r["refused"] = bool(n > own and self.end[i1 - 1] > self.start[fb + n])
        return r

    def cut(self, cuts):
        """a sorted list of cut blocks -> the ranges [0, c0), [c0, c1), ..., [ck, n_blocks)"""
        edges = [0] + [int(c) for c in cuts] + [self.n_blocks]
        assert edges == sorted(edges)
        return [self.range(a, b - a) for a, b in zip(edges[:-1], edges[1:])]

    def anchors(self, ranges):
        """as distributed.check_range_anchors takes them"""
        return [(r["first_block"], r["n_own"], r["range_first"], r["range_next"]) for r in ranges]

    def ranks(self, world):
        from trueconsense_amd.distributed import block_range
        return [self.range(*block_range(self.n_blocks, r, world)) for r in range(world)]

    def sub_ranges(self, first_block, cnt, K):
        """tcmi_split_step's sub-ranges of a rank's range (csrc/split_step.cpp: at most 8, each of 64 blocks or more) -> (K taken, the
        ranges, whether they decode and join: none refused, each behind the first with a start of its own, each with an end)"""
        K = int(min(min(K, 8), max(1, cnt // 64)))
        fb = [first_block + cnt * k // K for k in range(K + 1)]
        rg = [self.range(a, b - a) for a, b in zip(fb[:-1], fb[1:])]
        ok = all(not r["refused"] and r["range_next"] >= 0 and (k == 0 or r["range_first"] >= 0) for k, r in enumerate(rg))
        return K, rg, ok

    def long_records(self, min_blocks=3):
        """indices of the records that touch at least min_blocks blocks"""
        return [int(i) for i in np.nonzero(self.end_block - self.rec_block + 1 >= min_blocks)[0]]

    def recordless_runs(self):
        """maximal runs [a, b] of blocks without a record start, the end-of-file block and header blocks left out"""
        runs, b = [], 0
        while b < self.n_blocks:
            if self.first[b] == NONE and self.entry[b] == -2 and self.ulen[b] > 0:
                a = b
                while b + 1 < self.n_blocks and self.first[b + 1] == NONE and self.ulen[b + 1] > 0:
                    b += 1
                runs.append((a, b))
            b += 1
        return runs

    def table_text(self, windows):
        """the input of `bgzf_host_main chainfile`: the block table as a decoder that is right reports it, then the windows
        (first_block, nb_own, nb, ranged)"""
        lines = ["%d" % self.n_blocks]
        lines += ["%d %d %d %d 0" % (self.entry[b], self.ulen[b], self.first[b], self.over[b]) for b in range(self.n_blocks)]
        lines.append("%d" % len(windows))
        lines += ["%d %d %d %d" % tuple(w) for w in windows]
        return "\n".join(lines) + "\n"


def model(path):
    return Model(path)


def check_conditions(brim512, htslib512, brim1024):
    """What the three files must be for the tests to reach the paths they are about, from the models alone:
    rec_vouch / rec_scan walk ceil(blocks / 1024) blocks a lane — 3 in one file, 2 in another; pk_place looks back 64 blocks a trip —
    a record over more than 128 blocks (three trips), one over 65 .. 128, one over fewer than 64; a run of record-less blocks that
    crosses a lane's stretch above block 1024; a block that starts afresh right behind a long record in the file cut as htslib cuts."""
    assert brim512.n_blocks > 2048 and htslib512.n_blocks > 2048 and 1025 <= brim1024.n_blocks <= 2048
    for m in (brim512, htslib512, brim1024):
        touch = [e - s + 1 for s, e in (m.touched(i) for i in m.long_records())]
        assert len(touch) == len(LONG), touch
        if m is not brim1024:
            assert max(touch) > 128 and any(65 <= t <= 128 for t in touch) and any(3 <= t < 64 for t in touch), touch
            per = (m.n_blocks + 1023) // 1024                       # (the file of 1024-byte blocks ends 19 blocks above 1024: its runs lie below)
            assert per == 3 and any(a > 1024 and any(b % per == 0 for b in range(a + 1, z + 1)) for a, z in m.recordless_runs())
        assert not false_finds(m)
    touch = [e - s + 1 for s, e in (brim1024.touched(i) for i in brim1024.long_records())]
    assert any(65 <= t <= 128 for t in touch) and any(3 <= t < 64 for t in touch), touch
    for i in htslib512.long_records():
        s, e = htslib512.touched(i)
        assert htslib512.rec[i] == htslib512.start[s] and htslib512.first[e + 1] == 0 and htslib512.ulen[e] < 512, (i, s, e)


def cut_lists(m, n_random=0, seed=5):
    """Cut lists (model.cut) that put cuts inside long records and ranges wholly inside one.  With [s, e] the blocks of a long record:
    a range that holds s and does not reach e - 1 is refused, so the lists that join without a refusal cut at s, e and e + 1 only."""
    se = [m.touched(i) for i in m.long_records()]
    lists = [[e for _, e in se],                                    # every range behind the first begins in the block a long record ends in
             [s for s, _ in se],                                    # ... in the block a long record starts in
             sorted([s for s, _ in se] + [e + 1 for _, e in se]),   # a long record's blocks a range of their own
             sorted([se[0][1], se[1][0], se[1][1], se[2][1] + 1, se[3][1]]),
             [(s + e) // 2 for s, e in se],                         # every range begins in the middle of a long record (and the one in front is refused)
             sorted(x for s, e in se[:2] for x in (s + 1, e - 1)),  # ranges wholly inside one record
             sorted([se[2][0] + 2, se[2][0] + 3, se[2][1]])]        # one block inside a record
    rng = np.random.default_rng(seed)
    for _ in range(n_random):
        k = int(rng.integers(1, 9))
        cuts = set(int(x) for x in rng.integers(1, m.n_blocks, k))
        for s, e in se:                                             # ... half of them with cuts at or inside the long records
            if rng.random() < 0.5:
                cuts.add(int(rng.choice([s, e, e + 1, int(rng.integers(s + 1, e))])))
        lists.append(sorted(cuts))
    return lists


def sweep_windows(m, seed=3, n_random=3):
    """for every first block: the range of one block, up to and with the next block that holds a record start, one short of that, to the
    end of the file, and a few of random lengths -> [(first_block, nb_own, nb, ranged)]"""
    rng = np.random.default_rng(seed)
    nb = m.n_blocks
    has = np.nonzero(m.first != NONE)[0]
    out = []
    for fb in range(nb):
        k = int(np.searchsorted(has, fb, "right"))
        lens = {1, nb - fb} | set(int(x) for x in rng.integers(1, nb - fb + 1, n_random))
        if k < len(has):
            lens |= {int(has[k]) - fb + 1, int(has[k]) - fb}
        for own in sorted(lens):
            out.append((fb, own, own + (1 if fb + own < nb else 0), int(not (fb == 0 and own == nb))))
    return out


# ---- the decoder's own search, restated (csrc/bgzf_copy.hip: plausible) -----------------------------------------------------------------------
def plausible(stream, c, avail, n_ref=1):
    """Could an alignment record start at offset c of the stream, judged by the `avail` bytes of it that lie in its block (40: all the
    fixed fields the search looks at)?"""
    s = bytes(stream[c:c + 40]) + bytes(40)
    bs, refid, pos, w2, w3, l_seq, nref, npos = struct.unpack_from("<IIiIIIIi", s, 0)
    l_name, n_cig = w2 & 0xFF, w3 & 0xFFFF
    need = 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
    ok = avail >= 4 and 33 <= bs < 1 << 24
    if avail >= 8:
        ok = ok and (refid + 1) & 0xFFFFFFFF <= n_ref
    if avail >= 12:
        ok = ok and pos >= -1
    if avail >= 13:
        ok = ok and l_name >= 1
    if avail >= 24:
        ok = ok and l_seq < 1 << 28 and need <= bs
    if avail >= 28:
        ok = ok and (nref + 1) & 0xFFFFFFFF <= n_ref
    if avail >= 32:
        ok = ok and npos >= -1
    return bool(ok)


def block_search(m, b, n_ref=1):
    """what block b's own search finds: the first offset at which a record can plausibly start (NONE: nowhere).  Only offsets whose
    four size bytes read as 33 <= block_size < 2^24 are looked at closely."""
    u0, u1 = int(m.start[b]), int(m.start[b + 1])
    if u1 - u0 < 4:
        return NONE
    s = m.stream[u0:u1].astype(np.uint32)
    bs = s[:-3] | (s[1:-2] << 8) | (s[2:-1] << 16) | (s[3:] << 24)
    for c in np.nonzero((bs >= 33) & (bs < 1 << 24))[0]:
        if plausible(m.stream, u0 + int(c), min(40, u1 - u0 - int(c)), n_ref):
            return int(c)
    return NONE


def predict(m, n_ref=1):
    """The whole decode restated in Python for a file whose long records may hold plausible heads by accident: every block's own
    search and its chain of size fields (bgzf_copy), rec_vouch's withdrawal of a tail find inside a record, and the host rule
    (tcmi_bam_chain_check) -> None where the file decodes (then to the model's record list), else why it is refused."""
    u32 = lambda at: int.from_bytes(bytes(m.stream[at:at + 4]), "little")
    nb = m.n_blocks
    first, over, bad = [NONE] * nb, [0] * nb, [False] * nb
    for b in range(nb):
        u0, u1 = int(m.start[b]), int(m.start[b + 1])
        if m.entry[b] == -1:
            continue
        f = int(m.entry[b]) if m.entry[b] >= 0 else block_search(m, b, n_ref)
        first[b] = f
        if f == NONE:
            continue
        at = u0 + f
        while at + 4 <= u1:                                         # the chain of size fields, as far as the block goes
            bs = u32(at)
            if not 32 <= bs <= 1 << 28:
                bad[b] = True
                break
            at += 4 + bs
        if bad[b]:
            continue
        if at < u1:                                                 # a start in the last three bytes: its size is read from the stream later
            bs = u32(at) if at + 4 <= m.inflated else 0
            over[b] = at + 4 + bs - u1 if 32 <= bs <= 1 << 28 else -1
        else:
            over[b] = at - u1
    expect = -1
    for b in range(nb):
        ulen = int(m.ulen[b])
        if m.entry[b] == -1:
            continue
        if m.entry[b] >= 0:
            expect = int(m.entry[b])
        if first[b] != NONE and first[b] != expect and m.entry[b] < 0 and expect >= ulen and first[b] + 40 > ulen:
            first[b], over[b], bad[b] = NONE, 0, False              # rec_vouch: a tail find in a block that lies inside a record
        if bad[b]:
            return "impossible block_size in block %d" % b
        if first[b] == NONE:
            if expect < ulen:
                return "no record found where one must start in block %d" % b
            expect -= ulen
            continue
        if first[b] != expect or over[b] < 0:
            return "the chain does not close at block %d (found %d, expected %d)" % (b, first[b], expect)
        expect = over[b]
    return None if expect <= 0 else "the last record runs past the file"


def build_arbitrary(tmp, seed):
    """a file of about 300 blocks of 512 bytes whose two long records carry random QUAL bytes (0 .. 93) and SEQ with N and = nibbles
    -> (path, reads, L)"""
    rng = np.random.default_rng(1000 + seed)
    specs, which = make_specs(seed=100 + seed, n_short=600, long_reads=((150, 20_000), (420, 15_000)), rng_long=rng)
    path, _, reads, L, _ = build(tmp, 512, True, name="arbitrary%d.bam" % seed, specs=specs, which=which)
    return path, reads, L


def false_finds(m):
    """blocks that look for their first record themselves (entry -2) and find something else than the model's first record start:
    [(block, found, true)] — empty for a file whose long records hold no plausible head by accident"""
    out = []
    for b in range(m.n_blocks):
        if m.entry[b] != -2:
            continue
        got, true = block_search(m, b), int(m.first[b])
        if true != NONE and m.ulen[b] - true < 4:
            true = NONE                                             # (a start in the block's last three bytes is found by the chain only)
        if got != true:
            out.append((b, got, true))
    return out
