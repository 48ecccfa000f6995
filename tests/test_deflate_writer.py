"""CPU: the tests' own deflate writer (tests/deflate_writer.py) and every file that tests/test_inflate_foreign.py feeds the device decoder
(tests/foreign_files.py).  zlib's INFLATE is the reference — it accepts what zlib's deflate never writes —: every member of every file
inflates to the source stream, both host readers read the same reads from it as from the source file, and the file hits what it is for:
the condition of the decoder line it is aimed at, read from the writer's log (foreign_files.prove)."""
import gzip
import zlib

import numpy as np
import pytest

from oracle import c_oracle
from tests import deflate_writer as dw
from tests import foreign_files as ff
from tests import refused_streams as rf
from trueconsense_amd import engine


def test_canonical_codes_and_the_makers():
    assert dw.canonical([3, 3, 3, 3, 3, 2, 4, 4]) == [(0b010, 3), (0b110, 3), (0b001, 3), (0b101, 3), (0b011, 3), (0b00, 2), (0b0111, 4), (0b1111, 4)]   # RFC 1951 3.2.2, reversed
    assert dw.canonical(dw.FIXED_LL)[0] == (0b00001100, 8) and dw.canonical(dw.FIXED_LL)[256] == (0, 7) and dw.canonical(dw.FIXED_LL)[280] == (0b00000011, 8)
    assert dw.len_symbol(3) == (257, 0, 0) and dw.len_symbol(257) == (284, 5, 30) and dw.len_symbol(258) == (285, 0, 0) and dw.len_symbol(131) == (281, 5, 0)
    assert dw.dist_symbol(1) == (0, 0, 0) and dw.dist_symbol(32768) == (29, 13, 8191) and dw.dist_symbol(16385) == (28, 13, 0) and dw.dist_symbol(5) == (4, 1, 0)
    for n, maker in ((286, dw.deep), (30, dw.deep), (286, dw.flat), (257, dw.flat)):
        order = list(np.random.default_rng(n).permutation(n))
        lens = maker(n, order)
        assert dw.kraft(lens) == 32768 and all(lens) and lens[order[-1]] == max(lens)
    assert sorted(set(dw.flat(286, list(range(286))))) == [8, 9]
    lens = dw.deep(286, list(range(286)))
    assert lens[:6] == [1, 2, 3, 4, 5, 6] and set(lens[6:]) == {14, 15}
    lens = dw.huffman([1 << k for k in range(40)])              # a Fibonacci-like tree, held to 15 bits
    assert max(lens) == 15 and dw.kraft(lens) == 32768
    assert dw.huffman([0, 7, 0]) == [0, 1, 0]


def test_the_code_length_encodings():
    seq = [0] * 140 + [5] * 8 + [0, 0] + [7, 7, 7]
    assert dw.code_length_symbols(seq, "none", 145) == [(v, 0, 0) for v in seq]
    greedy = dw.code_length_symbols(seq, "greedy", 145)         # the run of fives is cut at HLIT
    assert greedy == [(18, 7, 127), (0, 0, 0), (0, 0, 0), (5, 0, 0), (16, 2, 1), (5, 0, 0), (5, 0, 0), (5, 0, 0), (0, 0, 0), (0, 0, 0), (7, 0, 0), (7, 0, 0), (7, 0, 0)]
    assert dw.code_length_symbols(seq, "max", 145)[:5] == [(18, 7, 127), (0, 0, 0), (0, 0, 0), (5, 0, 0), (16, 2, 3)]


@pytest.mark.parametrize("policy", ["nearest", "farthest", "literals"])
def test_streams_of_every_kind_inflate_with_zlib(policy):
    rng = np.random.default_rng(5)
    piece = rng.integers(0, 42, 1500).astype(np.uint8).tobytes()
    data = (piece * 30)[:40000] + rng.integers(0, 255, 3000).astype(np.uint8).tobytes() + b"\x07" * 700
    plan = [(39000, 258, 32768), (39300, 3, 32768), (43100, 258, 1)] if policy != "nearest" else []
    for o, l, d in plan[:2]:
        data = data[:o] + data[o - d:o - d + l] + data[o + l:]
    tokens = dw.tokenize(data, policy, plan)
    assert all(("match", l, d) in tokens for _, l, d in plan)
    n = len(tokens)
    ll, d = dw.lengths_for(tokens, "deep", "deep")
    ll2, d2 = dw.lengths_for(tokens[2 * (n // 4):], "flat", "huffman")
    for blocks in ([dict(kind="dynamic", n=n, ll=ll, d=d)], [dict(kind="fixed", n=n)], [dict(kind="stored", n=n // 4), dict(kind="stored", n=n - n // 4)],
                   [dict(kind="fixed", n=n // 4), dict(kind="stored", n=0), dict(kind="stored", n=n // 4), dict(kind="fixed", n=0),
                    dict(kind="dynamic", n=n - 2 * (n // 4), ll=ll2, d=d2, clenc="none", hclen=19), dict(kind="stored", n=0)]):
        payload, log = dw.encode(tokens, blocks)
        assert zlib.decompress(payload, -15) == data == log["data"]
        if len(payload) + 26 <= 65536:                              # (literals of 15 bits: more than a BGZF block holds)
            assert gzip.decompress(dw.bgzf(payload, data)) == data


@pytest.mark.parametrize("name", ff.NAMES)
def test_every_foreign_file_is_valid_and_hits_what_it_is_for(name, tmp_path):
    c = ff.build(tmp_path, name)
    want = gzip.decompress(open(c.src_path, "rb").read())
    assert gzip.decompress(open(c.path, "rb").read()) == want           # zlib's inflate accepts every member
    assert sum(g["ulen"] for g in c.logs) == len(want) <= 1 << 20
    ff.prove(c)
    assert (c.ratio >= 12) == (name in ff.ABOVE_12) and (c.ratio < 4) == (name in ff.BELOW_4), c.ratio
    a, b = engine.BamFile(c.path), engine.BamFile(c.src_path)           # the host reader
    assert a.n_reads == b.n_reads > 0 and a.inflated_bytes == len(want)
    ra, rb = a.arrays(), b.arrays()
    for key in ("pos", "flag", "l_qseq", "cigar_off", "cigar", "seq_off", "seq", "qual", "name_off", "names"):
        assert np.array_equal(ra[key], rb[key]), key
    oa, ob = c_oracle.read_bam(c.path), c_oracle.read_bam(c.src_path)   # the oracle's reader
    for key in ("pos", "flag", "l_qseq", "cigar", "seq", "qual"):
        assert np.array_equal(oa[key], ob[key]) and np.array_equal(oa[key], ra[key][:len(oa[key])]), key


@pytest.mark.parametrize("name", sorted(rf.REFUSED))
def test_zlib_refuses_the_streams_that_must_be_refused(name, tmp_path):
    """... and inflates the members around them: the damage is where the case says and nowhere else."""
    for where in rf.WHERE:
        path, k, n_blocks = rf.build(tmp_path, name, where)
        raw = open(path, "rb").read()
        offs, o = [], 0
        while o < len(raw):
            offs.append(o)
            o += int.from_bytes(raw[o + 16:o + 18], "little") + 1
        assert len(offs) == n_blocks + 1 and k == {"zero": 0, "first": 1}.get(where, n_blocks // 2) < n_blocks - 1
        for j, o in enumerate(offs[:-1]):
            member = raw[o:offs[j + 1]]
            if j != k:
                gzip.decompress(member)
                continue
            isize = int.from_bytes(member[-4:], "little")
            z = zlib.decompressobj(-15)
            try:
                got = z.decompress(member[18:-8])
                ok = z.eof and not z.unused_data and len(got) == isize
            except zlib.error:
                ok = False
            assert not ok, "zlib inflates this member to ISIZE bytes"
        with pytest.raises(engine._ffi.TcmiError):                      # the host reader refuses the file, too
            engine.BamFile(path)
