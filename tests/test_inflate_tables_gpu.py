"""GPU: the device decoder's Huffman tables (csrc/bgzf_device.h: build_table; csrc/huffman_rule.h) on headers that sit on the edges of how
they are built — the rank's groups of 64 symbols, the 16-entry table of counts, offsets and limits, the slots' count of limits, the long
codes moved down in place.  Every file is a BAM of four reads in ONE data block of about 3 KB (the block in front holds the BAM header,
which the host inflates): a deflate block of plain literals, then the deflate block the case is about, written over the first read's
quality bytes (free bytes) with tests/deflate_writer.py, then plain literals again.  The device's stream is held against the bytes that
were written, byte for byte, and its record starts against a walk of them; where the code is complete zlib's inflate is asked too (it
refuses incomplete literal/length codes, the device accepts them: DESIGN §5.1).  tests/test_huffman_rule.py checks the rule on the CPU."""
import gzip
import os
import struct

import numpy as np
import pytest

from tests import deflate_writer as dw
from tests import foreign_files as ff
from trueconsense_amd import _ffi, _state, engine

pytestmark = pytest.mark.gpu

D4 = [2, 2, 2, 2]                                                       # distances 1 .. 4, a complete code
EDGE_BYTES = [63, 64, 127, 128, 255, 0, 62, 65, 126, 129, 191, 192, 254]       # symbols on both sides of every group of 64
# one code of every length 1 .. 13, one of 14 and two of 15 bits: complete; the symbols lie in all five groups of the rank
ALL_LENGTHS = dict(zip([0, 63, 64, 65, 127, 128, 129, 191, 192, 255, 256, 257, 258, 285, 1, 2], list(range(1, 15)) + [15, 15]))
# 226 codes of 8 bits, then 60 of 9 on the literals 196 .. 255: literal 255 has the last code, nine ones
LAST_IS_255 = list(range(256, 286)) + list(range(256))


def lits(*values):
    return [("lit", v) for v in values]


def edge_tokens():
    return lits(*EDGE_BYTES) * 3 + [("match", 3, 1), ("match", 4, 2)] + lits(*EDGE_BYTES[::-1]) + [("match", 258, 3), ("match", 3, 4)] + lits(255, 0, 63, 64)


def case_edges():
    return dw.flat(286, list(range(286))), D4, edge_tokens()


def case_all_lengths():
    ll = [ALL_LENGTHS.get(s, 0) for s in range(286)]
    assert dw.kraft(ll) == 32768 and sorted(set(ll)) == list(range(16))
    toks = []
    for s in sorted(ALL_LENGTHS, key=ALL_LENGTHS.get, reverse=True):    # the longest codes first, every coded symbol at least once
        toks += lits(s) if s < 256 else [("match", {257: 3, 258: 4, 285: 258}[s], 1 + s % 4)] if s > 256 else []
    return ll, D4, lits(0, 63, 64, 65) + toks + lits(2, 1, 255, 192) + [t for t in toks[::-1] if t[:2] != ("match", 258)]


def case_no_root_entry():
    ll = [10 + s % 3 for s in range(286)]                               # 10 .. 12 bits: not one slot of the 9-bit root table is filled
    assert dw.kraft(ll) < 32768
    return ll, D4, edge_tokens()


def case_all_nine():
    return [9] * 286, D4, edge_tokens()                                 # 286 of 512 codes: incomplete, every slot a 9-bit code or none


def case_one_distance():
    return dw.flat(286, list(range(286))), [1], lits(*EDGE_BYTES) + [("match", 5, 1), ("match", 3, 1)] + lits(7, 7, 9) + [("match", 258, 1)]


def case_incomplete():
    ll = dw.flat(286, LAST_IS_255)
    assert ll[255] == 9 and dw.canonical(ll)[255] == (0x1FF, 9)
    ll[255] = 0                                                         # its code stays unused
    return ll, D4, [t for t in edge_tokens() if t != ("lit", 255)]


CASES = {"edges": case_edges, "all-lengths": case_all_lengths, "no-root-entry": case_no_root_entry, "all-nine": case_all_nine,
         "one-distance": case_one_distance, "incomplete": case_incomplete, "fixed": lambda: (None, None, edge_tokens())}
COMPLETE = {"edges", "all-lengths", "one-distance", "fixed"}            # what zlib's inflate accepts


def write_block(bw, tokens, ll, d, final, stray=None):
    """one deflate block by hand (ll None: fixed codes); stray: a code written in front of the end-of-block code"""
    bw.bits(final, 1)
    bw.bits(1 if ll is None else 2, 2)
    if ll is None:
        ll, d = dw.FIXED_LL, dw.FIXED_D
    else:
        dw.dynamic_header(bw, ll, d)
    lc, dc = dw.canonical(ll), dw.canonical(d)
    for t in tokens:
        if t[0] == "lit":
            bw.bits(*lc[t[1]])
        else:
            ls, leb, lev = dw.len_symbol(t[1])
            ds, deb, dev = dw.dist_symbol(t[2])
            bw.bits(*lc[ls])
            bw.bits(lev, leb)
            bw.bits(*dc[ds])
            bw.bits(dev, deb)
    if stray:
        bw.bits(*stray)
    bw.bits(*lc[256])


def plain_block(bw, data, final):
    toks = lits(*data)
    ll, d = dw.lengths_for(toks, d="none")
    write_block(bw, toks, ll, d, final)


def build(tmp, name, stray=None):
    """-> (path, the inflated stream as written, its record starts)"""
    ll, d, tokens = CASES[name]()
    stream, fields = ff.source_stream(0.5, 4)
    head = 12 + int.from_bytes(stream[4:8], "little")
    head += 8 + int.from_bytes(stream[head:head + 4], "little")
    q0 = fields[0][0]
    seg = bytearray(stream[:q0])
    dw.token_bytes(tokens, seg)
    seg = seg[q0:]
    assert len(seg) <= fields[0][1], len(seg)
    stream[q0:q0 + len(seg)] = seg
    data = bytes(stream[head:])
    bw = dw.BitWriter()
    plain_block(bw, data[:q0 - head], 0)
    write_block(bw, tokens, ll, d, 0, stray)
    plain_block(bw, data[q0 - head + len(seg):], 1)
    bw.align()
    payload = bytes(bw.out)
    assert len(payload) <= 4000, len(payload)                           # two blocks per workgroup: the bench file's kernel
    path = os.path.join(str(tmp), name + (".stray" if stray else "") + ".bam")
    with open(path, "wb") as fh:
        fh.write(dw.bgzf(dw.plain_recipe(65000)(bytes(stream[:head]), 0)[0], bytes(stream[:head])))
        fh.write(dw.bgzf(payload, data))
        fh.write(dw.EOF_BLOCK)
    rec, o = [], head
    while o < len(stream):
        rec.append(o)
        o += 4 + struct.unpack_from("<i", stream, o)[0]
    assert o == len(stream) and len(rec) == 4
    return path, np.frombuffer(bytes(stream), np.uint8), np.array(rec, np.uint64)


@pytest.fixture(scope="module")
def ctx():
    return _state.default_context()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp, made = tmp_path_factory.mktemp("tables"), {}

    def get(name):
        if name not in made:
            made[name] = build(tmp, name)
            if name in COMPLETE:                                        # the writer wrote what it meant to
                assert gzip.decompress(open(made[name][0], "rb").read()) == made[name][1].tobytes(), name
        return made[name]
    return get


def check(ctx, path, want_stream, want_rec):
    d = engine.DeviceBam(path)
    try:
        assert d.inflated_bytes == len(want_stream)
        stream, rec = d.decode_to_host(ctx)
        assert np.array_equal(stream, want_stream), np.argwhere(stream != want_stream)[:5]
        assert np.array_equal(rec, want_rec), (rec, want_rec)
    finally:
        d.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_headers_on_the_edges_of_the_table_builder(ctx, files, name):
    check(ctx, *files(name))


@pytest.mark.parametrize("name", ["all-lengths", "edges", "no-root-entry"])
def test_pass_b_reads_the_same_tables(ctx, files, name):
    """lanes that overflow their scratch send the block through pass B's C++ decoder: root tables, long-code tables and limits as the
    rounds of pass A read them"""
    ctx.set_option("sym_scratch_div", 64)
    try:
        check(ctx, *files(name))
    finally:
        ctx.set_option("sym_scratch_div", 1)


def test_the_unused_code_of_an_incomplete_code_is_refused_when_sent(ctx, tmp_path):
    path, _, _ = build(tmp_path, "incomplete", stray=(0x1FF, 9))
    d = engine.DeviceBam(path)
    try:
        with pytest.raises(_ffi.TcmiError) as e:
            ctx.upload_bamfile(d)
        assert e.value.code == _ffi.E_FORMAT and "block 1" in str(e.value), str(e.value)
        with pytest.raises(_ffi.TcmiError) as e:
            d.decode_to_host(ctx)
        assert e.value.code == _ffi.E_FORMAT, str(e.value)
    finally:
        d.close()
