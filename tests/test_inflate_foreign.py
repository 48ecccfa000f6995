"""GPU: the device inflate (bgzf_symbols + bgzf_copy) on deflate streams that zlib's deflate never writes — what htslib with libdeflate,
igzip and vendor pipelines may: distances up to 32 768 and length-3 matches far back, codes of 15 bits and the 48-bit symbol, odd code
shapes and headers, stored and Huffman blocks mixed at any bit alignment.  The files come from tests/foreign_files.py (made with
tests/deflate_writer.py; tests/test_deflate_writer.py shows on the CPU that zlib's inflate accepts them); every case proves from the
writer's log that it hits the decoder line it is aimed at, then: the stream byte for byte against zlib's inflate and the record index
(check_decode), the counts against the oracle (check_counts).  Exact equality throughout.
Every group is written at three BGZF block sizes, one per symbol decoder (the file's largest payload decides: "-A" two blocks a workgroup,
"-B" one block with two-literal tokens, "-C" windowed); bgzf_copy's variant follows the file's ratio (12 : 1, 4 : 1): both asserted.
Streams that must be REFUSED (tests/refused_streams.py, each with the decoder line that refuses it) end in E_FORMAT."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import c_oracle
from tests import foreign_files as ff
from tests import refused_streams as rf
from tests.device_file import check_counts, check_decode
from trueconsense_amd import _ffi, _state, engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return _state.default_context()


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """the files, built once each"""
    tmp, made = tmp_path_factory.mktemp("foreign"), {}

    def get(name):
        if name not in made:
            made[name] = ff.build(tmp, name)
            ff.prove(made[name])
        return made[name]
    return get


def check_file(ctx, c):
    d = check_decode(ctx, c.path)
    pay = max((((g["cin"] & 3) * 8 + g["clen"] * 8 + 31) // 32 + 6) * 4 for g in c.logs)       # (bgzf_host.cpp:62 -> bgzf_symbols.hip:985-994)
    assert ("two blocks" if pay <= 4096 else "one block" if pay <= 16384 else "windowed") == ff.VARIANT[c.name[-1]], pay
    assert (d.inflated_bytes >= 12 * d.file_bytes) == (c.name in ff.ABOVE_12)                   # bgzf_copy<false, false> (if "-A") or <true, false>
    assert (d.inflated_bytes < 4 * d.file_bytes) == (c.name in ff.BELOW_4)                      # bgzf_copy<true, true>
    d.close()
    check_counts(ctx, c.path, ff.REF_LEN)


@pytest.mark.parametrize("name", ff.NAMES)
def test_streams_zlib_never_writes(ctx, cases, name):
    check_file(ctx, cases(name))


@pytest.mark.parametrize("name", ff.SUBSET)
def test_pass_b_cuts_them_into_the_same_tokens(ctx, cases, name):
    """lanes that overflow their scratch send the block through pass B's C++ decoder (bgzf_symbols.hip:767-803, :945-955): 48-bit
    symbols, long codes and two-literal tokens must come out as from the hand-scheduled rounds"""
    ctx.set_option("sym_scratch_div", 64)
    try:
        check_file(ctx, cases(name))
    finally:
        ctx.set_option("sym_scratch_div", 1)


@pytest.mark.timeout(300)
def test_small_windows_end_inside_their_symbols_headers_and_stored_blocks(tmp_path):
    """bgzf_symbols<1, true> with a window of 2 KB (read once per process: a child): window ends fall inside 48-bit symbols, dynamic
    headers of 316 code lengths and stored blocks"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys\n"
            "from tests import foreign_files as ff, test_inflate_foreign as t\n"
            "from trueconsense_amd import _state\n"
            "ctx = _state.default_context()\n"
            "for name in ff.SUBSET:\n"
            "    c = ff.build(sys.argv[1], name)\n"
            "    ff.prove(c)\n"
            "    t.check_file(ctx, c)\n"
            "print('windowed ok')\n")
    env = dict(os.environ, TCMI_SYM_WINDOW="2048", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path)], cwd=root, env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0 and "windowed ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("name", list(ff.FAR))
def test_far_matches_in_block_ranges(ctx, cases, name):
    """a range of the file's blocks re-bases the block table (uout, tok): matches that reach back 32 768 bytes must not care"""
    c = cases(name)
    want = c_oracle.tally(c_oracle.read_bam(c.path), ff.REF_LEN)
    try:
        for one_sync in (1, 0):
            ctx.set_option("one_sync", one_sync)
            d = engine.DeviceBam(c.path)
            nb = d.n_blocks
            acc = np.zeros_like(want, dtype=np.int64)
            for first, count in ((0, nb // 2), (nb // 2, nb - nb // 2)):
                rs = ctx.upload_bamfile(d, blocks=(first, count))
                acc += ctx.step(rs, ff.REF_LEN, 30, True)[3]
                rs.free()
            d.close()
            assert np.array_equal(acc, want), (one_sync, np.argwhere(acc != want)[:5])
    finally:
        ctx.set_option("one_sync", 1)


@pytest.mark.parametrize("name", sorted(rf.REFUSED))
def test_streams_that_must_be_refused(ctx, tmp_path, name):
    """one damaged member in block 0, in the first block behind the header's and in a middle block (tests/refused_streams.py says which
    line of the decoder refuses each): E_FORMAT from the upload and from the whole-file decode — never a stream"""
    for where in rf.WHERE:
        path, k, _ = rf.build(tmp_path, name, where)
        try:
            d = engine.DeviceBam(path)
        except _ffi.TcmiError as e:                 # block 0 holds the BAM header: the host inflates it, and refuses
            assert where == "zero" and e.code == _ffi.E_FORMAT, (where, e)
            continue
        assert where != "zero"
        with pytest.raises(_ffi.TcmiError) as e:
            ctx.upload_bamfile(d)
        assert e.value.code == _ffi.E_FORMAT and ("block %d" % k) in str(e.value), (where, str(e.value))
        with pytest.raises(_ffi.TcmiError) as e:
            d.decode_to_host(ctx)
        assert e.value.code == _ffi.E_FORMAT, (where, str(e.value))
        d.close()
