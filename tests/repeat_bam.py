"""A BAM file with every record of another one repeated R times in place (r0 x R, r1 x R, ...: still coordinate-sorted), for the tests
that need more records than a capped grid takes in one trip (tests/test_stream_scale.py): every count the device gives for such a file
is exactly R times the count of the small file, which the committed yardsticks can afford.  Python's zlib inflates the source (BGZF is
concatenated gzip members), trueconsense_amd.io.bamwriter._bgzf_block compresses the result; repeated records compress to under 2 %
of their size, so 80 MB of them are written in well under a second.  No GPU, no tests in here (tests/test_repeat_bam.py)."""
import os
import re
import struct
import zlib

from tests.cli_run import ROOT
from trueconsense_amd.io import bamwriter

BLOCK = 0xFF00
CSRC = os.path.join(ROOT, "trueconsense_amd", "csrc")
MASK_LONG_GRID, MASK_LONG_BLOCK = 64, 256                                       # pk_mask_long's launch: tests/test_stream_scale.py's file B


def stream_count_caps():
    """-> (SC_BLOCK, SC_WG_PER_CU) as csrc/stream_count.h states them; the counting kernels' grid is min(ceil(records / SC_BLOCK),
    compute units * SC_WG_PER_CU)"""
    text = open(os.path.join(CSRC, "stream_count.h")).read()
    block, per_cu = (re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text) for name in ("SC_BLOCK", "SC_WG_PER_CU"))
    assert block and per_cu, "csrc/stream_count.h no longer states SC_BLOCK and SC_WG_PER_CU as constexpr int"
    return int(block.group(1)), int(per_cu.group(1))


def inflate(path):
    """the inflated stream of a BGZF file, member by member"""
    with open(path, "rb") as fh:
        data = fh.read()
    out = []
    while data:
        d = zlib.decompressobj(31)
        out.append(d.decompress(data))
        assert d.eof, "a truncated gzip member in %s" % path
        data = d.unused_data
    return b"".join(out)


def block_sizes(path):
    """the inflated size of every BGZF block of a file, the end-of-file block (0) included"""
    with open(path, "rb") as fh:
        data = fh.read()
    sizes, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 12:at + 14] == b"BC", "no BGZF block at offset %d of %s" % (at, path)
        at += struct.unpack_from("<H", data, at + 16)[0] + 1
        sizes.append(struct.unpack_from("<I", data, at - 4)[0])
    return sizes


def n_blocks(path):
    return len(block_sizes(path))


def split(stream):
    """an inflated BAM stream -> (the header's bytes, [every record with its length prefix])"""
    assert stream[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", stream, 4)
    at = 8 + l_text
    n_ref, = struct.unpack_from("<i", stream, at)
    at += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", stream, at)
        at += 4 + l_name + 4
    header, records = stream[:at], []
    while at < len(stream):
        size, = struct.unpack_from("<i", stream, at)
        assert size >= 32 and at + 4 + size <= len(stream), "a record that overruns the stream at offset %d" % at
        records.append(stream[at:at + 4 + size])
        at += 4 + size
    return header, records


def repeat_records(src, dst, times, keep=None, level=1, brim=False):
    """Write `dst` with the header of `src` and every record of it `times` times in place -> the number of records written.
    keep: which records of `src` are repeated, the others are left out — a collection of record indices, or a predicate over
    (index, the record's bytes behind its length prefix); None: all.
    Blocks are cut as bamwriter.write_bam cuts them: the header gets blocks of its own and a record that does not fit into the current
    block starts the next one (only a record larger than a block spans several); brim=True fills every block to 0xFF00 bytes instead,
    so records straddle blocks."""
    header, records = split(inflate(src))
    if keep is None:
        chosen = records
    elif callable(keep):
        chosen = [r for i, r in enumerate(records) if keep(i, r[4:])]
    else:
        want = set(int(i) for i in keep)
        assert all(0 <= i < len(records) for i in want), "keep names a record the file does not hold"
        chosen = [r for i, r in enumerate(records) if i in want]
    with open(dst, "wb") as fh:
        def put(data):
            for o in range(0, len(data), BLOCK):
                fh.write(bamwriter._bgzf_block(bytes(data[o:o + BLOCK]), level))
        if brim:
            put(header + b"".join(r * times for r in chosen))
        else:
            put(header)
            out = bytearray()
            for r in chosen:
                left = times
                while left:
                    fit = (BLOCK - len(out)) // len(r)
                    if fit == 0 and out:
                        put(out)
                        out = bytearray()
                        continue
                    take = min(max(fit, 1), left)       # (fit == 0 on an empty block: a record larger than a block, on its own)
                    out += r * take
                    left -= take
                    if len(out) >= BLOCK:
                        put(out)
                        out = bytearray()
            put(out)
        fh.write(bamwriter._EOF)
    return len(chosen) * times
