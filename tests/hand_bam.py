"""BAM files put together outside the product's usual writer calls: the file assembled byte by byte from the SAM specification (§4.1
BGZF, §4.2 BAM) with struct.pack — two @SQ lines, aux tags of several types, a multi-op CIGAR, an unmapped tail, an extra gzip subfield
in front of BC, a stored deflate block, an empty block, and (straddle) records across block boundaries —, and a file whose header
takes several blocks.  No tests in here."""
import struct
import zlib

from trueconsense_amd import synthetic as sy
from trueconsense_amd.io import bamwriter

NT16 = "=ACMGRSVTWYHKDBN"
OPS = "MIDNSHP=XBabcdef"                           # (9-15: reserved op codes, tests/synth_small.py's letters)


def rec(tid, pos, name, flag, cigar, seq, qual, aux=b"", mapq=37, mtid=-1, mpos=-1, tlen=0):
    cg = b"".join(struct.pack("<I", (n << 4) | OPS.index(op)) for n, op in cigar)
    l = len(seq)
    codes = [NT16.index(c) for c in seq] + ([0] if l & 1 else [])
    sq = bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2))
    nm = name.encode() + b"\0"
    body = struct.pack("<iiBBHHHIiii", tid, pos, len(nm), mapq, 4680, len(cigar), flag, l, mtid, mpos, tlen) + nm + cg + sq + bytes(qual) + aux
    return struct.pack("<i", len(body)) + body


def bgzf(data, level=6, extra_subfield=False, stored=False):
    if stored:
        body = b"\x01" + struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data      # BFINAL=1, BTYPE=00
    else:
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        body = co.compress(data) + co.flush()
    xtra = (b"XY" + struct.pack("<H", 3) + b"abc" if extra_subfield else b"")            # another subfield in front of BC
    xlen = len(xtra) + 6
    bsize = 12 + xlen + len(body) + 8
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", xlen) + xtra + b"BC\x02\x00" + struct.pack("<H", bsize - 1) +
            body + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def build(path, straddle):
    text = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chrA\tLN:500\n@SQ\tSN:chrB\tLN:300\n@PG\tID:hand\n".encode()
    head = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 2)
    for name, ln in (("chrA", 500), ("chrB", 300)):
        nb = name.encode() + b"\0"
        head += struct.pack("<i", len(nb)) + nb + struct.pack("<i", ln)
    aux = b"NMC\x02" + b"MDZ10A5\0" + b"ASs" + struct.pack("<h", -7) + b"XBBi" + struct.pack("<ii", 2, 11) + struct.pack("<i", -3)
    reads = [
        rec(0, 3, "r1", 0, [(20, "M")], "ACGTACGTACGTACGTACGT", [30] * 20, aux),
        rec(0, 3, "read_with_a_longer_name/1", 99, [(2, "S"), (8, "M"), (2, "I"), (6, "M"), (3, "D"), (5, "M"), (1, "H")],
            "NNACGTACGTGGACGTACCCCCC"[:23], list(range(10, 33)), b"", mtid=0, mpos=40, tlen=80),
        rec(0, 10, "r3", 16, [(5, "="), (1, "X"), (9, "M")], "ACGTAGACGTNRACG", [2] * 15, b"RGZgrp\0"),
        rec(0, 40, "read_with_a_longer_name/1", 147, [(15, "M")], "TTTTTGGGGGCCCCC", [40] * 15, b"", mtid=0, mpos=3, tlen=-80),
        rec(0, 100, "skip", 0, [(4, "M"), (50, "N"), (4, "M")], "ACGTACGT", [25] * 8),
        rec(0, 480, "past_the_end", 0, [(30, "M")], "ACGTAC" * 5, [20] * 30),
        rec(0, 120, "placed_unmapped", 4 | 1 | 64, [], "ACGT", [9] * 4, mtid=0, mpos=120),
        rec(-1, -1, "u1", 4, [], "ACGTN", [1, 2, 3, 4, 5]),
        rec(-1, -1, "u2_no_seq", 4, [], "", []),
    ]
    # sort order of a coordinate-sorted BAM: (tid, pos), unplaced last
    order = [0, 1, 2, 3, 4, 6, 5, 7, 8]
    reads = [reads[i] for i in order]
    with open(path, "wb") as fh:
        fh.write(bgzf(head, extra_subfield=True))
        if not straddle:
            fh.write(bgzf(b"".join(reads[:2]), level=9))
            fh.write(bgzf(b""))                                     # an empty block between two data blocks
            fh.write(bgzf(b"".join(reads[2:5]), stored=True))       # deflate "stored" block
            fh.write(bgzf(b"".join(reads[5:]), level=1, extra_subfield=True))
        else:
            blob = b"".join(reads)
            cuts = [0, 37, 38, 120, 121, 300, len(blob)]            # through block_size fields and record bodies
            for a, b in zip(cuts[:-1], cuts[1:]):
                fh.write(bgzf(blob[a:b], level=6))
        fh.write(EOF_BLOCK)
    return order


def small_reads(n=400, seed=3):
    ref, _ = sy.make_reference()
    return sy.make_reads(ref[:3000], n, seed=seed, indel_sites=None)


def long_header_bam(path):
    """A header of several blocks (300 @SQ with long names, block = 700) whose first record starts in the middle of a block."""
    refs = [("contig_%04d_with_a_rather_long_name_as_assemblies_have_them" % k, 1000 + k) for k in range(300)]
    refs[0] = (refs[0][0], 3000)
    bamwriter.write_bam(path, small_reads(), block=700, split_records=True, refs=refs)
    return refs
