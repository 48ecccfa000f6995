"""CPU: the host parser of the container format (csrc/bgzf_host.h, bgzf_host.cpp: the BGZF block walk, a member's inflate, the BAM
header, the record-chain rule) in a program of its own — tests/bgzf_host_main.cpp, built here with AddressSanitizer + UBSan and run
as a child process — against a restatement of the format in this file (struct + zlib), on intact files and on damaged ones: the same
verdict, the same tables, and no report from either sanitizer (a report ends the program with a non-zero status)."""
import struct
import zlib

import numpy as np
import pytest

from tests import hand_bam as hand
from tests import host_program
from tests.hand_bam import EOF_BLOCK, long_header_bam, small_reads
from trueconsense_amd import synthetic as sy
from trueconsense_amd.io import bamwriter

E_FORMAT = -5


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return host_program.build(["tests/bgzf_host_main.cpp", "trueconsense_amd/csrc/bgzf_host.cpp"], tmp_path_factory.mktemp("bgzf_host") / "bgzf_host_main", libs=["-lz"])


def run(prog, *args):
    return host_program.run(prog, *args).stdout


def split_output(text):
    """{path: lines} of a `table` / `damaged` run"""
    files, cur = {}, None
    for line in text.split("\n"):
        if line.startswith("file "):
            cur = files.setdefault(line[5:], [])
        elif line and not line.startswith("damaged:"):
            cur.append(line)
    return files


# ---- the restatement: SAM spec §4.1 (a BGZF block is a gzip member with a BC extra subfield), §4.2 (the BAM header) --------------------
def restate(data):
    """The lines the program must print for these bytes."""
    n, off, uout, blocks = len(data), 0, 0, []
    u16 = lambda at: struct.unpack_from("<H", data, at)[0]
    u32 = lambda at: struct.unpack_from("<I", data, at)[0]
    refuse = lambda at: ["refused %d %d" % (E_FORMAT, at)]
    while off < n:
        if n - off < 18:
            return refuse(off)
        if data[off:off + 3] != b"\x1f\x8b\x08" or not data[off + 3] & 4:
            return refuse(off)
        xlen = u16(off + 10)
        if n - off < 12 + xlen:
            return refuse(off)
        bsize, x = 0, 0
        while x + 4 <= xlen:                                          # the extra subfields: SI1 SI2 SLEN data
            slen = u16(off + 12 + x + 2)
            if data[off + 12 + x:off + 12 + x + 2] == b"BC" and slen == 2 and x + 6 <= xlen:
                bsize = u16(off + 12 + x + 4) + 1
            x += 4 + slen
        if bsize < 12 + xlen + 8 or n - off < bsize:
            return refuse(off)
        crc, ulen = u32(off + bsize - 8), u32(off + bsize - 4)
        if ulen > 65536:
            return refuse(off)
        blocks.append(dict(cin=off + 12 + xlen, clen=bsize - 12 - xlen - 8, ulen=ulen, uout=uout, crc=crc))
        uout += ulen
        off += bsize

    def inflate(b):                                                 # the block's bytes, or None: no deflate stream of exactly ulen bytes
        if b["ulen"] == 0:
            return b""
        d = zlib.decompressobj(-15)
        try:
            got = d.decompress(data[b["cin"]:b["cin"] + b["clen"]], b["ulen"] + 1)
        except zlib.error:
            return None
        return got if d.eof and len(got) == b["ulen"] else None

    # the header, from as many leading blocks as it occupies (their CRC-32 is not looked at)
    head, nb = bytearray(), 0

    def need(k):
        nonlocal nb
        while len(head) < k:
            if nb >= len(blocks):
                return False
            got = inflate(blocks[nb])
            if got is None:
                return False
            head.extend(got)
            nb += 1
        return True

    if not need(12) or head[:4] != b"BAM\1":
        return refuse(0)
    l_text = struct.unpack_from("<I", head, 4)[0]
    if not need(12 + l_text):
        return refuse(8)
    text = bytes(head[8:8 + l_text])
    o = 8 + l_text
    n_ref = struct.unpack_from("<I", head, o)[0]
    o += 4
    refs = []
    for _ in range(n_ref):
        if not need(o + 4):
            return refuse(o)
        l_name = struct.unpack_from("<I", head, o)[0]
        o += 4
        if not need(o + l_name + 4):
            return refuse(o)
        refs.append((struct.unpack_from("<I", head, o + l_name)[0], bytes(head[o:o + max(l_name - 1, 0)])))
        o += l_name + 4
    # where the first record starts: blocks in front of it are header only (-1), its block knows the offset, the others (-2) look for theirs
    before, hit = 0, False
    for b in blocks:
        if not hit and o >= before + b["ulen"]:
            b["entry"] = -1
            before += b["ulen"]
        elif not hit:
            b["entry"] = o - before
            hit = True
        else:
            b["entry"] = -2
    # the records behind the header in what was inflated for it: their mean size, from 16 on
    at, cnt = o, 0
    while at + 4 <= len(head):
        bs = struct.unpack_from("<I", head, at)[0]
        if bs < 32 or bs > 1 << 24 or at + 4 + bs > len(head):
            break
        at += 4 + bs
        cnt += 1
    hint = (at - o) // cnt if cnt >= 16 else 0
    # the decoder's token accounting per block (csrc/bgzf_device.h: a token per literal / match, as many again of scratch)
    tok_total = pay = 0
    for b in blocks:
        tok_total += (2 * (min(b["ulen"], 8 * b["clen"]) + b["clen"] // 2 + 8) + 3) & ~3
        pay = max(pay, ((b["cin"] & 3) * 8 + b["clen"] * 8 + 31) // 32 + 6)
    lines = ["parsed %d %d %d %d %d %d %d" % (len(blocks), uout, o, len(refs), hint, tok_total, pay)]
    all_ok = True
    for b in blocks:
        got = inflate(b)
        ok = got is not None and (b["ulen"] == 0 or zlib.crc32(got) & 0xFFFFFFFF == b["crc"])
        all_ok = all_ok and ok
        lines.append("block %d %d %d %d %d %d %d" % (b["cin"], b["clen"], b["ulen"], b["uout"], b["crc"], b["entry"], ok))
    lines.append("text " + text.hex())
    lines += ["ref %d %s" % (ln, name.hex()) for ln, name in refs]
    if all_ok:
        lines.append("whole %d" % o)
    return lines


def compare(prog, mode, paths):
    out = run(prog, mode, *paths)
    got = split_output(out)
    assert len(got) == len(paths)
    verdicts = []
    for p in paths:
        want = restate(open(p, "rb").read())
        assert got[p] == want, (p, [(g, w) for g, w in zip(got[p], want) if g != w][:3], len(got[p]), len(want))
        verdicts.append(want[0].split()[0])
    return out, verdicts


def test_block_table_and_header_match_the_restatement(prog, tmp_path):
    paths = []
    for straddle in (False, True):
        paths.append(str(tmp_path / ("hand%d.bam" % straddle)))
        hand.build(paths[-1], straddle)
    paths.append(str(tmp_path / "block700.bam"))
    bamwriter.write_bam(paths[-1], small_reads(), "refid", 3000, block=700)
    paths.append(str(tmp_path / "long_header.bam"))
    refs = long_header_bam(paths[-1])
    paths.append(str(tmp_path / "zero_bytes.bam"))
    open(paths[-1], "wb").close()
    paths.append(str(tmp_path / "eof_only.bam"))
    open(paths[-1], "wb").write(EOF_BLOCK)
    _, verdicts = compare(prog, "table", paths)
    assert verdicts == ["parsed"] * 4 + ["refused"] * 2
    # (the restatement against what the files were written from)
    want = restate(open(paths[3], "rb").read())
    assert [l for l in want if l.startswith("ref ")] == ["ref %d %s" % (ln, name.encode().hex()) for name, ln in refs]
    entries = [int(l.split()[6]) for l in want if l.startswith("block ")]
    assert entries.count(-1) > 10 and 0 < [e for e in entries if e >= 0][0] < 700          # several header blocks; the first record mid-block
    want = restate(open(paths[0], "rb").read())
    assert want[0].split()[:2] == ["parsed", "6"] and [l for l in want if l.startswith("ref ")] == ["ref 500 " + b"chrA".hex(), "ref 300 " + b"chrB".hex()]


def member(payload, isize=None, bsize=None, extra=None):
    """One BGZF block around `payload`, with the fields a test wants to lie about."""
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = co.compress(payload) + co.flush()
    xtra = b"BC\x02\x00" + struct.pack("<H", (12 + 6 + len(body) + 8 if bsize is None else bsize) - 1) if extra is None else extra
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", len(xtra)) + xtra + body +
            struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload) if isize is None else isize))


def bam_head(l_text=None, n_ref=None, l_name=None, tail=b""):
    text = b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c\tLN:400\n"
    return (b"BAM\1" + struct.pack("<I", len(text) if l_text is None else l_text) + text + struct.pack("<I", 1 if n_ref is None else n_ref) +
            struct.pack("<I", 2 if l_name is None else l_name) + b"c\0" + struct.pack("<i", 400) + tail)


def test_damaged_files_get_the_restatements_verdict(prog, tmp_path):
    # the damaged-file loop of tools/san_damaged_loop.py: its file, its four kinds of damage, its seed
    seed, n = 11, 400
    ref, _ = sy.make_reference()
    reads = sy.make_reads(ref[:3000], 2000, seed=seed, indel_sites=None)
    rng = np.random.default_rng(seed)
    good = str(tmp_path / "g.bam")
    bamwriter.write_bam(good, reads, "refid", 3000, block=4000)
    raw = open(good, "rb").read()
    paths = []
    for trial in range(n):
        data = bytearray(raw)
        kind = trial % 4
        if kind == 0:
            data = data[:int(rng.integers(1, len(data)))]
        elif kind == 1:
            for _ in range(int(rng.integers(1, 4))):
                data[int(rng.integers(0, len(data)))] ^= 1 << int(rng.integers(0, 8))
        elif kind == 2:
            a = int(rng.integers(0, len(data) - 64))
            data[a:a + int(rng.integers(1, 64))] = bytes(int(rng.integers(0, 256)) for _ in range(1))
        else:
            a = int(rng.integers(0, len(data) - 8))
            data[a:a + 4] = int(rng.integers(0, 1 << 32)).to_bytes(4, "little")
        paths.append(str(tmp_path / ("d%03d.bam" % trial)))
        open(paths[-1], "wb").write(bytes(data))
    out, verdicts = compare(prog, "damaged", paths)
    refused, parsed = verdicts.count("refused"), verdicts.count("parsed")
    print("damaged: %d refused, %d parsed" % (refused, parsed))
    assert out.rstrip().split("\n")[-1] == "damaged: %d files, %d refused, %d parsed" % (n, refused, parsed)
    assert refused >= 50 and parsed >= 50
    # ... and one file for each way the framing and the header can lie
    rec = hand.rec(0, 5, "ok", 0, [(20, "M")], "ACGTACGTACGTACGTACGT", [30] * 20)
    one = {
        "cut_in_the_block_header": raw[:10],
        "xlen_past_the_end": EOF_BLOCK[:10] + struct.pack("<H", 60000) + EOF_BLOCK[12:],
        "no_bc_subfield": member(bam_head(), extra=b"XY\x02\x00ab") + EOF_BLOCK,
        "bsize_below_header_and_trailer": member(bam_head(), bsize=20) + EOF_BLOCK,
        "isize_above_64k": member(bam_head(), isize=70000) + EOF_BLOCK,
        "l_text_ffffffff": member(bam_head(l_text=0xFFFFFFFF)) + EOF_BLOCK,
        "n_ref_ffffffff": member(bam_head(n_ref=0xFFFFFFFF)) + member(rec) + EOF_BLOCK,
        "l_name_ffffffff": member(bam_head(l_name=0xFFFFFFFF)) + member(rec) + EOF_BLOCK,
        "l_name_past_the_stream": member(bam_head(l_name=1000)) + member(rec) + EOF_BLOCK,
        "intact": member(bam_head()) + member(rec) + EOF_BLOCK,
    }
    paths = []
    for name, data in one.items():
        paths.append(str(tmp_path / (name + ".bam")))
        open(paths[-1], "wb").write(data)
    _, verdicts = compare(prog, "damaged", paths)
    assert verdicts == ["refused"] * 9 + ["parsed"]


def test_record_chain_cases(prog):
    out = run(prog, "chain")
    lines = out.rstrip().split("\n")
    assert lines[-1].startswith("chain: ") and lines[-1].endswith(", 0 failed"), out
    assert len(lines) - 1 >= 9 and all(l.startswith("ok ") for l in lines[:-1]), out
