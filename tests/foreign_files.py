"""The BAM files of tests/test_deflate_writer.py (CPU: zlib's inflate accepts them, they hit what they are for) and of
tests/test_inflate_foreign.py (GPU: the device decoder gives the same bytes): deflate streams that zlib's deflate never writes, made with
tests/deflate_writer.py.  build(tmp, name) writes one case and returns it; prove(case) asserts, from the writer's log, that the case
meets the condition of the decoder line it is aimed at.  The line numbers name the decoder as of this commit:

    far        bgzf_copy.hip:399 copy_any `dist + a0 > at`; :400 / :498-499 `dist > CNEAR` (5 880); :498 `dm + mylen <= CWIN`, `sm + mylen <= CWIN`
               (the ring's end, 8 192); bgzf_device.h:21 / bgzf_symbols.hip:801 (dist - 1) << 9 up to 32 767 under TOK_LIT2 = 1 << 24
    deep       bgzf_symbols.hip:110-153 build_long / long_lookup, :539-652 LLl / LLd, :98 peek64 (the 48-bit symbol)
    flat       bgzf_symbols.hip:363-364 / :780-784 two literals in one token; the lanes' re-synchronisation (:805-840)
    shapes     bgzf_symbols.hip:209-334 block_header: HLIT / HDIST / HCLEN, the code-length slab and its runs; bgzf_device.h:117 build_table
    structure  bgzf_symbols.hip:186-206 stored blocks -> TOK_RAW pieces (RAW_PIECE, bgzf_device.h:195); bgzf_copy.hip:446-477 the raw batch

Quality bytes are free bytes: a planned match is made to exist by copying its source over quality bytes."""
import gzip
import os
import struct

import numpy as np

from tests import deflate_writer as dw
from trueconsense_amd import synthetic as sy
from trueconsense_amd.io import bamwriter

CNEAR, CWIN, LL_ROOT, D_ROOT = 8192 - 2048 - 264, 8192, 9, 8           # bgzf_copy.hip:29-33, bgzf_device.h:35-40
REF_LEN = 3000


def source_stream(noise, n_reads=400, group=2, seed=3):
    """The inflated stream of a BAM of n_reads reads of 500 bases (798-byte records): `group` reads, each over and over — as compressible as a
    writer likes, from a block's second group on — except that a fraction `noise` of them has random qualities.
    -> (bytearray, [(start, len)] of the quality fields)"""
    import tempfile
    ref, _ = sy.make_reference(L=REF_LEN, cds=[(10, 600)])
    g, k = group, n_reads // group
    grp = sy.make_reads(ref, g, read_len=500, seed=seed)
    rng = np.random.default_rng(seed)
    qual = np.repeat(rng.integers(0, 42, (g, 500)).astype(np.uint8), k, axis=0)
    noisy = rng.random(g * k) < noise
    qual[noisy] = rng.integers(0, 42, (int(noisy.sum()), 500)).astype(np.uint8)
    n = g * k
    rep = lambda key, w=1: np.repeat(np.asarray(grp[key]).reshape(g, w), k, axis=0).reshape(-1)      # (sorted by position, as the reads come)
    reads = {"n_reads": n, "pos": rep("pos"), "flag": rep("flag"), "l_qseq": rep("l_qseq"), "tid": np.zeros(n, np.int32),
             "cigar_off": np.arange(n + 1, dtype=np.uint64), "cigar": rep("cigar"), "seq_off": np.arange(n + 1, dtype=np.uint64) * np.uint64(250),
             "seq": rep("seq", 250), "qual": qual.reshape(-1), "names": np.frombuffer(b"".join(b"q%06d" % i for i in range(n)), np.uint8),
             "name_off": np.arange(n + 1, dtype=np.uint64) * np.uint64(7)}
    with tempfile.TemporaryDirectory() as tmp:
        p = os.path.join(tmp, "s.bam")
        bamwriter.write_bam(p, reads, "r", REF_LEN)
        stream = bytearray(gzip.decompress(open(p, "rb").read()))
    o = 12 + struct.unpack_from("<i", stream, 4)[0]
    o += 8 + struct.unpack_from("<i", stream, o)[0]                    # (one reference)
    fields = []
    while o < len(stream):
        bs, = struct.unpack_from("<i", stream, o)
        l_name, n_cig, l_seq = stream[o + 12], struct.unpack_from("<H", stream, o + 16)[0], struct.unpack_from("<i", stream, o + 20)[0]
        fields.append((o + 36 + l_name + 4 * n_cig + (l_seq + 1) // 2, l_seq))
        o += 4 + bs
    assert o == len(stream) and fields[-1][0] + fields[-1][1] == o
    return stream, fields


def write_plain(path, stream):
    """the stream as a BAM file the usual way (zlib, 0xFF00-byte blocks): the source file the rewritten one is held against"""
    with open(path, "wb") as fh:
        for o in range(0, len(stream), 0xFF00):
            fh.write(bamwriter._bgzf_block(bytes(stream[o:o + 0xFF00]), 6))
        fh.write(dw.EOF_BLOCK)


def block_for(total, around, min_last=0):
    """a BGZF block size near `around` whose last block of a stream of `total` bytes is at least min_last bytes long"""
    return next(b for b in range(around, 0, -1) if total % b >= min_last)


class Planter:
    """Plans matches and makes them exist: the source's bytes are copied over quality bytes.  A planned match lies inside one BGZF block
    (`block` inflated bytes each) and inside one quality field; what a plan has read or written is left alone afterwards."""

    def __init__(self, stream, fields, block):
        self.stream, self.fields, self.block = stream, fields, block
        self.plan, self.frozen, self.made, self.turn = {}, [], [], 0

    def free(self, a, b):
        return all(b <= x or y <= a for x, y in self.frozen)

    def plant(self, length, dist=None, ok=lambda k, o, a0: True, fields=None, step=1):
        """the next place (field by field from the last one used on, so that the plans spread over the file; byte by byte) where a match (length, dist) fits and ok(block, offset in it, the block's
        uout & 15) holds; dist None: the source starts at the block's first byte (dist = offset); a function: dist(block, offset).  -> (block, offset, dist)"""
        turn = self.turn if fields is None else 0
        for n, (start, flen) in enumerate(self.fields[turn:] + self.fields[:turn] if fields is None else fields):
            for p in range(start, start + flen - length + 1, step):
                k, o = divmod(p, self.block)
                dd = o if dist is None else dist(k, o) if callable(dist) else dist
                if not (1 <= dd <= min(o, 32768)) or o + length > min(self.block, len(self.stream) - k * self.block):
                    continue
                if not ok(k, o, (k * self.block) & 15) or not self.free(p, p + length):
                    continue
                for i in range(length):
                    self.stream[p + i] = self.stream[p + i - dd]
                self.frozen += [(p, p + length), (p - dd, p - dd + length)]
                self.plan.setdefault(k, []).append((o, length, dd))
                self.made.append((k, o, length, dd))
                if fields is None:
                    self.turn = (turn + n + 1) % len(self.fields)
                return k, o, dd
        raise AssertionError("no place for a match of %d bytes at distance %s" % (length, dist))


class Case:
    def __init__(self, name, path, src_path, logs, planter=None, **more):
        self.name, self.path, self.src_path, self.logs, self.planter = name, path, src_path, logs, planter
        self.__dict__.update(more)

    @property
    def payload(self):
        """bytes of bgzf_symbols' staged payload for the file's largest block, as the host sizes it (bgzf_host.cpp:62): the variant"""
        return max((((g["cin"] & 3) * 8 + g["clen"] * 8 + 31) // 32 + 6) * 4 for g in self.logs)

    @property
    def variant(self):
        return "two blocks" if self.payload <= 4096 else "one block" if self.payload <= 16384 else "windowed"

    @property
    def ratio(self):
        return sum(g["ulen"] for g in self.logs) / os.path.getsize(self.path)

    def tokens(self):
        """every token of the file: (log of its BGZF block, bit position, deflate block, len or -1, dist or byte, code bits, extra bits,
        distance code bits, distance extra bits)"""
        return [(g,) + t for g in self.logs for t in g["tokens"]]

    def matches(self):
        return [t for t in self.tokens() if t[3] >= 0]


def finish(tmp, name, stream, recipe, planter=None, **more):
    src = os.path.join(str(tmp), name + ".src.bam")
    dst = os.path.join(str(tmp), name + ".bam")
    write_plain(src, stream)
    return Case(name, dst, src, dw.rewrite_bam(src, dst, recipe), planter, **more)


# ---- far -----------------------------------------------------------------------------------------------------------------------------
FAR = {"far-A": (0.0, 65280), "far-B": (0.25, 65001), "far-C": (0.8, 60013)}        # noise, BGZF block size (a0 = 0 / any)


def build_far(tmp, name):
    noise, block = FAR[name]
    stream, fields = source_stream(noise)
    P = Planter(stream, fields, block)
    P.plant(258, 32768)
    P.plant(3, 32768)
    for i in range(50):                                                 # the last 262 distances, which zlib's deflate never uses
        P.plant(3 + (i * 37) % 256, 32507 + (i * 53) % 262)
    for i in range(50):                                                 # zlib drops these as TOO_FAR
        P.plant(3, 4097 + (i * 577) % 28672)
    for dist in (CNEAR - 1, CNEAR, CNEAR + 1):                          # bgzf_copy.hip:400, :498-499: near / far
        for length in (5, 40, 64, 65, 200, 258):
            P.plant(length, dist)
    for lo in (1, CNEAR + 1):                                           # :399: the source starts at the block's first byte
        for length in (3, 70):
            P.plant(length, None, ok=lambda k, o, a0, lo=lo: o >= lo)
    for length, dist in ((100, 7), (258, 1), (64, 64), (200, 200), (65, 64), (201, 200), (4, 3), (3, 3), (3, 2)):    # :404-417 periods
        P.plant(length, dist)
    for dist in (300, 5000, CNEAR + 7, 20000):                          # :498: destination / source across the ring's end
        for length in (9, 70, 258):
            P.plant(length, dist, ok=lambda k, o, a0, l=length: (a0 + o) // CWIN != (a0 + o + l - 1) // CWIN)
            P.plant(length, dist, ok=lambda k, o, a0, l=length, d=dist: (a0 + o - d) // CWIN != (a0 + o - d + l - 1) // CWIN)
    return finish(tmp, name, stream, dw.plain_recipe(block, "farthest", P.plan), P)


def prove_far(c):
    m = c.matches()
    count = lambda f: sum(1 for t in m if f(t[3], t[4]))
    assert count(lambda l, d: d == 32768 and l == 258) >= 1
    assert count(lambda l, d: d == 32768 and l == 3) >= 1
    assert count(lambda l, d: 32507 <= d <= 32768) >= 50
    assert count(lambda l, d: l == 3 and d > 4096) >= 50
    made = c.planter.made
    in_log = {(id(t[0]), t[3], t[4]) for t in m}
    for k, o, l, d in made:                                             # every planned match is in the stream as planned
        assert (id(c.logs[k]), l, d) in in_log, (k, o, l, d)
    for dist in (CNEAR - 1, CNEAR, CNEAR + 1):
        assert sum(1 for k, o, l, d in made if d == dist) >= 6
    assert any(d == o and o <= CNEAR for k, o, l, d in made) and any(d == o and o > CNEAR for k, o, l, d in made)
    assert any(d < l - 1 for k, o, l, d in made) and any(d == l for k, o, l, d in made) and any(d == l - 1 for k, o, l, d in made)
    a0 = lambda k: c.logs[k]["uout"] & 15
    assert sum(1 for k, o, l, d in made if (a0(k) + o) // CWIN != (a0(k) + o + l - 1) // CWIN) >= 12
    assert sum(1 for k, o, l, d in made if (a0(k) + o - d) // CWIN != (a0(k) + o - d + l - 1) // CWIN) >= 12


# ---- deep ----------------------------------------------------------------------------------------------------------------------------
DEEP = {"deep-A": (0.01, 30011), "deep-B": (0.15, 30000), "deep-C": (0.6, 29989)}


def is_48(t):
    return t[5:9] == (15, 5, 15, 13)


def build_deep(tmp, name):
    noise, around = DEEP[name]
    stream, fields = source_stream(noise, group=1)
    block = block_for(len(stream), around, 21000)
    P = Planter(stream, fields, block)
    # 15 + 5 + 15 + 13 bits: a length of 131 .. 257 (symbols 281 - 284) at a distance beyond 16 384 (symbols 28, 29) — first the
    # stream's last bytes (the payload's last symbol), then two in every quality field that lies far enough into its block
    P.plant(140, 20000, fields=fields[-1:], ok=lambda k, o, a0: o + 140 == len(stream) - k * block)
    i = 0
    for f in fields[:-1]:
        for part in (0, 1):
            length = 131 + (i * 29) % 120
            i += 1
            try:
                P.plant(length, lambda k, o, i=i: 16385 + (i * 1237) % max(1, min(o, 32768) - 16384), fields=[(f[0] + 250 * part, 250)], step=250)
            except AssertionError:                                      # (within 16 384 bytes of the block's start, or across its end)
                pass

    def layout(tokens, k):
        # cuts behind the 3rd and the 9th planned match of the block: 48-bit symbols in front of an end-of-block code, fresh tables behind
        cuts, at = [], 0
        want = {o for o, _, _ in sorted(P.plan.get(k, ()))[2::6][:2]}
        for j, t in enumerate(tokens):
            if at in want:
                cuts.append(j + 1)
            at += 1 if t[0] == "lit" else t[1]
        blocks, a = [], 0
        for b in cuts + [len(tokens)]:
            ll, d = dw.lengths_for(tokens[a:b], "deep", "deep")
            blocks.append(dict(kind="dynamic", n=b - a, ll=ll, d=d))
            a = b
        return blocks
    return finish(tmp, name, stream, dw.plain_recipe(block, "farthest", P.plan, layout), P)


def prove_deep(c):
    toks = c.tokens()
    wide = [t for t in toks if is_48(t)]
    assert {((t[0]["cin"] & 3) * 8 + t[1]) % 32 for t in wide} == set(range(32)), "the 48-bit symbol at every bit residue of a dword"
    assert all(131 <= t[3] <= 257 and t[4] > 16384 for t in wide) and len(wide) >= 100
    # ... as the last symbol in front of an end-of-block code (blocks cut behind one), and as the payload's last symbol
    last_of = {}
    for t in toks:
        last_of[(id(t[0]), t[2])] = t
    n_before_eob = sum(1 for t in last_of.values() if is_48(t))
    assert n_before_eob >= 3
    g = c.logs[-1]
    t = g["tokens"][-1]
    assert is_48((g,) + t) and g["blocks"][-1]["eob"] == t[0] + 48 and g["blocks"][-1]["final"] == 1
    # nearly every symbol is a code longer than the root tables, in both trees; all 286 / 30 symbols are coded
    lit_len = [t[5] for t in toks]
    dist = [t[7] for t in toks if t[3] >= 0]
    assert sum(1 for b in lit_len if b > LL_ROOT) >= 0.9 * len(lit_len) and sum(1 for b in dist if b > D_ROOT) >= 0.9 * len(dist)
    for g in c.logs:
        for b in g["blocks"]:
            assert (b["hlit"], b["hdist"], b["hclen"]) == (286, 30, 19) and all(b["ll"]) and all(b["d"])
            assert all(b["ll"][s] == 15 for s in (281, 282, 283, 284)) and b["d"][28] == b["d"][29] == 15


# ---- flat ----------------------------------------------------------------------------------------------------------------------------
FLAT = {"flat-lit-A": (0.5, 3300, "literals", 96), "flat-lit-B": (0.5, 12000, "literals", 200), "flat-lit-C": (0.5, 20000, "literals", 200),
        "flat-match-A": (0.0, 16000, "nearest", 200), "flat-match-B": (0.2, 60000, "nearest", 400), "flat-match-C": (0.7, 60000, "nearest", 400)}


def build_flat(tmp, name):
    noise, block, policy, n = FLAT[name]
    stream, fields = source_stream(noise, n)
    return finish(tmp, name, stream, dw.plain_recipe(block, policy, ll="flat", d="none" if policy == "literals" else "huffman"))


def prove_flat(c):
    toks = c.tokens()
    assert all(t[5] in (8, 9) for t in toks)                            # literal / length codes of 8 and 9 bits, nothing else
    assert all(set(b["ll"]) == {8, 9} and b["hlit"] == 286 for g in c.logs for b in g["blocks"])
    assert any(t[3] >= 0 for t in toks) == ("match" in c.name)
    assert any(s == 16 and ev == 3 for g in c.logs for b in g["blocks"] for s, ev in b["cl"])        # code 16 with 6


# ---- shapes --------------------------------------------------------------------------------------------------------------------------
SHAPES = {"single0-A": (0.5, 5000), "single0-B": (0.5, 20000), "single0-C": (0.5, 40000), "single29-C": (0.5, 40000),
          "nodist-A": (0.5, 5000), "nodist-B": (0.5, 20000), "nodist-C": (0.5, 40000),
          "full-none-B": (0.2, 30000), "full-max-B": (0.2, 30000), "full-greedy-B": (0.2, 30000),
          "hclen5-A": (0.5, 3300), "hclen19-A": (0.5, 3300), "runs-B": (0.5, 20000)}


def build_shapes(tmp, name):
    noise, block = SHAPES[name]
    kind = name.split("-")[0]
    stream, fields = source_stream(noise, 200)
    P = Planter(stream, fields, block)
    if kind == "single0":                                               # one distance code of one bit, symbol 0: runs of a byte
        for i, f in enumerate(fields[::3]):
            P.plant(3 + (i * 41) % 256, 1, fields=[f])
        recipe = dw.plain_recipe(block, "literals", P.plan, d="single")
    elif kind == "single29":                                            # ... symbol 29 (HDIST = 30, 29 zeros in front): distances 24 577 .. 32 768
        for i, f in enumerate(fields):
            try:
                P.plant(3 + (i * 41) % 256, 24577 + (i * 1361) % 8192, fields=[f])
            except AssertionError:
                pass
        recipe = dw.plain_recipe(block, "literals", P.plan, d="single")
    elif kind == "nodist":                                              # no distance code at all: HDIST = 1 with length 0, HLIT = 257
        recipe = dw.plain_recipe(block, "literals", d="none")
    elif kind == "full":                                                # every one of the 286 + 30 symbols coded, the three ways to write the lengths
        recipe = dw.plain_recipe(block, "farthest", ll="deep", d="deep", clenc=name.split("-")[1])
    elif kind in ("hclen5", "hclen19"):
        # 256 codes of 8 bits — every literal but one the block does not use, and the end-of-block code —: the code-length code needs
        # 16, 17, 18, 0 and 8 only, HCLEN = 5, the least a valid header can have (with 4 no length but 0 can be written: no
        # end-of-block code, see the refused streams); "hclen19": the same with all 19 written, the last 14 of them 0
        def layout(tokens, k):
            used = {t[1] for t in tokens}
            unused = next(b for b in range(255, -1, -1) if b not in used)
            return [dict(kind="dynamic", n=len(tokens), ll=[8 * (s != unused) for s in range(257)], d=[0], hclen=int(kind[5:]), clenc="none")]
        recipe = dw.plain_recipe(block, "literals", layout=layout)
    else:
        # "runs": a deflate block of quality bytes alone (values under 42): 214 literals in a row without a code — code 18 with 138 —, and
        # a code the data does not need: 254, 255, 256 and eight distance symbols at 3 bits, written as one sequence — a code-16 run
        # from the literal lengths into the distance lengths
        assert kind == "runs"
        starts = {}
        for start, flen in fields:
            k, o = divmod(start, block)
            if o + flen <= block:
                starts.setdefault(k, o)

        def layout(tokens, k):
            o = starts[k]
            blocks = []
            for a, b in ((0, o), (o, o + 250), (o + 250, o + 500), (o + 500, len(tokens))):
                ll, d = dw.lengths_for(tokens[a:b], "huffman", "none")
                blocks.append(dict(kind="dynamic", n=b - a, ll=ll, d=d, clenc="greedy"))
            used = sorted({t[1] for t in tokens[o + 250:o + 500]})
            order = [254, 255, 256] + [s for s in range(254) if s not in used] + used
            blocks[2].update(ll=dw.complete(257, [3, 3, 3], order), d=[3] * 8, clenc="max")
            return blocks
        recipe = dw.plain_recipe(block, "literals", layout=layout)
    return finish(tmp, name, stream, recipe, P)


def prove_shapes(c):
    kind = c.name.split("-")[0]
    blocks = [b for g in c.logs for b in g["blocks"]]
    m = c.matches()
    if kind == "single0":
        assert len(m) >= 30 and all(t[4] == 1 and t[7] == 1 for t in m) and any(b["d"] == [1] for b in blocks)
    elif kind == "single29":
        assert len(m) >= 30 and all(t[4] >= 24577 and t[7] == 1 for t in m) and any(b["d"] == [0] * 29 + [1] for b in blocks)
    elif kind == "nodist":
        assert not m and all(b["d"] == [0] and b["hdist"] == 1 for b in blocks) and any(b["hlit"] == 257 for b in blocks)
    elif kind == "full":
        assert all((b["hlit"], b["hdist"], b["hclen"]) == (286, 30, 19) and all(b["ll"]) and all(b["d"]) for b in blocks)
        repeats = any(s >= 16 for b in blocks for s, _ in b["cl"])
        assert repeats == (c.name != "full-none-B") and all(len(b["cl"]) == 316 for b in blocks if not repeats)
    elif kind in ("hclen5", "hclen19"):
        assert all(b["hclen"] == int(kind[5:]) and b["hlit"] == 257 and b["hdist"] == 1 for b in blocks)
    else:
        assert any((18, 127) in b["cl"] for b in blocks) and sum(b["crossing16"] for b in blocks) >= len(c.logs) - 1
        assert any(s == 16 and ev == 3 for b in blocks for s, ev in b["cl"])


# ---- structure -----------------------------------------------------------------------------------------------------------------------
STRUCTURE = {"structure-A": 3000, "structure-B": 10000, "structure-C": 65505}


def empty_dynamic(hclen=None):
    return dict(kind="dynamic", n=0, ll=[0] * 256 + [1], d=[0], hclen=hclen)           # the end-of-block code and nothing else


def build_structure(tmp, name):
    """Literal tokens only (a token is a byte) and one planned match per block; what BGZF block k holds:
       k % 4 == 0   stored blocks whose header starts at every bit alignment 0 .. 7 (fillers: empty fixed blocks of 10 bits, empty dynamic
                    ones of an odd number of bits), an empty dynamic block, non-final empty fixed and stored blocks, an empty stored block last
       k % 4 == 1   >= 30 deflate blocks of ~ 60 bytes, the kinds in turn, every dynamic one with tables of its own
       k % 4 == 2   a stored block of 1 byte, then one of 700 bytes ("A") or of 8 191, 8 192, 8 193 bytes — one per BGZF block in "B", all in
                    one in "C" —, then a dynamic block whose planned match has its source in the stored bytes
       k % 4 == 3   ("C") one stored block of 65 505 bytes: the largest a BGZF block holds (5 + 65 505 + 26 = 65 536)"""
    block = STRUCTURE[name]
    stream, fields = source_stream(0.5, {"A": 96, "B": 200, "C": 400}[name[-1]])
    P = Planter(stream, fields, block)
    n_blocks = (len(stream) + block - 1) // block
    cls = name[-1]
    edges = {"A": [[700]], "B": [[8191], [8192], [8193]], "C": [[8191, 8192, 8193]]}[cls]
    stored_of = {}
    for k in range(2, n_blocks - 1, 4):
        stored_of[k] = [1] + edges[(k // 4) % len(edges)]
        first = 1 + sum(stored_of[k])
        # a match in the Huffman block behind the stored ones, its source the last stored block's last bytes but twenty
        P.plant(40, lambda k2, o, first=first: o - (first - 60), ok=lambda k2, o, a0, k=k, first=first: k2 == k and o >= first + 300)
    bits_of = lambda b: dw.encode([], [b])[1]["blocks"][0]["eob"] + 1
    odd = empty_dynamic(None if bits_of(empty_dynamic()) % 2 else 19)   # (19: one more 3-bit length — an odd number of bits)
    e_bits = bits_of(odd)
    assert e_bits % 2 == 1

    def pieces(tokens, sizes):
        """token counts of deflate blocks that hold `sizes` bytes each (a planned match is one token of several bytes)"""
        out, j = [], 0
        for s in sizes:
            n, got = 0, 0
            while got < s:
                got += 1 if tokens[j][0] == "lit" else tokens[j][1]
                j, n = j + 1, n + 1
            assert got == s, "a deflate block would end inside a planned match"
            out.append(n)
        return out

    def layout(tokens, k):
        total = sum(1 if t[0] == "lit" else t[1] for t in tokens)
        if k % 4 == 0 and total >= 1200:
            blocks, sizes = [], []
            for a in range(8):                                          # after a stored block the stream is byte-aligned: fillers of a (mod 8) bits
                j, f = next((j, f) for j in range(8) for f in range(4) if (e_bits * j + 10 * f) % 8 == a)
                blocks += [dict(odd, final=0) for _ in range(j)] + [dict(kind="fixed", n=0, final=0) for _ in range(f)] + [dict(kind="stored")]
                sizes += [0] * (j + f) + [100 + a]
            blocks += [dict(kind="stored", n=0, final=0), dict(kind="huffman"), dict(empty_dynamic(), final=0), dict(kind="stored", n=0, final=1)]
            sizes += [0, total - sum(sizes), 0, 0]
        elif k % 4 == 1 and total >= 2400:
            kinds = ("huffman", "fixed", "stored", "flat", "fixed", "deep", "stored")
            blocks = [dict(kind=kinds[i % 7]) for i in range(36)]
            sizes = [60 + i for i in range(35)]
            sizes.append(total - sum(sizes))
        elif k in stored_of:
            blocks = [dict(kind="stored") for _ in stored_of[k]] + [dict(kind="huffman")]
            sizes = stored_of[k] + [total - sum(stored_of[k])]
        elif k % 4 == 3 and total == 65505:
            blocks, sizes = [dict(kind="stored")], [total]
        else:
            blocks, sizes = [dict(kind="huffman")], [total]
        at = 0
        for b, n in zip(blocks, pieces(tokens, sizes)):
            if b.get("n") is None:
                b["n"] = n
            if b["kind"] in ("huffman", "flat", "deep"):
                ll, d = dw.lengths_for(tokens[at:at + n], b["kind"], "huffman" if b["kind"] == "huffman" else "none")
                if len(ll) == 286:                                      # the codes of the literals the piece does not use, shuffled: no two tables alike
                    idle = [s for s in range(256) if ("lit", s) not in tokens[at:at + n]]
                    for s, l in zip(idle, [ll[s] for s in np.random.default_rng(1000 * k + at).permutation(idle)]):
                        ll[s] = l
                b.update(kind="dynamic", ll=ll, d=d)
            at += b["n"]
        return blocks
    return finish(tmp, name, stream, dw.plain_recipe(block, "literals", P.plan, layout), P, stored_of=stored_of)


def prove_structure(c):
    cls = c.name[-1]
    blocks = [(g, b) for g in c.logs for b in g["blocks"]]
    stored = [b for g, b in blocks if b["kind"] == "stored"]
    want = {"A": {1, 700}, "B": {1, 8191, 8192, 8193}, "C": {1, 8191, 8192, 8193, 65505}}[cls]
    assert want <= {b["bytes"] for b in stored}
    assert {b["bit"] % 8 for b in stored if b["bytes"]} == set(range(8))            # a stored block's header at every bit alignment
    assert max(len(g["blocks"]) for g in c.logs) >= 30
    g = next(g for g in c.logs if len(g["blocks"]) >= 30)
    kinds = [b["kind"] for b in g["blocks"]]
    assert all(a != b for a, b in zip(kinds, kinds[1:])) and {"stored", "fixed", "dynamic"} == set(kinds)
    tables = [tuple(b["ll"]) for b in g["blocks"] if b["kind"] == "dynamic"]
    assert len(set(tables)) == len(tables) >= 10                                    # fresh, unrelated tables
    assert any(b["kind"] == "dynamic" and b["n"] == 0 and b["ll"] == [0] * 256 + [1] and b["final"] == 0 for g, b in blocks)     # end-of-block code only
    assert any(b["kind"] == "fixed" and b["n"] == 0 and not b["final"] for g, b in blocks)
    assert any(b["kind"] == "stored" and b["bytes"] == 0 and not b["final"] for g, b in blocks)
    assert any(b["kind"] == "stored" and b["bytes"] == 0 and b["final"] and b is g["blocks"][-1] for g, b in blocks)
    # a match in a Huffman block whose source lies in the stored bytes of an earlier deflate block
    n_into = 0
    for k, o, l, d in c.planter.made:
        b_src = [b for b in c.logs[k]["blocks"] if b["out"] <= o - d and o - d + l <= b["out"] + b["bytes"]]
        b_dst = [b for b in c.logs[k]["blocks"] if b["out"] <= o < b["out"] + b["bytes"]]
        n_into += bool(b_src) and b_src[0]["kind"] == "stored" and b_dst[0]["kind"] == "dynamic"
    assert n_into >= 1 and n_into == len(c.stored_of)


GROUPS = {"far": (FAR, build_far, prove_far), "deep": (DEEP, build_deep, prove_deep), "flat": (FLAT, build_flat, prove_flat),
          "shapes": (SHAPES, build_shapes, prove_shapes), "structure": (STRUCTURE, build_structure, prove_structure)}
NAMES = [n for cases, _, _ in GROUPS.values() for n in cases]
SUBSET = ["far-B", "deep-B", "flat-lit-B", "flat-match-B", "structure-B"]      # the middle block size of far, deep, flat, structure: pass B, small windows
# the symbol decoder each file must get (bgzf_symbols.hip:986-994, by the largest payload) and the side of 12 : 1 it lies on
# (bam_device.hip:227: bgzf_copy<false, false> at 12 : 1 and more if the payloads are small, bgzf_copy<true, *> under it)
VARIANT = {"A": "two blocks", "B": "one block", "C": "windowed"}
ABOVE_12 = {"far-A", "flat-match-A"}
BELOW_4 = {n for n in NAMES if n[-1] != "A" and n not in ("far-B", "deep-B", "flat-match-B")} | {"flat-lit-A", "single0-A", "nodist-A", "hclen5-A", "hclen19-A", "structure-A"}


def build(tmp, name):
    group = next(g for g, (cases, _, _) in GROUPS.items() if name in cases)
    return GROUPS[group][1](tmp, name)


def prove(case):
    group = next(g for g, (cases, _, _) in GROUPS.items() if case.name in cases)
    assert case.variant == VARIANT[case.name[-1]], (case.name, case.payload)
    GROUPS[group][2](case)
