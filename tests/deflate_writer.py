"""A DEFLATE writer for the tests, from RFC 1951: what zlib's deflate never emits, written on purpose.  Plain Python, readable over
fast (the files are small); zlib is used for the CRC-32 and, in rewrite_bam, to INFLATE the source file — never to compress.
Test-side only: nothing under trueconsense_amd/ imports this.

    tokens    ("lit", byte) | ("match", len, dist)                                  tokenize(): a policy + matches planned by the caller
    blocks    {"kind": "stored" | "fixed" | "dynamic", "n": tokens in the block,    encode(): one deflate block each, in order
               "ll": [...], "d": [...]           code lengths (dynamic), given — the makers below give complete codes of a shape
               "hclen": count, "clenc": "none" | "max" | "greedy"                   the header's code-length code and its repeats
               "final": 0 | 1}                   (default: 1 on the last block)
    log       what encode() wrote where: log["tokens"][i] = (bit position, block, len or -1, dist, code bits, extra bits, distance code
              bits, distance extra bits), log["blocks"][j] = {"kind", "bit", "n", "bytes", "out", ...header fields}
"""
import bisect
import gzip
import heapq
import struct
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k // 2 for k in range(2, 28)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8                # (288: 286 and 287 have codes, never written)
FIXED_D = [5] * 30                                                  # (30 and 31 have codes too: never written)
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def len_symbol(length):
    """-> (literal/length symbol, extra bits, their value)"""
    s = 28 if length == 258 else bisect.bisect_right(LEN_BASE, length) - 1
    return 257 + s, LEN_EXTRA[s], length - LEN_BASE[s]


def dist_symbol(dist):
    s = bisect.bisect_right(DIST_BASE, dist) - 1
    return s, DIST_EXTRA[s], dist - DIST_BASE[s]


class BitWriter:
    """Bits go out least significant first (RFC 1951 3.1.1); Huffman codes are handed over already reversed."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    @property
    def pos(self):
        return 8 * len(self.out) + self.n

    def bits(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data


def kraft(lens):
    """sum of 2^-len in units of 2^-15: 32768 for a complete code"""
    return sum(1 << (15 - l) for l in lens if l)


def canonical(lens):
    """code lengths -> [(code with its bits reversed, length) or None]: RFC 1951 3.2.2"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        out.append((int(format(nxt[l], "0%db" % l)[::-1], 2), l) if l else None)
        nxt[l] += 1 if l else 0
    return out


# ---- code-length makers ------------------------------------------------------------------------------------------------------------
def huffman(freqs, limit=15):
    """Huffman lengths for the symbols with freqs > 0, none longer than `limit` (frequencies halved until the tree fits)."""
    f = list(freqs)
    while True:
        heap = [(w, s, [s]) for s, w in enumerate(f) if w > 0]
        lens = [0] * len(f)
        if len(heap) == 1:
            lens[heap[0][1]] = 1                    # one code of one bit: incomplete, and legal
            return lens
        heapq.heapify(heap)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                lens[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        if max(lens) <= limit:
            return lens
        f = [(w + 1) // 2 if w else 0 for w in f]


def complete(n, short, order):
    """A complete code over n symbols: the first symbols of `order` (a permutation of range(n)) get the lengths in `short`, all others
    two adjacent lengths L - 1 and L, L as large as completeness allows; the LAST symbols of `order` get L."""
    m, left = n - len(short), 32768 - kraft(short)
    for L in range(15, 0, -1):
        unit = 1 << (15 - L)
        if left % unit == 0 and m <= left // unit <= 2 * m:
            a = left // unit - m                    # a symbols of L - 1 bits, m - a of L bits
            lens = [0] * n
            for s, l in zip(order, list(short) + [L - 1] * a + [L] * (m - a)):
                lens[s] = l
            assert kraft(lens) == 32768
            return lens
    raise ValueError("no complete code of this shape")


def deep(n, order):
    """a chain 1 .. k, the rest at 14 / 15 bits: nearly every symbol is a code longer than the decoder's root tables"""
    for k in range(1, 14):
        try:
            lens = complete(n, range(1, k + 1), order)
        except ValueError:
            continue
        if max(lens) == 15:
            return lens
    raise ValueError(n)


def flat(n, order):
    """all 8 / 9 bits (n = 257 .. 286)"""
    return complete(n, [], order)


def by_use(freqs, n, last=()):
    """a permutation of range(n) for the makers above: unused and rare symbols first (they get the short codes of a chain), the most
    used ones at the end — and behind them `last`, the symbols that must get the longest codes"""
    order = sorted((s for s in range(n) if s not in last), key=lambda s: (freqs[s] if s < len(freqs) else 0, s))
    return order + list(last)


def token_freqs(tokens):
    ll, d = [0] * 286, [0] * 30
    ll[256] = 1
    for t in tokens:
        if t[0] == "lit":
            ll[t[1]] += 1
        else:
            ll[len_symbol(t[1])[0]] += 1
            d[dist_symbol(t[2])[0]] += 1
    return ll, d


def lengths_for(tokens, ll="huffman", d="huffman", last_ll=(281, 282, 283, 284), last_d=(28, 29)):
    """code lengths of a named shape for a block of these tokens -> (ll lengths, d lengths)"""
    fl, fd = token_freqs(tokens)

    def trim(lens, least):                          # HLIT / HDIST: up to the last symbol that has a code
        return lens[:max([least] + [s + 1 for s, l in enumerate(lens) if l])]
    if ll == "huffman":
        L = trim(huffman(fl), 257)
    else:
        L = (deep if ll == "deep" else flat)(286, by_use(fl, 286, last_ll))
    if d == "huffman":
        D = trim(huffman(fd), 1) if any(fd) else [0]
    elif d == "deep":
        D = deep(30, by_use(fd, 30, last_d))
    elif d == "single":                             # one distance code of one bit (all matches must use its symbol)
        used = [s for s, w in enumerate(fd) if w]
        assert len(used) <= 1, used
        D = [0] * used[0] + [1] if used else [0]
    else:
        assert d == "none" and not any(fd)
        D = [0]                                     # HDIST = 1 with length 0: no distance code at all
    return L, D


# ---- the code lengths in a dynamic block's header -----------------------------------------------------------------------------------
def code_length_symbols(seq, mode, hlit):
    """RFC 1951 3.2.7 -> [(symbol 0 .. 18, extra bits, value)].  "none": no repeat codes at all; "greedy": the longest repeat at every
    place, literal/length and distance lengths apart (zlib's way); "max": the longest repeats over both as ONE sequence — runs cross
    from the literal lengths into the distance lengths."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v = seq[i]
        stop = n if mode == "max" or i >= hlit else hlit
        j = i
        while j < stop and seq[j] == v:
            j += 1
        run = j - i
        if mode == "none" or run < 3 + (v != 0):
            out.append((v, 0, 0))
            i += 1
        elif v == 0:
            r = min(run, 138)
            out.append((17, 3, r - 3) if r <= 10 else (18, 7, r - 11))
            i += r
        else:
            out.append((v, 0, 0))
            i, run = i + 1, run - 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, 2, r - 3))
                i, run = i + r, run - r
    return out


def dynamic_header(bw, ll, d, hclen=None, clenc="greedy"):
    """HLIT, HDIST, HCLEN, the code-length code, the code lengths -> what was written, for the log"""
    assert 257 <= len(ll) <= 286 and 1 <= len(d) <= 30
    syms = code_length_symbols(list(ll) + list(d), clenc, len(ll))
    freq = [0] * 19
    for s, _, _ in syms:
        freq[s] += 1
    cl = huffman(freq, 7)
    need = max(4, max(i for i in range(19) if cl[CL_ORDER[i]]) + 1)
    count = need if hclen is None else hclen
    assert need <= count <= 19, (need, count)
    bw.bits(len(ll) - 257, 5)
    bw.bits(len(d) - 1, 5)
    bw.bits(count - 4, 4)
    for i in range(count):
        bw.bits(cl[CL_ORDER[i]], 3)
    codes = canonical(cl)
    crossing = 0
    at = 0
    for s, eb, ev in syms:
        bw.bits(*codes[s])
        bw.bits(ev, eb)
        rep = 1 if s < 16 else ev + (3 if s < 18 else 11)
        crossing += s == 16 and at < len(ll) < at + rep
        at += rep
    return {"hlit": len(ll), "hdist": len(d), "hclen": count, "cl": [(s, ev) for s, _, ev in syms], "crossing16": crossing}


# ---- tokens ------------------------------------------------------------------------------------------------------------------------
def _common(a, b):
    x = int.from_bytes(a, "little") ^ int.from_bytes(b, "little")
    return len(a) if x == 0 else ((x & -x).bit_length() - 1) // 8


def tokenize(data, policy="nearest", plan=()):
    """data -> tokens.  policy: "nearest" (the longest of the eight latest candidates, ties to the nearer one), "farthest" (the longest of
    the 32 candidates furthest back within 32 768, ties to the further one; length-3 matches at any distance included), "literals".  plan: [(offset,
    len, dist)] — emitted as exactly these matches, whatever the policy; the bytes must agree."""
    planned = {o: (l, dd) for o, l, dd in plan}
    starts = sorted(planned) + [len(data)]
    tokens, table, i, n, nxt = [], {}, 0, len(data), 0
    while i < n:
        while starts[nxt] < i:
            nxt += 1
        if i in planned:
            l, dd = planned[i]
            assert 3 <= l <= 258 and 1 <= dd <= min(i, 32768) and i + l <= n, (i, l, dd)
            assert all(data[i + k] == data[i + k - dd] for k in range(l)), ("planned match: bytes differ", i, l, dd)
            assert starts[nxt + 1] >= i + l, ("planned matches overlap", i)
            best = (l, dd)
        else:
            best, limit = None, min(258, starts[nxt] - i)
            cands = table.get(data[i:i + 3]) if policy != "literals" and limit >= 3 else None
            if cands:
                k = bisect.bisect_left(cands, i - 32768)
                for c in (cands[k:k + 32] if policy == "farthest" else cands[:-9:-1]):
                    l = _common(data[i:i + limit], data[c:c + limit])
                    if c >= i - 32768 and l >= 3 and (best is None or l > best[0]):
                        best = (l, i - c)
        if best is None:
            tokens.append(("lit", data[i]))
            best = (1, 0)
        else:
            tokens.append(("match", best[0], best[1]))
        if policy != "literals":
            for j in range(i, min(i + best[0], n - 2)):
                table.setdefault(data[j:j + 3], []).append(j)
        i += best[0]
    return tokens


def token_bytes(tokens, out):
    """appends what the tokens stand for to `out` (a bytearray: the block's output so far)"""
    for t in tokens:
        if t[0] == "lit":
            out.append(t[1])
        else:
            assert 1 <= t[2] <= len(out), ("a match reaches before the first byte", t, len(out))
            for _ in range(t[1]):
                out.append(out[-t[2]])


# ---- the stream ----------------------------------------------------------------------------------------------------------------------
def encode(tokens, blocks, bw=None, out=None):
    """tokens cut into the deflate blocks `blocks` -> (raw deflate bytes, log).  bw / out: go on in a stream begun with low-level calls."""
    bw, out = bw or BitWriter(), bytearray() if out is None else out
    log = {"tokens": [], "blocks": []}
    ti = 0
    for bi, b in enumerate(blocks):
        toks = tokens[ti:ti + b["n"]]
        assert len(toks) == b["n"]
        ti += b["n"]
        entry = {"kind": b["kind"], "bit": bw.pos, "n": b["n"], "out": len(out), "final": b.get("final", int(bi == len(blocks) - 1))}
        bw.bits(entry["final"], 1)
        bw.bits({"stored": 0, "fixed": 1, "dynamic": 2}[b["kind"]], 2)
        if b["kind"] == "stored":
            first = len(out)
            token_bytes(toks, out)
            raw = bytes(out[first:])
            assert len(raw) <= 65535
            bw.align()
            bw.bits(len(raw), 16)
            bw.bits(len(raw) ^ 0xFFFF, 16)
            bw.raw(raw)
        else:
            ll, d = (FIXED_LL, FIXED_D) if b["kind"] == "fixed" else (b["ll"], b["d"])
            if b["kind"] == "dynamic":
                entry.update(dynamic_header(bw, ll, d, b.get("hclen"), b.get("clenc", "greedy")), ll=list(ll), d=list(d))
            lc, dc = canonical(ll), canonical(d)
            for t in toks:
                at = bw.pos
                if t[0] == "lit":
                    bw.bits(*lc[t[1]])
                    log["tokens"].append((at, bi, -1, t[1], lc[t[1]][1], 0, 0, 0))
                else:
                    ls, leb, lev = len_symbol(t[1])
                    ds, deb, dev = dist_symbol(t[2])
                    bw.bits(*lc[ls])
                    bw.bits(lev, leb)
                    bw.bits(*dc[ds])
                    bw.bits(dev, deb)
                    log["tokens"].append((at, bi, t[1], t[2], lc[ls][1], leb, dc[ds][1], deb))
            token_bytes(toks, out)
            entry["eob"] = bw.pos
            bw.bits(*lc[256])
        entry["bytes"] = len(out) - entry["out"]
        log["blocks"].append(entry)
    assert ti == len(tokens)
    bw.align()
    log["data"] = bytes(out)
    return bytes(bw.out), log


def bgzf(payload, data, isize=None):
    """a raw deflate payload as a BGZF block (SAM spec 4.1): header with BSIZE, CRC-32 of `data`, ISIZE (default len(data))"""
    assert len(payload) + 26 <= 65536, len(payload)
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(payload) + 25) + payload +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data) if isize is None else isize))


def plain_recipe(block, policy="nearest", plan=None, layout=None, **shape):
    """recipe for rewrite_bam: BGZF blocks of `block` inflated bytes; plan: {block index: [(offset, len, dist)]}; layout(tokens, k) ->
    deflate blocks (default: one dynamic block with lengths_for(tokens, **shape))"""
    def recipe(data, k):
        tokens = tokenize(data, policy, (plan or {}).get(k, ()))
        if layout:
            blocks = layout(tokens, k)
        else:
            ll, d = lengths_for(tokens, **{key: shape[key] for key in ("ll", "d") if key in shape})
            blocks = [dict(kind="dynamic", n=len(tokens), ll=ll, d=d, **{key: v for key, v in shape.items() if key in ("hclen", "clenc")})]
        return encode(tokens, blocks)
    recipe.block = block
    return recipe


def rewrite_bam(src_path, dst_path, recipe):
    """The inflated stream of the BAM at src_path, cut into BGZF blocks of recipe.block inflated bytes (records straddle them), each
    written as recipe(data, k) -> (payload, log) says; the end-of-file block stays htslib's.  -> the logs, one per block, with the
    block's place: "cin" (payload's first byte in the file), "clen", "uout", "ulen"."""
    stream = gzip.decompress(open(src_path, "rb").read())
    logs = []
    with open(dst_path, "wb") as fh:
        for k, o in enumerate(range(0, len(stream), recipe.block)):
            data = stream[o:o + recipe.block]
            payload, log = recipe(data, k)
            assert log["data"] == data, ("the tokens do not give the block's bytes", k)
            log.update(cin=fh.tell() + 18, clen=len(payload), uout=o, ulen=len(data))
            fh.write(bgzf(payload, data))
            logs.append(log)
        fh.write(EOF_BLOCK)
    return logs
