"""BGZF members that zlib's inflate refuses, and the device decoder must: one damaged member in an otherwise good file, written with the
low-level calls of tests/deflate_writer.py.  Each case names the line of the decoder that refuses it (as of this commit) and what the
kernels have touched by then; none of them reads or writes global memory through a value taken from the damaged stream before that line.

Common to all: bgzf_symbols stages the payload and decodes symbols from LDS; tokens go to the block's own token range, guarded by tok_cap
(bgzf_symbols.hip:197, :498-501 `room`, :878).  A block whose status is not ST_OK gets no tokens in bgzf_copy (bgzf_copy.hip:274-275: ntok = 0)
and writes nothing but its status words; tcmi_bam_chain_check (bgzf_host.cpp:110-112) turns ST_BAD_STREAM / ST_BAD_LENGTH into E_FORMAT.

  before-1, before-32768    a match whose source starts before the block's first byte.  The symbols are valid, the token is written.
                            bgzf_copy.hip:498-499: `dist + a0 <= dst` fails, so the match is neither `plain` nor `far_ok` (kind 2 in vB): it is
                            not `far_now` (:516, no fetch from `out` in the set-up of bgzf_copy<true, *>, :518-580), not `teamable` (:592: no
                            team slot, srcend = ~0), and TCMI_LM_ASM hands kind 2 to C++ (:110-111) -> copy_any -> :399 `dist + a0 > at`: bad,
                            before `out + (at - dist)` is formed (:401).  The raw-token batch calls copy_any directly (:471).  -> :741
  ll-286, ll-287            fixed block, literal/length symbols 286 / 287: make_entry gives no entry (bgzf_device.h:97), the root slot is 0, the
  dist-30, dist-31          long-code look-up finds no code (bgzf_symbols.hip:148-151; LLl / LLd :571-589, :630-648): the lane is dead where it
                            stands, the chain ends on a dead lane in front of the payload's end -> :863.  (bgzf_device.h:105 for 30 / 31)
  hlit-287, hlit-288        dynamic block with HLIT / HDIST beyond 286 / 30 (the only way to name those symbols there) -> bgzf_symbols.hip:220
  hdist-31, hdist-32
  over-cl, over-ll, over-d  an over-subscribed code-length / literal / distance code: build_table's `left < 0` (bgzf_device.h:146-147)
                            -> bgzf_symbols.hip:230, :338, :339.  The table it has filled by then is LDS, indexed below the symbol count.
  no-eob, hclen-4           no end-of-block code (hclen-4: a header of four code-length codes can write no length but 0) -> bgzf_symbols.hip:334
  first-16                  the first code-length symbol is a repeat of nothing -> bgzf_symbols.hip:309 (`first && lane == 0 && v == 16`)
  repeat-past               a repeat that runs past HLIT + HDIST -> bgzf_symbols.hip:309 (`at + rep > total`), before the store at :313
  len-nlen                  a stored block whose NLEN is not ~LEN -> bgzf_symbols.hip:192
  type-3                    block type 3 -> bgzf_symbols.hip:207
  truncated                 the payload ends before the end-of-block code (the last bits are ones: no code of the fixed tree): the lanes stop at
                            the payload's end (bgzf_symbols.hip:433-436 LDend, :494-495 LDover) -> :863
  isize-small, isize-large  ISIZE one too small / too large over a good stream: bgzf_copy.hip:453 / :460 / :470 / :487 `> vend` before the batch
                            is written, :742 `op != vend`.  The output is sized by the ISIZEs, the block stays inside its own range."""
import os
import zlib

from tests import deflate_writer as dw
from tests import foreign_files as ff

BLOCK = 5000


def fixed_header(bw, final=1):
    bw.bits(final, 1)
    bw.bits(1, 2)
    return dw.canonical(dw.FIXED_LL), dw.canonical(dw.FIXED_D + [5, 5])       # (FIXED_LL has the codes of 286 and 287; + those of 30, 31)


def literals(bw, codes, data):
    for b in data:
        bw.bits(*codes[b])


def done(bw):
    bw.align()
    return bytes(bw.out)


def match_before(at, dist):
    def make(data):
        bw = dw.BitWriter()
        lc, dc = fixed_header(bw)
        literals(bw, lc, data[:at])
        bw.bits(*lc[257])                           # length 3
        ds, eb, ev = dw.dist_symbol(dist)
        bw.bits(*dc[ds])
        bw.bits(ev, eb)
        literals(bw, lc, data[at + 3:])
        bw.bits(*lc[256])
        return done(bw), len(data)
    return make


def bad_symbol(ll_sym=None, d_sym=None):
    def make(data):
        bw = dw.BitWriter()
        lc, dc = fixed_header(bw)
        literals(bw, lc, data[:100])
        bw.bits(*lc[ll_sym if ll_sym else 257])
        if d_sym:
            bw.bits(*dc[d_sym])
        literals(bw, lc, data[100:])
        bw.bits(*lc[256])
        return done(bw), len(data)
    return make


def dynamic_counts(hlit, hdist):
    def make(data):
        bw = dw.BitWriter()
        bw.bits(1, 1)
        bw.bits(2, 2)
        bw.bits(hlit - 257, 5)
        bw.bits(hdist - 1, 5)
        bw.bits(15, 4)
        bw.bits(0, 19 * 3 + 64)                     # (the counts are refused before anything behind them is looked at)
        return done(bw), len(data)
    return make


def header(cl, symbols, hlit=257, hdist=1, count=19):
    """a dynamic block's header by hand: code-length code lengths `cl` (by symbol), then `symbols` [(symbol, extra bits, value)]"""
    def make(data):
        bw = dw.BitWriter()
        bw.bits(1, 1)
        bw.bits(2, 2)
        bw.bits(hlit - 257, 5)
        bw.bits(hdist - 1, 5)
        bw.bits(count - 4, 4)
        for i in range(count):
            bw.bits(cl[dw.CL_ORDER[i]], 3)
        codes = dw.canonical(cl)
        for s, eb, ev in symbols:
            bw.bits(*codes[s])
            bw.bits(ev, eb)
        bw.bits(0xFFFFFFFF, 32)                     # (whatever follows is never looked at)
        return done(bw), len(data)
    return make


def cl_of(*lens):
    cl = [0] * 19
    for s, l in lens:
        cl[s] = l
    return cl


def stored_bad_nlen(data):
    bw = dw.BitWriter()
    bw.bits(1, 1)
    bw.bits(0, 2)
    bw.align()
    bw.bits(len(data), 16)
    bw.bits((len(data) ^ 0xFFFF) ^ 0x0100, 16)
    bw.raw(data)
    return done(bw), len(data)


def type_3(data):
    bw = dw.BitWriter()
    bw.bits(1, 1)
    bw.bits(3, 2)
    bw.bits(0, 29)
    bw.raw(data)
    return done(bw), len(data)


def truncated(data):
    bw = dw.BitWriter()
    lc, _ = fixed_header(bw)
    literals(bw, lc, data)
    bw.bits(0xFF >> (bw.n or 8), (8 - bw.n) % 8)    # ones up to the byte's end: the start of a 9-bit code, not an end-of-block code
    return bytes(bw.out), len(data)


def good_with_isize(delta):
    def make(data):
        tokens = dw.tokenize(data, "nearest")
        ll, d = dw.lengths_for(tokens)
        return dw.encode(tokens, [dict(kind="dynamic", n=len(tokens), ll=ll, d=d)])[0], len(data) + delta
    return make


REFUSED = {
    "before-1": match_before(7, 8), "before-32768": match_before(0, 32768),
    "ll-286": bad_symbol(ll_sym=286), "ll-287": bad_symbol(ll_sym=287), "dist-30": bad_symbol(d_sym=30), "dist-31": bad_symbol(d_sym=31),
    "hlit-287": dynamic_counts(287, 1), "hlit-288": dynamic_counts(288, 1), "hdist-31": dynamic_counts(257, 31), "hdist-32": dynamic_counts(257, 32),
    "over-cl": header(cl_of((0, 1), (8, 1), (9, 1)), []),
    # 257 lengths of 7 (sum 2^-7 * 257 > 1) and no distance code; one length of 1 and three distance lengths of 1
    "over-ll": header(cl_of((7, 1), (0, 2), (16, 2)), [(7, 0, 0)] + [(16, 2, 3)] * 42 + [(7, 0, 0)] * 4 + [(0, 0, 0)]),
    "over-d": header(cl_of((1, 1), (0, 2), (18, 2)), [(1, 0, 0), (18, 7, 127), (18, 7, 106), (1, 0, 0), (1, 0, 0), (1, 0, 0), (1, 0, 0)], hdist=3),
    "no-eob": header(cl_of((8, 1), (0, 1)), [(8, 0, 0)] * 256 + [(0, 0, 0)] * 2),
    "hclen-4": header(cl_of((0, 1), (18, 1)), [(18, 7, 127), (18, 7, 109)], count=4),
    "first-16": header(cl_of((16, 1), (8, 2), (0, 2)), [(16, 2, 0)] + [(8, 0, 0)] * 255 + [(0, 0, 0)]),
    "repeat-past": header(cl_of((8, 1), (16, 2), (0, 2)), [(8, 0, 0)] * 256 + [(16, 2, 3)]),
    "len-nlen": stored_bad_nlen, "type-3": type_3, "truncated": truncated,
    "isize-small": good_with_isize(-1), "isize-large": good_with_isize(+1),
}
WHERE = ("zero", "first", "middle")                 # block 0 (with the BAM header: the host inflates it), the block behind a header-only one, a middle one


def build(tmp, name, where):
    """-> (path, index of the damaged block, blocks without the end-of-file marker)"""
    stream, _ = ff.source_stream(0.5, 48)
    head = 12 + int.from_bytes(stream[4:8], "little")
    head += 8 + int.from_bytes(stream[head:head + 4], "little")
    cuts = ([0, head] if where == "first" else [0]) + list(range(head if where == "first" else 0, len(stream), BLOCK))[1:] + [len(stream)]
    k = {"zero": 0, "first": 1, "middle": (len(cuts) - 1) // 2}[where]
    good = dw.plain_recipe(BLOCK)
    path = os.path.join(str(tmp), "%s.%s.bam" % (name, where))
    with open(path, "wb") as fh:
        for j, (a, b) in enumerate(zip(cuts, cuts[1:])):
            data = bytes(stream[a:b])
            if j == k:
                payload, isize = REFUSED[name](data)
                fh.write(dw.bgzf(payload, data, isize))
            else:
                fh.write(dw.bgzf(good(data, j)[0], data))
        fh.write(dw.EOF_BLOCK)
    return path, k, len(cuts) - 1
