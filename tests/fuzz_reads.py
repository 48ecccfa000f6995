"""Random reads with arbitrary CIGARs (every op of SAM spec §4.2: M I D N S H P = X), odd SEQ
content (N, IUPAC codes, '=', SEQ '*'), flags and placements — for differential tests between
the column-major Python emulator, the read-major C oracle and the HIP kernels.  random_cigar's CIGARs are structured ([H][S] core
[S][H], every op at least one base long, op codes 0-8); the shapes a BAM file may hold and no aligner writes — ops in any order, ops of
length 0, the reserved op codes, query totals far from len(SEQ) — are tests/odd_cigars.py's."""
import numpy as np

from tests import synth_small as ss

_BASES = "ACGT"
_ODD = "NRYKM="


def random_cigar(rng, long_reads=False):
    """A structurally valid CIGAR: [H][S] core [S][H], core = ops over M I D N P = X."""
    n_core = int(rng.integers(1, 9))
    core = []
    last = None
    for _ in range(n_core):
        op = "MMMM=XIDDNP"[int(rng.integers(0, 11))]
        if op == last and op in "MIDNP=X" and rng.random() < 0.7:
            continue
        ln = int(rng.integers(1, 400 if long_reads and op in "MN" else 12 if op in "IDP" else 40))
        core.append((ln, op))
        last = op
    if not core:
        core = [(int(rng.integers(1, 30)), "M")]
    pre, post = [], []
    if rng.random() < 0.2:
        pre.append((int(rng.integers(1, 5)), "H"))
    if rng.random() < 0.3:
        pre.append((int(rng.integers(1, 9)), "S"))
    if rng.random() < 0.3:
        post.append((int(rng.integers(1, 9)), "S"))
    if rng.random() < 0.2:
        post.append((int(rng.integers(1, 5)), "H"))
    return pre + core + post


def random_specs(rng, n, L, long_reads=False):
    """-> list of read dicts (synth_small.reads_from_spec's input), unsorted."""
    reads = []
    for _ in range(n):
        cig = random_cigar(rng, long_reads)
        qlen = sum(l for l, op in cig if op in "MIS=X")
        r = rng.random()
        if r < 0.03:
            seq = "*"
        elif r < 0.06 and qlen > 3:
            seq = "".join(_BASES[int(k)] for k in rng.integers(0, 4, qlen - int(rng.integers(1, 3))))   # SEQ shorter than the CIGAR says
        else:
            seq = "".join((_ODD[int(rng.integers(0, len(_ODD)))] if rng.random() < 0.03 else _BASES[int(rng.integers(0, 4))])
                          for _ in range(qlen))
            if not seq:
                seq = "*"
        span = sum(l for l, op in cig if op in "MDN=X")
        pos = int(rng.integers(0, max(1, L - min(span, L // 2))))
        flag = int(rng.choice([0, 16, 0, 16, 4, 0x100, 0x400, 1, 3, 0x10 | 0x200]))
        reads.append({"pos": pos, "flag": flag, "cigar": "".join("%d%s" % t for t in cig), "seq": seq,
                      "qual": int(rng.integers(0, 41)), "tid": -1 if rng.random() < 0.01 else 0})
    return reads


def random_reads(rng, n, L, long_reads=False, sort=True):
    reads = random_specs(rng, n, L, long_reads)
    if sort:
        reads.sort(key=lambda r: r["pos"])
    return ss.reads_from_spec({"reads": reads})


# ------------------------------------------------------------------------------------------------------------- insert tokens
# Read sets for the insert-token paths (Events.ExtractInserts, Events.py:47-82: pysam's default region pile-up): named reads with
# per-base qualities around min_base_quality, the flags the samtools stepper filters, overlapping mate pairs with random CIGARs on
# both mates, and planted insertion sites that make columns real candidates.
_IUPAC = "RYKMSWBDHVN"
_EDGE_Q = (12, 13)                       # min_base_quality = 13: one below, exactly on it


def _span(cig):
    return sum(l for l, op in cig if op in "MDN=X")


def _qlen(cig):
    return sum(l for l, op in cig if op in "MIS=X")


def _cigar_text(cig):
    return "".join("%d%s" % t for t in cig)


def _quals(rng, n, floor=0):
    """per-base qualities 0-41 (12 and 13 often), or a read without QUAL (every byte 0xFF)"""
    if n and floor == 0 and rng.random() < 0.04:
        return [255] * n
    q = rng.integers(floor, 42, n)
    edge = rng.random(n) < 0.25
    q[edge] = np.maximum(rng.choice(_EDGE_Q, int(edge.sum())), floor)
    return [int(x) for x in q]


def _bases(rng, n, odd=0.0):
    return "".join((_IUPAC[int(rng.integers(0, len(_IUPAC)))] if rng.random() < odd / 2 else "=") if rng.random() < odd
                   else _BASES[int(rng.integers(0, 4))] for _ in range(n))


def _seq_for(rng, ref, pos, cig, odd=0.01):
    """the query of a read placed at `pos` with CIGAR `cig`: reference bases on M / = / X (a few mutated), random ones elsewhere"""
    out, x = [], pos
    for l, op in cig:
        if op in "M=X":
            for k in range(l):
                b = ref[x + k] if 0 <= x + k < len(ref) else _BASES[int(rng.integers(0, 4))]
                out.append(_bases(rng, 1, 1.0) if rng.random() < odd else (_BASES[int(rng.integers(0, 4))] if rng.random() < 0.03 else b))
            x += l
        elif op in "IS":
            out.append(_bases(rng, l, odd))
        elif op in "DN":
            x += l
    return "".join(out)


def _read(rng, ref, pos, cig, flag, name, tid=0, floor=0, seq=None, **mate):
    seq = _seq_for(rng, ref, pos, cig) if seq is None else seq
    r = {"pos": int(pos), "flag": int(flag), "cigar": _cigar_text(cig), "seq": seq or "*", "name": name, "tid": tid,
         "qual": _quals(rng, len(seq), floor) if seq and seq != "*" else []}
    r.update(mate)
    return r


def _shorten(rng, r, how):
    """a mate without its SEQ ('*') or with fewer bases than its CIGAR says"""
    if how == "star" or len(r["seq"]) < 3:
        r["seq"], r["qual"] = "*", []
    else:
        n = int(rng.integers(1, len(r["seq"])))
        r["seq"], r["qual"] = r["seq"][:n], r["qual"][:n]


def _pairs(rng, ref, L, n, tag, tid, n_ref):
    """overlapping mate pairs, random CIGARs on both mates (deletions and ref-skips on shared columns: the probe path), some with
    the mate on another reference, an inconsistent mpos < pos, a mate without SEQ or with a short SEQ, or not properly paired"""
    out = []
    for k in range(n):
        c1, c2 = random_cigar(rng), random_cigar(rng)
        s1 = _span(c1)
        p1 = int(rng.integers(0, max(1, L - s1)))
        p2 = p1 + int(rng.integers(0, max(1, min(s1, 40))))
        e2 = p2 + _span(c2)
        tlen = max(p1 + s1, e2) - p1
        kind = rng.random()
        f1, f2 = (99, 147) if rng.random() < 0.5 else (163, 83)
        if kind < 0.06:
            f1, f2 = f1 & ~2, f2 & ~2                           # paired, not proper: orphans to the samtools stepper
        elif kind < 0.1:
            f1, f2 = f1 | 8, f2                                 # "mate unmapped" on the first
        name = "%sp%d" % (tag, k)
        mt = tid if kind < 0.9 or n_ref < 2 else (tid + 1) % n_ref          # (a mate on another reference: not an overlapping pair)
        m1 = p2 if rng.random() > 0.05 else max(0, p1 - int(rng.integers(1, 20)))        # (mpos < pos: never waits for its mate)
        a = _read(rng, ref, p1, c1, f1, name, tid, mtid=mt, mpos=m1, tlen=tlen)
        b = _read(rng, ref, p2, c2, f2, name, tid, mtid=mt, mpos=p1, tlen=-tlen)
        if rng.random() < 0.5 and b["seq"] != "*":             # the second mate copies the first where they overlap: bases agree
            b["seq"] = _seq_like(rng, a, b)
            b["qual"] = _quals(rng, len(b["seq"]))
        if rng.random() < 0.2:
            _shorten(rng, a if rng.random() < 0.5 else b, "star" if rng.random() < 0.5 else "short")
        out += [a, b]
    return out


def _seq_like(rng, a, b):
    """b's query with the bases of a where both have a matched base on the same reference position"""
    from tests import synth_small as ss
    def matched(r):
        m, x, y = {}, r["pos"], 0
        for op, l in ss.parse_cigar(r["cigar"]):
            if op in (0, 7, 8):
                for j in range(l):
                    m[x + j] = y + j
            if op in (0, 2, 3, 7, 8):
                x += l
            if op in (0, 1, 4, 7, 8):
                y += l
        return m
    ma, mb = matched(a), matched(b)
    s = list(b["seq"])
    for rp, qb in mb.items():
        qa = ma.get(rp)
        if qa is not None and qa < len(a["seq"]) and qb < len(s):
            s[qb] = a["seq"][qa]
    return "".join(s)


_SHAPES = ("MI", "MI", "MPI", "MIPI", "DI", "NI", "MDD", "SIM", "MI_past_seq", "MI_end")


def _site(rng, ref, L, c, tag, tid, n, shape, ins_len, tie):
    """n reads planted on 0-based column c: an insertion behind it in the given CIGAR shape (or a double deletion: "MDD"); with `tie`
    two insertion variants of exactly equal count (first seen wins the vote)"""
    out = []
    variants = []
    while len(variants) < (2 if tie else 1 + int(rng.integers(0, 2))):
        v = _bases(rng, ins_len, 0.0 if tie or rng.random() < 0.5 else 0.25)     # ('=' would split a tie by strand)
        if v not in variants:
            variants.append(v)
    for k in range(n):
        ins = variants[k % len(variants)] if tie else variants[0 if rng.random() < 0.8 else -1]
        rev = rng.random() < 0.5
        flag = 16 if rev else 0
        a = int(rng.integers(1, min(c, 30) + 1)) if c > 0 else 1
        b = int(rng.integers(1, 30))
        pos = c - a + 1
        if shape == "MI_end":                                  # the insertion is the CIGAR's last query op (column L: nothing behind)
            b = 0
        gap = int(rng.integers(1, 6))
        if shape in ("DI", "NI"):                              # the insertion behind a deletion / ref-skip: '*+' / '>+' on its last column
            a = max(1, a - gap)
            pos = c - a - gap + 1
            if pos < 0:
                pos, a = 0, 1
                gap = c
                if gap < 1:
                    shape = "MI"
        cig = [(a, "M")]
        if shape == "MPI":
            cig += [(int(rng.integers(1, 4)), "P"), (ins_len, "I")]
        elif shape == "MIPI" and ins_len > 1:
            h = int(rng.integers(1, ins_len))
            cig += [(h, "I"), (int(rng.integers(1, 4)), "P"), (ins_len - h, "I")]
        elif shape in ("DI", "NI"):
            cig += [(gap, "D" if shape == "DI" else "N"), (ins_len, "I")]
        elif shape == "MDD":
            cig += [(gap, "D"), (int(rng.integers(1, 4)), "D")]
        elif shape == "SIM":                                   # an insertion in front of the first matched base: on no column
            cig = [(int(rng.integers(1, 5)), "S"), (ins_len, "I"), (a, "M")]
        else:
            cig += [(ins_len, "I")]
        if b:
            cig.append((b, "M"))
        if rng.random() < 0.2 and shape != "SIM":
            cig.append((int(rng.integers(1, 5)), "S"))
        seq = []
        x = pos
        for l, op in cig:
            if op in "M=X":
                seq.append(ref[x:x + l] + "A" * max(0, x + l - len(ref)))
                x += l
            elif op == "I":
                seq.append(ins[:l] if l == ins_len else (ins[:h] if len(seq) == 1 else ins[h:]))
            elif op == "S":
                seq.append(_bases(rng, l))
            elif op in "DN":
                x += l
        seq = "".join(seq)
        if shape == "MI_past_seq":                             # SEQ ends inside the insertion: its bases beyond SEQ print as 'N'
            seq = seq[:a + int(rng.integers(0, ins_len))]
        out.append(_read(rng, ref, pos, cig, flag, "%ss%d_%d" % (tag, c, k), tid, floor=13 if tie else 0, seq=seq))
    return out


def token_specs(rng, ref, tid=0, tag="", n_ref=2, background=None, n_pairs=None, n_sites=None, deep=False, overhang=True):
    """-> list of read dicts (synth_small.reads_from_spec's input) for one reference `ref`, sorted by position: background reads
    (random CIGARs, every filtered flag, supplementary, orphans, unplaced reads at the end), overlapping mate pairs and planted
    insertion sites (lengths 1-12, 12, 13 and 40+; '=' / IUPAC codes on either strand; the CIGAR shapes of _SHAPES; exact ties).
    deep: one start position with more than 8 000 reads, filtered ones among them (max_depth).  overhang: a few reads run past
    the reference's end."""
    L = len(ref)
    out = []
    nb = L // 3 if background is None else background
    for k in range(nb):
        cig = random_cigar(rng)
        s = _span(cig)
        pos = int(rng.integers(0, max(1, L - s + (8 if overhang else 0))))
        flag = int(rng.choice([0, 16, 0, 16, 0x100, 0x200, 0x400 | 16, 0x800, 0x800 | 16, 1, 1 | 16 | 0x40, 3 | 0x40, 4]))
        out.append(_read(rng, ref, pos, cig, flag, "%sb%d" % (tag, k), tid))
        if flag & 0x800 and rng.random() < 0.5:                # (a supplementary record shares its name: one name three times)
            out[-1]["name"] = "%sp%d" % (tag, int(rng.integers(0, max(1, L // 20))))
    out += _pairs(rng, ref, L, L // 20 if n_pairs is None else n_pairs, tag, tid, n_ref)
    ns = max(len(_SHAPES), L // 60) if n_sites is None else n_sites
    lens = [int(rng.integers(1, 12)), 12, 13, int(rng.integers(40, 61))]
    for k in range(ns):
        c = int(rng.integers(1, L - 1))
        if k == 0:
            c = 0                                              # column 1
        elif k == 1:
            c = L - 1                                          # column L
        shape = "MI_end" if k == 1 else _SHAPES[k % len(_SHAPES)]
        tie = k % 4 == 2
        out += _site(rng, ref, L, c, tag, tid, 2 * int(rng.integers(20, 31)) if tie else int(rng.integers(8, 41)), shape, lens[k % len(lens)], tie)
    if deep:
        c = L // 2
        for k in range(8600):
            flag = 0x400 if k % 37 == 5 else 0x100 if k % 53 == 7 else 16 if k % 3 else 0
            cig = [(5, "M"), (2, "I"), (5, "M")] if k < 4000 else [(12, "M")]
            out.append(_read(rng, ref, c - 4, cig, flag, "%sd%d" % (tag, k), tid, seq=ref[c - 4:c + 1] + "GT" + ref[c + 1:c + 6] if k < 4000 else None))
    out.sort(key=lambda r: r["pos"])
    for k in range(3):                                          # unplaced: no reference, at the end of a sorted file
        r = _read(rng, ref, 0, [(20, "M")], 0, "%su%d" % (tag, k), -1)
        r["pos"] = -1
        out.append(r)
    for r in out:
        if r["tid"] < 0:
            r["mtid"], r["mpos"] = -1, -1
    return out
