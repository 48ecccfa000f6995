"""Record specs of the tests (dicts of pos, flag, cigar, seq, qual, name, tid, mapq) and what is made of them: their arrays, the read
filter's rule on them, the mixed fixture of ~3 000 records that most command-line tests run on, a two-contig set, a pair of files "A
under the filter / B without the failing records", and the oracle's count matrix under a base-quality floor.  No tests in here."""
import functools

import numpy as np

from oracle import tc_oracle as orc
from tests import fuzz_reads as fz
from tests import synth_small as ss
from trueconsense_amd import synthetic as sy
from trueconsense_amd.io import bamwriter

L = 2000
MAPQS = (0, 1, 19, 20, 21, 60, 255)
BITS = ((0x100, 0.1), (0x200, 0.1), (0x400, 0.25), (0x800, 0.1), (0x2, 0.75))      # FLAG bit, how often it is ORed in
FILTERS = {"mapq": (20, 0, 0), "require": (0, 0x2, 0), "exclude": (0, 0, 0x500), "all": (1, 0x2, 0x400)}
FLAGS = ["--min-mapq", "1", "--require-flags", "0x2", "--exclude-flags", "1024"]       # FILTERS["all"] on the command line


def passes(r, f):
    return r["mapq"] >= f[0] and (r["flag"] & f[1]) == f[1] and (r["flag"] & f[2]) == 0


def randomise(rng, specs):
    """MAPQ from MAPQS and random filterable FLAG bits onto every record"""
    for r in specs:
        r["mapq"] = int(rng.choice(MAPQS))
        for bit, p in BITS:
            if rng.random() < p:
                r["flag"] |= bit
    return specs


def arrays(specs):
    d = ss.reads_from_spec({"reads": specs})
    d["mapq"] = np.array([r["mapq"] for r in specs], np.uint8)
    return d


def kept(specs, f):
    """B's records and the number that failed; the fixture's condition: 20 - 60 % fail, both classes there"""
    b = [r for r in specs if passes(r, f)]
    n_fail = len(specs) - len(b)
    assert b and n_fail and 0.2 <= n_fail / len(specs) <= 0.6, (n_fail, len(specs))
    return b, n_fail


def background(rng, ref, n, tid=0, tag=""):
    """reads of 30 - 150 bases: plain, with an insertion, a deletion or soft clips; a few unmapped (FLAG 0x4) ones among them"""
    out = []
    for k in range(n):
        ln = int(rng.integers(30, 151))
        pos = int(rng.integers(0, len(ref) - ln - 8))
        a = int(rng.integers(5, ln - 10))
        shape = rng.random()
        if shape < 0.7:
            cig = [(ln, "M")]
        elif shape < 0.8:
            cig = [(a, "M"), (int(rng.integers(1, 4)), "I"), (ln - a, "M")]
        elif shape < 0.9:
            cig = [(a, "M"), (int(rng.integers(1, 6)), "D"), (ln - a, "M")]
        else:
            cig = [(3, "S"), (ln, "M"), (2, "S")]
        flag = (16 if rng.random() < 0.5 else 0) | (4 if rng.random() < 0.02 else 0)
        out.append(fz._read(rng, ref, pos, cig, flag, "%sr%d" % (tag, k), tid))
    return out


@functools.lru_cache(maxsize=None)
def mixed():
    """-> (reference, GFF rows, A's records): ~3 000 background reads on L = 2 000 and three planted insertions (insert candidates)"""
    rng = np.random.default_rng(20240)
    ref, orfs = sy.make_reference(seed=3, L=L, cds=[(100, 900), (1100, 1900)])
    specs = background(rng, ref, 2400)
    for c, n_ins in ((400, 2), (1000, 13), (1500, 5)):
        specs += fz._site(rng, ref, L, c, "", 0, 200, "MI", n_ins, False)
    specs.sort(key=lambda r: r["pos"])
    return ref, orfs, randomise(rng, specs)


def write_pair(tmp_path, specs, f, tag="", **kw):
    """A and B as files -> (path A, path B, B's arrays, failing records)"""
    b, n_fail = kept(specs, f)
    pa, pb = str(tmp_path / (tag + "A.bam")), str(tmp_path / (tag + "B.bam"))
    kw.setdefault("block", 4096)
    kw.setdefault("ref_len", L)
    bamwriter.write_bam(pa, arrays(specs), **kw)
    rb = arrays(b)
    bamwriter.write_bam(pb, rb, **kw)
    return pa, pb, rb, n_fail


def two_contigs():
    """-> ([(name, sequence)], [(name, orfs)], records): 500 background reads and a planted insertion on each of c0 (1 500) and c1 (1 200)"""
    rng = np.random.default_rng(8)
    recs, rows, specs = [], [], []
    for t, (name, ln) in enumerate((("c0", 1500), ("c1", 1200))):
        ref, orfs = sy.make_reference(seed=30 + t, L=ln, cds=[(100, 700)])
        recs.append((name, ref))
        rows.append((name, orfs))
        part = background(rng, ref, 500, tid=t, tag=name)
        part += fz._site(rng, ref, ln, 800, name, t, 100, "MI", 3, False)
        specs += sorted(part, key=lambda r: r["pos"])
    for r in specs:
        r["mapq"] = 60
    return recs, rows, specs


def mk(rng, pos, cig, qual, name, seq=None, flag=0):
    """one record by hand: cig = [(n, op)]; random bases and qualities around the floor unless given"""
    n = sum(k for k, op in cig if op in "MIS=X")
    if seq is None:
        seq = "".join("ACGT"[int(k)] for k in rng.integers(0, 4, n))
    if qual is None:
        qual = [int(x) for x in rng.choice((12, 13, 30, 2, 41), len(seq))]
    qual = list(qual) if seq != "*" else []
    assert seq == "*" or len(qual) == len(seq), (name, len(qual), len(seq))
    return {"pos": int(pos), "flag": flag, "cigar": "".join("%d%s" % t for t in cig), "seq": seq, "qual": qual, "name": name, "tid": 0, "mapq": 60}


def record_bytes(rd, i):
    return 36 + int(rd["name_off"][i + 1] - rd["name_off"][i]) + 1 + 4 * int(rd["cigar_off"][i + 1] - rd["cigar_off"][i]) + \
        (int(rd["l_qseq"][i]) + 1) // 2 + int(rd["l_qseq"][i])


def seq_starts(rd, inflated):
    """byte offset of every record's SEQ in the inflated stream (the header takes what the records do not)"""
    sizes = [record_bytes(rd, i) for i in range(int(rd["n_reads"]))]
    at = inflated - sum(sizes)
    out = []
    for i, n in enumerate(sizes):
        out.append(at + 36 + int(rd["name_off"][i + 1] - rd["name_off"][i]) + 1 + 4 * int(rd["cigar_off"][i + 1] - rd["cigar_off"][i]))
        at += n
    return out


def oracle_counts(rd, q, n_pos):
    """the yardstick of the base-quality floor: int32 [n_pos, 7] (coverage, A, T, C, G, X, I)"""
    out = np.zeros((n_pos, 7), np.int32)
    for c, toks in orc.pileup_columns(rd, min_base_quality=q).items():
        out[c] = orc.tally_tokens(toks)
    return out
