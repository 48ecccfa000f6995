"""Valid BAM files beyond the capacities the one-sync file path (pk_index + pk_place + pk_pack, tcmi_bamfile_step) sizes its device
arrays for before anybody has seen the file, one per rung of the ladder behind it (csrc/pack_caps.h: pk_one_sync_caps and the
PKF_* flags; tests/test_pack_caps.py holds the header's own numbers against the restatement below):

    rec_cap    min(inflated / 64 + 1024, inflated / 36 + 16, inflated / hint * 5 / 4 + 8192)     PKF_REC_OVF    0x800
    word_cap   inflated / 24 + 8 * rec_cap + 64                                                   PKF_WORD_OVF   64
    chunk_cap  min(rec_cap, 4 * n_wg + (ref_len[0] + 65536) / 128 + 64)                           PKF_CHUNK_OVF  16
    event_cap  max(1 << 20, rec_cap / 2)                                                          PKF_EVENT_OVF  8

`hint` is the mean size of the whole records the host finds behind the header in the leading blocks it inflates FOR the header
(bgzf_host.cpp tcmi_bam_front_header; fewer than 16: none, and the context's last file stands in).  A header that ends with its block —
what bamwriter.write_bam writes unless told to fill every block to the brim — shows the host no record: the files that must carry a
hint of their own are written with split_records=True, the one that must not (stale_hint) is not.  `facts` restates those rules on the
file as written; tests/test_capacity_files.py asserts that every file is still beyond the capacity it is here for.

Plain Python on synth_small.reads_from_spec + bamwriter.write_bam: sorted, one reference carries the reads, header ref_len 5000, level 1.
Test infrastructure; nothing here is imported by the product."""
import functools
import gzip
import struct

import numpy as np

from tests import synth_small as ss
from trueconsense_amd.io import bamwriter

REF_LEN = 5000
MAXPOS = 768                    # positions of a chunk's window (TCMI_F_MAXW * 8)
N_SPARSE = 4000                 # reads of sparse_beyond_ref_len: a chunk each
# ... which is beyond chunk_cap = 4 * n_wg + 615 while the packer's grid n_wg = n_cu * wg_per_cu stays below this:
SPARSE_MAX_SLOTS = (N_SPARSE - (REF_LEN + 65536) // 128 - 64 - 1) // 4
EVENT_FLOOR = 1 << 20           # event_cap of a file of fewer than 2 M records
PKF_EVENT_OVF, PKF_CHUNK_OVF, PKF_WORD_OVF, PKF_REC_OVF = 8, 16, 64, 0x800


def _bases(rng, n):
    return "".join("ACGT"[k] for k in rng.integers(0, 4, n))


def words_of(length):
    """plane words of a kept read of `length` positions (pack_device.hip words_of)"""
    return (2 * ((length + 31) >> 5) + 2 + 3) & ~3


# ------------------------------------------------------------------------------------------------------------------------ the reads
def _long(rng, k):
    return {"pos": k, "flag": 0, "cigar": "1000S100M", "seq": _bases(rng, 1100), "name": "long%04d" % k}


def hint_too_large_specs(flag_quarter=False):
    """a: 40 reads 1000S100M (1703 bytes a record: the header's block shows the host 38 of them), then 20 000 reads 40M.
    flag_quarter: every fourth short read carries FLAG 0x400 (the read-filter case)."""
    rng = np.random.default_rng(101)
    specs = [_long(rng, k) for k in range(40)]
    for i in range(20000):
        specs.append({"pos": 40 + i // 5, "flag": 0x400 if flag_quarter and i % 4 == 1 else 0, "cigar": "40M", "seq": _bases(rng, 40), "name": "s%d" % i})
    return specs


def long_only_specs():
    """f's helper: 80 records of a's long kind as a file of its own (more than 64: the context remembers their mean size)"""
    rng = np.random.default_rng(106)
    return [_long(rng, k) for k in range(80)]


def tiny_records_specs():
    """b: 20 000 reads 1M, name r: 44 bytes a record, more records than inflated / 64 + 1024"""
    return [{"pos": i // 8, "flag": 0, "cigar": "1M", "seq": "ACGT"[(i // 8) & 3], "name": "r"} for i in range(20000)]


def wide_skips_specs(quals=None):
    """c: 20 000 reads 1M500N1M, SEQ AC, 71 bytes a record, 8 reads per start: 36 plane words each.  quals: per-read quality"""
    return [{"pos": i // 8, "flag": 0, "cigar": "1M500N1M", "seq": "AC", "name": "name%015d" % i, "qual": 30 if quals is None else int(quals[i])}
            for i in range(20000)]


def sparse_specs():
    """d: N_SPARSE reads 50M, 800 positions apart (a window holds 768): every read opens a chunk; far beyond the header's ref_len"""
    rng = np.random.default_rng(104)
    return [{"pos": 800 * i, "flag": 0, "cigar": "50M", "seq": _bases(rng, 50), "name": "d%d" % i} for i in range(N_SPARSE)]


def all_n_specs(qual=30):
    """e: 7 500 reads 150M, SEQ all N, 4 reads per start: 1 125 000 OTHER events.  qual: one value, or the 150 values of every read"""
    return [{"pos": i // 4, "flag": 0, "cigar": "150M", "seq": "N" * 150, "name": "n%d" % i, "qual": qual} for i in range(7500)]


def stale_hint_specs():
    """f: 20 000 reads 40M (behind a header of 300 references that has its blocks to itself: the file carries no hint)"""
    rng = np.random.default_rng(107)
    return [{"pos": i // 5, "flag": 0, "cigar": "40M", "seq": _bases(rng, 40), "name": "s%d" % i} for i in range(20000)]


def stale_hint_refs():
    refs = [("contig_%04d_with_a_rather_long_name_as_assemblies_have_them" % k, 1000 + k) for k in range(300)]
    refs[0] = (refs[0][0], REF_LEN)
    return refs


CASES = ("hint_too_large", "tiny_records", "wide_skips", "sparse_beyond_ref_len", "all_n", "stale_hint")
_SPECS = {"hint_too_large": hint_too_large_specs, "tiny_records": tiny_records_specs, "wide_skips": wide_skips_specs,
          "sparse_beyond_ref_len": sparse_specs, "all_n": all_n_specs, "stale_hint": stale_hint_specs, "long_only": long_only_specs}


@functools.lru_cache(maxsize=None)
def reads_of(case):
    """the case's reads as flat arrays (shared: nobody changes them)"""
    return ss.reads_from_spec({"reads": _SPECS[case]()})


def write_reads(path, reads, case):
    """the file of a case from `reads` (the case's own, or a variant of them: flags, qualities)"""
    if case == "stale_hint":
        bamwriter.write_bam(str(path), reads, level=1, refs=stale_hint_refs())
    else:
        bamwriter.write_bam(str(path), reads, "ref", REF_LEN, level=1, split_records=True)
    return str(path)


def write(path, case):
    return write_reads(path, reads_of(case), case)


# ------------------------------------------------------------------------------------------------------------------------ the rules, restated
def facts(path):
    """What decides the file's way through the one-sync path, from the file as written (zlib + a walk of the record chain)."""
    raw = open(path, "rb").read()
    blocks, at = [], 0                                              # inflated length of every BGZF block
    while at < len(raw):
        bsize, = struct.unpack_from("<H", raw, at + 16)
        blocks.append(struct.unpack_from("<I", raw, at + bsize + 1 - 4)[0])
        at += bsize + 1
    s = gzip.decompress(raw)
    assert sum(blocks) == len(s)
    l_text, = struct.unpack_from("<i", s, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", s, o)
    o += 4
    ref_len = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", s, o)
        ref_len.append(struct.unpack_from("<i", s, o + 4 + l_name)[0])
        o += 4 + l_name + 4
    first_record = o
    # the hint: the leading blocks the header needs, and the whole records behind the header in them (16 at least)
    got = 0
    for ulen in blocks:
        if got >= first_record:
            break
        got += ulen
    at, cnt = first_record, 0
    while at + 4 <= got:
        bs, = struct.unpack_from("<i", s, at)
        if bs < 32 or at + 4 + bs > got:
            break
        at += 4 + bs
        cnt += 1
    hint = (at - first_record) // cnt if cnt >= 16 else 0
    # the records: per kept read its reference span; events: the positions a read covers without an A/C/G/T base, deleted bases,
    # the base in front of an insertion
    n_rec = n_events = words = chunks = 0
    window_end = -1
    max_end = 0
    at = first_record
    while at < len(s):
        bs, tid, pos, l_name, _mq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiiBBHHHi", s, at)
        n_rec += 1
        c0 = at + 36 + l_name
        seq = s[c0 + 4 * n_cig:c0 + 4 * n_cig + (l_seq + 1) // 2]
        if not flag & 4 and tid == 0:
            span = y = 0
            for k in range(n_cig):
                cw, = struct.unpack_from("<I", s, c0 + 4 * k)
                op, ln = cw & 15, cw >> 4
                if op in (0, 7, 8):
                    codes = [(seq[q >> 1] >> (0 if q & 1 else 4)) & 15 for q in range(y, y + ln)]
                    n_events += sum(c not in (1, 2, 4, 8) for c in codes)
                    span += ln
                elif op in (2, 3):
                    n_events += ln
                    span += ln
                if op in (0, 1, 4, 7, 8):
                    y += ln
            words += words_of(span)
            if pos + span > window_end:                             # (a lower bound: a window holds the reads that END inside it)
                chunks += 1
                window_end = (pos & ~7) + MAXPOS
            max_end = max(max_end, pos + span)
        at += 4 + bs
    inflated = len(s)
    guess = min(inflated // 36 + 16, inflated // 64 + 1024)
    out = {"inflated": inflated, "n_rec": n_rec, "hint": hint, "ref_len": ref_len[0], "n_ref": n_ref, "events": n_events, "words": words,
           "chunks": chunks, "max_end": max_end, "safe_rec_cap": guess}

    def caps(h):
        rec = min(guess, inflated // h * 5 // 4 + 8192) if h >= 36 else guess
        return {"rec_cap": rec, "word_cap": inflated // 24 + 8 * rec + 64, "event_cap": max(EVENT_FLOOR, rec // 2)}
    out["caps"] = caps
    return out
