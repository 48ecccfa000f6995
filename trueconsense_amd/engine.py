"""Device context and the host-side calls of libtcmi, as thin Python objects.

    Context      one HIP stream on one MI355X (tcmi_ctx)
    ReadSet      reads resident in HBM (tcmi_readset)
    BamFile      a decoded BAM (tcmi_bam): flat read arrays + header
    consensus_walk / modal_tokens   the HOST entry points (no GPU involved)

Everything that computes goes through the C ABI (include/tcmi.h).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import dataclasses

import numpy as np

from . import _ffi
from ._ffi import check, lib, ptr


@dataclasses.dataclass(frozen=True)
class ReadRules:
    """Which tokens of a BAM reach the count matrix (csrc: struct tcmi_read_rules), one value from the command line to a context: read_filter =
    (min_mapq, require_flags, exclude_flags), min_baseq, primers = (rows, slack), mate_overlap, dedup (Context.set_*); the defaults mean
    none of them."""
    read_filter: tuple = None
    min_baseq: int = 0
    primers: tuple = None
    mate_overlap: bool = False
    dedup: bool = False


# struct tcmi_variant: one (position, non-reference allele) of the variant table
VARIANT_DTYPE = np.dtype([("pos", np.int32), ("allele", np.int32), ("count", np.int32), ("cov", np.int32)])
VARIANTS_HEADER = "REGION\tPOS\tREF\tALT\tALT_DP\tTOTAL_DP\tALT_FREQ\n"


def min_af_fraction(min_af):
    """min_af (a Fraction, or text / a number Fraction takes: "0.03", "3e-2", "3/100") -> (num, den) of the reduced fraction;
    ValueError unless 0 <= min_af <= 1 with a denominator of at most 10^6."""
    from fractions import Fraction
    try:
        f = Fraction(min_af if not isinstance(min_af, float) else repr(min_af))
    except (ValueError, ZeroDivisionError, TypeError):
        raise ValueError("%r is not a number or a fraction" % (min_af,))
    if not 0 <= f <= 1:
        raise ValueError("%s is outside 0..1" % (min_af,))
    if f.denominator > 1000000:
        raise ValueError("%s needs a denominator above 10^6 (%d)" % (min_af, f.denominator))
    return f.numerator, f.denominator


def _ref_bytes(ref):
    """str / bytes / uint8 array -> contiguous uint8 array (the reference on the count matrix's axis)"""
    if isinstance(ref, str):
        ref = ref.encode("latin-1")
    if isinstance(ref, (bytes, bytearray)):
        return np.frombuffer(bytes(ref), np.uint8)
    return np.ascontiguousarray(ref, np.uint8)


def variants_text(records, region, ref, pos_offset=0):
    """The table's rows for `records` (tcmi_variants_text, the one writer; HOST): REGION, POS = pos - pos_offset + 1, REF, ALT, ALT_DP,
    TOTAL_DP, ALT_FREQ.  ref: the reference on the records' axis.  -> str, without the header line (VARIANTS_HEADER)."""
    records = np.ascontiguousarray(records, VARIANT_DTYPE)
    ref = _ref_bytes(ref)
    n = len(records)
    cap = n * (len(str(region).encode()) + 96) + 1
    buf = C.create_string_buffer(cap)
    ln = C.c_int64(0)
    rc = lib().tcmi_variants_text(ptr(records), n, str(region).encode(), int(pos_offset), ptr(ref), len(ref), C.cast(buf, C.c_void_p), cap, C.byref(ln))
    if rc:
        raise _ffi.TcmiError(rc, "tcmi_variants_text: a record does not fit the reference, the offset or the buffer")
    return buf.raw[:ln.value].decode("latin-1")


# struct tcmi_interval_stat: the amplicon table's record of one interval of the coverage plane
INTERVAL_DTYPE = np.dtype([("sum", np.int64), ("n", np.int32), ("min", np.int32), ("min_pos", np.int32), ("median", np.int32),
                           ("below", np.int32), ("reserved", np.int32)])
AMPLICONS_HEADER = "SAMPLE\tREGION\tAMPLICON\tPOOL\tSTART\tEND\tLEN\tMEAN\tMEDIAN\tMIN\tMIN_POS\tBELOW\n"
INTERVAL_STAGE = 4096            # TCMI_INTERVAL_STAGE: columns of an interval the kernel stages in LDS


def _intervals(intervals):
    """[(start, end)] or an [n, 2] array -> (int64 starts, int64 ends), contiguous"""
    iv = np.asarray(intervals, np.int64).reshape(-1, 2)
    return np.ascontiguousarray(iv[:, 0]), np.ascontiguousarray(iv[:, 1])


def amplicons_text(records, sample, region, names, pools, starts, pos_offset=0):
    """The table's rows for `records` (tcmi_amplicons_text, the one writer; HOST): SAMPLE, REGION, AMPLICON = names[i], POOL =
    pools[i], START = starts[i] - pos_offset + 1, END, LEN, MEAN, MEDIAN, MIN, MIN_POS, BELOW.  -> str, without the header line
    (AMPLICONS_HEADER)."""
    records = np.ascontiguousarray(records, INTERVAL_DTYPE)
    n = len(records)
    starts = np.ascontiguousarray(starts, np.int64)
    if not (len(names) == len(pools) == len(starts) == n):
        raise ValueError("amplicons_text: %d records, %d names, %d pools, %d starts" % (n, len(names), len(pools), len(starts)))
    nm = (C.c_char_p * max(n, 1))(*[str(x).encode() for x in names])
    pl = (C.c_char_p * max(n, 1))(*[str(x).encode() for x in pools])
    args = (ptr(records) if n else None, n, str(sample).encode(), str(region).encode(), nm, pl, ptr(starts) if n else None, int(pos_offset))
    ln = C.c_int64(0)
    rc = lib().tcmi_amplicons_text(*args, None, 0, C.byref(ln))             # the sizing call
    if not rc:
        buf = C.create_string_buffer(ln.value + 1)
        rc = lib().tcmi_amplicons_text(*args, C.cast(buf, C.c_void_p), ln.value, C.byref(ln))
    if rc:
        raise _ffi.TcmiError(rc, "tcmi_amplicons_text: a record does not fit its start or the offset")
    return buf.raw[:ln.value].decode("utf-8", "replace")


# struct tcmi_amplicon_reads: the records of one amplicon (--amplicon-reads); rows n and n + 1 of a result: ambiguous, unassigned
AMPLICON_READS_DTYPE = np.dtype([("reads", np.int64), ("full", np.int64)])
AMPLICON_READS_HEADER = "SAMPLE\tREGION\tAMPLICON\tPOOL\tREADS\tFULL_LENGTH\n"
AMPLICON_READS_LDS = 512         # TCMI_AMPLICON_READS_LDS: amplicons whose table and counters the kernel stages in LDS


def _amps4(amps4):
    """[(fs, le, rs, fe)] or an [n, 4] array -> four contiguous int64 arrays"""
    a = np.asarray(amps4, np.int64).reshape(-1, 4)
    return tuple(np.ascontiguousarray(a[:, k]) for k in range(4))


def amplicon_reads_compile(amps4, slack=0):
    """The int32 table tcmi_readset_amplicon_reads' kernel searches (tcmi_amplicon_reads_compile; GPU-free) -> int32 [6, n]: the
    widened starts ascending, the prefix's largest end, whose it is, the second largest end, and le, rs in the order given.
    Raises TcmiError(E_ARG) with the library's words for a scheme it does not take."""
    fs, le, rs, fe = _amps4(amps4)
    n = len(fs)
    table = np.zeros((6, max(n, 1)), np.int32)
    msg = C.create_string_buffer(256)
    rc = lib().tcmi_amplicon_reads_compile(n, ptr(fs), ptr(le), ptr(rs), ptr(fe), int(slack), ptr(table), 6 * n, msg, 256)
    if rc:
        raise _ffi.TcmiError(rc, msg.value.decode("utf-8", "replace"))
    return table[:, :n]


# struct tcmi_strand_counts: the count matrix's seven planes at one column, split by the record's strand (--variant-strand)
STRAND_DTYPE = np.dtype([("fwd", np.int32, (7,)), ("rev", np.int32, (7,)), ("pos", np.int32), ("reserved", np.int32)])
VARIANTS_STRAND_HEADER = "REGION\tPOS\tREF\tALT\tALT_DP\tTOTAL_DP\tALT_FREQ\tREF_FWD\tREF_REV\tALT_FWD\tALT_REV\tTOTAL_FWD\tTOTAL_REV\tSTRAND\n"
STRAND_LDS = 256                 # TCMI_STRAND_LDS: columns whose list and counters the kernel stages in LDS
STRAND_MAX_COLS = 1 << 20        # the columns of one tcmi_readset_strand_counts call
STRAND_VERDICTS = ("PASS", "BIAS", "LOW")


def strand_verdict(alt_fwd, alt_rev, tot_fwd, tot_rev, min_strand_depth=10, strand_ratio="1/10"):
    """tcmi_strand_verdict (HOST, exact integers) -> 0 PASS, 1 BIAS, 2 LOW: LOW iff a strand's depth is below min_strand_depth, else
    BIAS iff the smaller of the two strand frequencies is below strand_ratio times the larger (a tie is PASS)."""
    num, den = min_af_fraction(strand_ratio)
    rc = lib().tcmi_strand_verdict(int(alt_fwd), int(alt_rev), int(tot_fwd), int(tot_rev), int(min_strand_depth), num, den)
    if rc < 0:
        raise _ffi.TcmiError(rc, "tcmi_strand_verdict: a negative count, min_strand_depth < 1 or a ratio outside 0..1")
    return rc


def variants_strand_text(records, strand, region, ref, pos_offset=0, min_strand_depth=10, strand_ratio="1/10"):
    """--variant-strand's rows for `records` (tcmi_variants_strand_text; HOST): variants_text's seven fields, then REF_FWD, REF_REV,
    ALT_FWD, ALT_REV, TOTAL_FWD, TOTAL_REV and STRAND.  strand: Context.strand_counts at the records' distinct positions, ascending.
    -> str, without the header line (VARIANTS_STRAND_HEADER).  TcmiError(E_ARG) when the counts do not belong to the records or do
    not add up to them."""
    records = np.ascontiguousarray(records, VARIANT_DTYPE)
    strand = np.ascontiguousarray(strand, STRAND_DTYPE)
    ref = _ref_bytes(ref)
    num, den = min_af_fraction(strand_ratio)
    args = (ptr(records) if len(records) else None, len(records), ptr(strand) if len(strand) else None, len(strand), int(min_strand_depth), num, den,
            str(region).encode(), int(pos_offset), ptr(ref) if len(ref) else None, len(ref))
    ln = C.c_int64(0)
    buf = None
    rc = lib().tcmi_variants_strand_text(*args, None, 0, C.byref(ln))       # the sizing call
    if not rc:
        buf = C.create_string_buffer(ln.value + 1)
        rc = lib().tcmi_variants_strand_text(*args, C.cast(buf, C.c_void_p), ln.value, C.byref(ln))
    if rc:
        raise _ffi.TcmiError(rc, "tcmi_variants_strand_text: the strand counts do not belong to the records or do not add up to them "
                                 "(or a record does not fit the reference, the offset or the thresholds)")
    return buf.raw[:ln.value].decode("latin-1")


# struct tcmi_evidence_counts: per plane of the count matrix at one column the tokens and the sums of their base quality, their records'
# MAPQ and their distance to the read's nearer end (--variant-evidence)
EVIDENCE_DTYPE = np.dtype([("qual", np.int64, (7,)), ("mapq", np.int64, (7,)), ("dist", np.int64, (7,)), ("n", np.int32, (7,)), ("pos", np.int32)])
VARIANTS_EVIDENCE_HEADER = ("REGION\tPOS\tREF\tALT\tALT_DP\tTOTAL_DP\tALT_FREQ\tREF_QUAL\tALT_QUAL\tREF_MAPQ\tALT_MAPQ\tREF_ENDDIST\tALT_ENDDIST\t"
                            "EVIDENCE\n")
EVIDENCE_LDS = 128               # TCMI_EVIDENCE_LDS: columns whose list and counters the kernel stages in LDS
EVIDENCE_MAX_COLS = 1 << 20      # the columns of one tcmi_readset_evidence_counts call
EVIDENCE_LOWQ, EVIDENCE_LOWMQ, EVIDENCE_END = 1, 2, 4
EVIDENCE_NAMES = ("LOWQ", "LOWMQ", "END")


def evidence_verdict(n, qual, mapq, dist, min_qual=20, min_mapq=20, min_enddist=5):
    """tcmi_evidence_verdict (HOST, exact integers) -> a bit set: 1 LOWQ iff qual < min_qual * n, 2 LOWMQ iff mapq < min_mapq * n, 4 END
    iff dist < min_enddist * n (the mean of the n tokens lies below the threshold); a threshold of 0 switches its bit off."""
    rc = lib().tcmi_evidence_verdict(int(n), int(qual), int(mapq), int(dist), int(min_qual), int(min_mapq), int(min_enddist))
    if rc < 0:
        raise _ffi.TcmiError(rc, "tcmi_evidence_verdict: a negative count or sum, or a threshold outside 0..255")
    return rc


def variants_evidence_text(records, evidence, region, ref, pos_offset=0, min_qual=20, min_mapq=20, min_enddist=5):
    """--variant-evidence's rows for `records` (tcmi_variants_evidence_text; HOST): variants_text's seven fields, then REF_QUAL, ALT_QUAL,
    REF_MAPQ, ALT_MAPQ, REF_ENDDIST, ALT_ENDDIST (means cut to one decimal) and EVIDENCE = PASS or LOWQ, LOWMQ, END joined by commas.
    evidence: Context.evidence_counts at the records' distinct positions, ascending.  -> str, without the header line
    (VARIANTS_EVIDENCE_HEADER).  TcmiError(E_ARG) when the counts do not belong to the records or do not add up to them."""
    records = np.ascontiguousarray(records, VARIANT_DTYPE)
    evidence = np.ascontiguousarray(evidence, EVIDENCE_DTYPE)
    ref = _ref_bytes(ref)
    args = (ptr(records) if len(records) else None, len(records), ptr(evidence) if len(evidence) else None, len(evidence), int(min_qual), int(min_mapq),
            int(min_enddist), str(region).encode(), int(pos_offset), ptr(ref) if len(ref) else None, len(ref))
    ln = C.c_int64(0)
    buf = None
    rc = lib().tcmi_variants_evidence_text(*args, None, 0, C.byref(ln))     # the sizing call
    if not rc:
        buf = C.create_string_buffer(ln.value + 1)
        rc = lib().tcmi_variants_evidence_text(*args, C.cast(buf, C.c_void_p), ln.value, C.byref(ln))
    if rc:
        raise _ffi.TcmiError(rc, "tcmi_variants_evidence_text: the evidence counts do not belong to the records or do not add up to them "
                                 "(or a record does not fit the reference, the offset or the thresholds)")
    return buf.raw[:ln.value].decode("latin-1")


# struct tcmi_link_counts: the kept records by token class at the two columns of a pair (--variant-links)
LINK_DTYPE = np.dtype([("j", np.int32, (7, 7)), ("a", np.int32), ("b", np.int32), ("reserved", np.int32)])
VARIANTS_LINKS_HEADER = "REGION\tPOS_A\tREF_A\tALT_A\tPOS_B\tREF_B\tALT_B\tSPAN\tBOTH\tONLY_A\tONLY_B\tNEITHER\tPHASE\n"
LINKS_LDS = 80                   # TCMI_LINKS_LDS: pairs (columns x neighbours) whose counters the kernel stages in LDS
LINKS_MAX_PAIRS = 1 << 17        # columns x neighbours of one tcmi_readset_link_counts call
LINK_PHASES = ("CIS", "TRANS", "MIXED", "NONE", "LOW")


def link_phase(both, only_a, only_b, span, min_depth=10, ratio="9/10"):
    """tcmi_link_phase (HOST, exact integers) -> 0 CIS, 1 TRANS, 2 MIXED, 3 NONE, 4 LOW: LOW iff span < min_depth; else with m the
    smaller of both + only_a and both + only_b: NONE iff m = 0, CIS iff both >= ratio * m, TRANS iff both <= (1 - ratio) * m, else
    MIXED.  ratio in (1/2, 1]."""
    num, den = min_af_fraction(ratio)
    rc = lib().tcmi_link_phase(int(both), int(only_a), int(only_b), int(span), int(min_depth), num, den)
    if rc < 0:
        raise _ffi.TcmiError(rc, "tcmi_link_phase: a negative count, min_depth < 1 or a ratio outside (1/2, 1]")
    return rc


def variants_links_text(records, links, k, region, ref, pos_offset=0, min_depth=10, ratio="9/10"):
    """--variant-links' rows for `records` (tcmi_variants_links_text; HOST): one per pair of records whose positions are at most k
    distinct positions apart, both alleles in A, T, C, G, *.  links: Context.link_counts at the records' distinct positions,
    ascending, with the same k.  -> str, without the header line (VARIANTS_LINKS_HEADER).  TcmiError(E_ARG) when the counts do not
    belong to the records or do not add up to them."""
    records = np.ascontiguousarray(records, VARIANT_DTYPE)
    links = np.ascontiguousarray(links, LINK_DTYPE)
    ref = _ref_bytes(ref)
    num, den = min_af_fraction(ratio)
    k = int(k)
    if k < 1 or len(links) % k:
        raise _ffi.TcmiError(_ffi.E_ARG, "tcmi_variants_links_text: %d link records are not a multiple of k = %d" % (len(links), k))
    args = (ptr(records) if len(records) else None, len(records), ptr(links) if len(links) else None, len(links) // k, k, int(min_depth), num, den,
            str(region).encode(), int(pos_offset), ptr(ref) if len(ref) else None, len(ref))
    ln = C.c_int64(0)
    buf = None
    rc = lib().tcmi_variants_links_text(*args, None, 0, C.byref(ln))        # the sizing call
    if not rc:
        buf = C.create_string_buffer(ln.value + 1)
        rc = lib().tcmi_variants_links_text(*args, C.cast(buf, C.c_void_p), ln.value, C.byref(ln))
    if rc:
        raise _ffi.TcmiError(rc, "tcmi_variants_links_text: the link counts do not belong to the records or do not add up to them "
                                 "(or a record does not fit the reference, the offset or the thresholds)")
    return buf.raw[:ln.value].decode("latin-1")


# struct tcmi_codon_counts: the kept records by token class at the three columns of a codon; struct tcmi_cds: one reading frame (--codon-table)
CODON_DTYPE = np.dtype([("j", np.int32, (7, 7, 7)), ("ins_inside", np.int32), ("pos", np.int32), ("reserved", np.int32)])
CDS_DTYPE = np.dtype([("start", np.int32), ("end", np.int32), ("strand", np.int32), ("phase", np.int32)])
CODONS_HEADER = ("REGION\tFEATURE\tSTRAND\tCODON\tPOS\tREF_CODON\tREF_AA\tALT_CODON\tALT_AA\tEFFECT\tSUBS\tCOUNT\tSPAN\tFREQ\tPARTIAL\tOTHER\t"
                 "INS_INSIDE\n")
CODONS_LDS = 11                  # TCMI_CODONS_LDS: codons whose first columns and counters the kernel stages in LDS
CODONS_MAX = 1 << 14             # the codons of one tcmi_readset_codon_counts call


def codon_aa(b0, b1, b2):
    """tcmi_codon_aa (HOST): three planes A..G (1..4: A, T, C, G) in coding order -> the amino acid's letter in the standard genetic
    code, "*" for a stop, "X" for anything else."""
    return chr(lib().tcmi_codon_aa(int(b0), int(b1), int(b2)))


def codon_select(records, cds):
    """tcmi_codon_select (HOST): the distinct first columns, ascending, of the codons of the frames `cds` (CDS_DTYPE) that hold at
    least one of the variant `records` with an allele in A, T, C, G, * -> int64 array."""
    records = np.ascontiguousarray(records, VARIANT_DTYPE)
    cds = np.ascontiguousarray(cds, CDS_DTYPE)
    args = (ptr(records) if len(records) else None, len(records), ptr(cds) if len(cds) else None, len(cds))
    n = C.c_int64(0)
    rc = lib().tcmi_codon_select(*args, None, 0, C.byref(n))                # the sizing call
    out = np.zeros(n.value, np.int64)
    if not rc and n.value:
        rc = lib().tcmi_codon_select(*args, ptr(out), len(out), C.byref(n))
    if rc:
        raise _ffi.TcmiError(rc, "tcmi_codon_select: a record outside the axis or the planes, or a frame with start < 0, end < start, "
                                 "a strand other than +1 / -1 or a phase outside 0..2")
    return out


def codons_text(counts, cds, names, matrix, region, ref, pos_offset=0, min_af="0.03", min_alt_depth=1, min_depth=10):
    """--codon-table's rows (tcmi_codons_text; HOST): one per (frame, counted codon inside it, reported triplet).  counts:
    Context.codon_counts, ascending; cds (CDS_DTYPE) and names: the frames and their FEATURE; matrix: the count matrix [L, 7] on the
    counts' axis.  -> str, without the header line (CODONS_HEADER).  TcmiError(E_ARG) when the counts do not add up to the matrix."""
    counts = np.ascontiguousarray(counts, CODON_DTYPE)
    cds = np.ascontiguousarray(cds, CDS_DTYPE)
    if len(names) != len(cds):
        raise ValueError("codons_text: %d frames, %d names" % (len(cds), len(names)))
    planes = np.ascontiguousarray(np.asarray(matrix, np.int32).reshape(-1, 7).T)       # [7][L]
    L = planes.shape[1]
    ref = _ref_bytes(ref)
    num, den = min_af_fraction(min_af)
    texts = [str(x).encode() for x in names]
    c_names = (C.c_char_p * max(len(texts), 1))(*texts)
    args = (ptr(counts) if len(counts) else None, len(counts), ptr(cds) if len(cds) else None, len(cds), C.cast(c_names, C.c_void_p),
            ptr(planes) if L else None, L, L, num, den, int(min_alt_depth), int(min_depth), str(region).encode(), int(pos_offset),
            ptr(ref) if len(ref) else None, len(ref))
    ln = C.c_int64(0)
    buf = None
    rc = lib().tcmi_codons_text(*args, None, 0, C.byref(ln))                # the sizing call
    if not rc:
        buf = C.create_string_buffer(ln.value + 1)
        rc = lib().tcmi_codons_text(*args, C.cast(buf, C.c_void_p), ln.value, C.byref(ln))
    if rc:
        raise _ffi.TcmiError(rc, "tcmi_codons_text: the codon counts do not add up to the count matrix "
                                 "(or a frame, the offset or the thresholds are out of range)")
    return buf.raw[:ln.value].decode("latin-1")


# struct tcmi_indel_event / tcmi_indel_totals: one insertion or deletion of the records at a column, the events per column (--indel-table)
INDEL_EVENT_DTYPE = np.dtype([("pos", np.int32), ("kind", np.int32), ("len", np.int32), ("count", np.int32), ("cov", np.int32),
                              ("reserved", np.int32), ("text_off", np.int64)])
INDEL_TOTALS_DTYPE = np.dtype([("pos", np.int32), ("ins_total", np.int32), ("del_total", np.int32), ("reserved", np.int32)])
INDELS_HEADER = "REGION\tPOS\tTYPE\tLEN\tSEQ\tCOUNT\tTOTAL_DP\tFREQ\n"
INDEL_INS, INDEL_DEL = 1, 2
INDEL_LDS = 512                  # TCMI_INDEL_LDS: columns whose list and totals the count kernel stages in LDS
INDEL_MAX_COLS = 1 << 20         # the columns of one tcmi_readset_indel_events call
INDEL_LETTERS = "=ACMGRSVTWYHKDBN"


def indel_hash(seed, nibbles, bits=34):
    """tcmi_indel_hash (HOST): the `bits` (0..34) low bits of the hash the device table keys an insertion of these SEQ nibbles (codes
    0..15) with under `seed`"""
    nib = np.ascontiguousarray(nibbles, np.uint8).reshape(-1)
    return int(lib().tcmi_indel_hash(int(seed), len(nib), ptr(nib) if len(nib) else None, int(bits)))


def indel_passes(count, cov, min_af="0.03", min_alt_depth=1, min_depth=10):
    """tcmi_indel_passes (HOST, exact integers): is an event of `count` records on a column of coverage `cov` reported — cov >=
    max(min_depth, 1), count >= min_alt_depth, count / cov >= min_af (a tie is in): the variant table's rule"""
    num, den = min_af_fraction(min_af)
    rc = lib().tcmi_indel_passes(int(count), int(cov), num, den, int(min_alt_depth), int(min_depth))
    if rc < 0:
        raise _ffi.TcmiError(rc, "tcmi_indel_passes: a negative count or coverage, min_alt_depth < 1, min_depth < 0 or min_af outside 0..1")
    return bool(rc)


def indels_text(events, text, totals, records, region, ref, pos_offset=0):
    """--indel-table's rows (tcmi_indels_text; HOST): REGION, POS, TYPE (INS / DEL), LEN, SEQ (the inserted bases / the deleted
    reference bases), COUNT, TOTAL_DP, FREQ.  events, text, totals: Context.indel_events at the distinct positions of the '*' and '+'
    rows among the variant `records`.  -> str, without the header line (INDELS_HEADER).  TcmiError(E_ARG) when the totals do not belong
    to the records, the insertions do not add up to a '+' row's depth, or an event does not fit."""
    events = np.ascontiguousarray(events, INDEL_EVENT_DTYPE)
    totals = np.ascontiguousarray(totals, INDEL_TOTALS_DTYPE)
    records = np.ascontiguousarray(records, VARIANT_DTYPE)
    text = bytes(text) if not isinstance(text, str) else text.encode("latin-1")
    ref = _ref_bytes(ref)
    args = (ptr(events) if len(events) else None, len(events), text if len(text) else None, len(text), ptr(totals) if len(totals) else None, len(totals),
            ptr(records) if len(records) else None, len(records), str(region).encode(), int(pos_offset), ptr(ref) if len(ref) else None, len(ref))
    ln = C.c_int64(0)
    buf = None
    rc = lib().tcmi_indels_text(*args, None, 0, C.byref(ln))                # the sizing call
    if not rc:
        buf = C.create_string_buffer(ln.value + 1)
        rc = lib().tcmi_indels_text(*args, C.cast(buf, C.c_void_p), ln.value, C.byref(ln))
    if rc:
        raise _ffi.TcmiError(rc, "tcmi_indels_text: the totals do not belong to the records' '*' and '+' rows, the insertions do not add up "
                                 "to a '+' row, or an event does not fit the records, the text, the reference or the order")
    return buf.raw[:ln.value].decode("latin-1")


def indel_columns(records):
    """the columns --indel-table asks about and their coverage: the distinct positions of the '*' and '+' rows of variant `records`
    -> (int64 columns ascending, int32 coverage)"""
    records = np.ascontiguousarray(records, VARIANT_DTYPE)
    mine = records[(records["allele"] == 5) | (records["allele"] == 6)]
    cols, first = np.unique(mine["pos"].astype(np.int64), return_index=True)
    return cols, np.ascontiguousarray(mine["cov"][first], np.int32)


def _grab(vp, dtype, n):
    """n items of dtype at address vp (memory the library owns) -> a fresh numpy array."""
    out = np.empty(n, dtype)
    C.memmove(out.ctypes.data, vp, out.nbytes)
    return out


def _reads_struct(reads):
    """BamFile or dict of flat arrays (tcmi_reads layout) -> (Reads struct, what keeps its arrays alive)."""
    return reads.as_struct() if isinstance(reads, BamFile) else _ffi.as_reads(reads)


def _borrowed_context(handle, device):
    """A Context over a tcmi_ctx that a pipeline or file runner owns: close() leaves it alone."""
    c = Context.__new__(Context)
    c.handle, c.device = C.c_void_p(handle), device
    c.close = lambda: None
    return c


def _token_buffer(attempt, ctx=None):
    """The token buffer of a modal-token call, grown until the tokens fit: attempt(buf, cap) -> rc makes the call; while it answers
    "token buffer too small" the buffer is tried 16 times as large, up to 1 GiB (csrc/walk_records.h does the same for the same calls).
    -> the filled buffer.  ctx: the context handle any other failure's message is read from (None: the thread's last error)."""
    cap = 1 << 16
    while True:
        buf = C.create_string_buffer(cap)
        rc = attempt(buf, cap)
        # (the vote has no context: its refusal is the thread's last error, whichever entry point made the call)
        if rc == _ffi.E_ARG and b"token buffer too small" in (lib().tcmi_last_error(None) or b"") and cap < (1 << 30):
            cap *= 16
            continue
        check(rc, ctx)
        return buf


def _token_dict(positions, buf, off, cnt):
    """What a modal-token call filled -> {position: (token or None, n_tokens)}."""
    return {int(p): (buf.raw[off[k]:off[k + 1]].decode("ascii") if cnt[k] else None, int(cnt[k])) for k, p in enumerate(positions)}


DEDUP_COUNTERS = ("templates", "duplicate_templates", "duplicate_records", "duplicate_sets")


class ReadSet:
    def __init__(self, ctx, handle, keep):
        self.ctx, self.handle, self._keep = ctx, handle, keep
        v = [C.c_int64(0) for _ in range(5)]
        check(lib().tcmi_readset_info(handle, *[C.byref(x) for x in v]))
        self.n_reads, self.n_piled, self.algorithmic_bytes, self.device_bytes, self.max_end = (x.value for x in v)
        o = C.c_int32(0)
        check(lib().tcmi_readset_origin(handle, C.byref(o)))
        self.packed_on_device = bool(o.value)       # pack_device.hip built it (else the host packer)
        a, b = C.c_int64(-1), C.c_int64(-1)
        check(lib().tcmi_readset_range_anchors(handle, C.byref(a), C.byref(b)))
        # a block range of a file: where its first record starts (a range in the middle of the file; nothing in front vouches for it)
        # and where the first record behind it starts, offsets into the file's inflated stream (-1: none) — distributed.check_range_anchors
        self.range_anchors = (a.value, b.value)
        n = C.c_int64(0)
        check(lib().tcmi_readset_filtered(handle, C.byref(n)))
        self.filtered = n.value                     # records that failed the read filter the set was built under (Context.set_read_filter)
        q = C.c_int32(0)
        check(lib().tcmi_readset_min_base_quality(handle, C.byref(q)))
        self.min_base_quality = q.value             # the base-quality floor the set was built under (Context.set_min_base_quality)
        np_, nm = C.c_int32(0), C.c_int64(0)
        check(lib().tcmi_readset_primers(handle, C.byref(np_), C.byref(nm)))
        self.primers = np_.value                    # primers of the table the set was built under (Context.set_primers; 0: none) ...
        self.primer_masked_reads = nm.value         # ... and its kept reads with a non-empty head or tail mask
        on, mv = C.c_int32(0), [C.c_int64(0) for _ in range(4)]
        check(lib().tcmi_readset_mate_overlap(handle, C.byref(on), *[C.byref(x) for x in mv]))
        # the mate-overlap rule the set was built under (Context.set_mate_overlap) and its join's counters
        self.mate_overlap = dict(zip(("on", "pairs", "clipped_reads", "clipped_columns", "ambiguous"), [on.value] + [x.value for x in mv]))
        on, dv = C.c_int32(0), [C.c_int64(0) for _ in range(4)]
        check(lib().tcmi_readset_dedup(handle, C.byref(on), *[C.byref(x) for x in dv]))
        # the duplicate rule the set was built under (Context.set_dedup) and its counters
        self.dedup = dict(zip(("on",) + DEDUP_COUNTERS, [on.value] + [x.value for x in dv]))

    def duplicates(self):
        """Built under the duplicate rule (Context.set_dedup): one bool per record of the file, True: the record belongs to a duplicate
        template.  While the decoded stream is resident on the context: E_UNSUPPORTED after its next upload."""
        out = np.zeros(max(int(self.n_reads), 1), np.uint8)
        n = C.c_int64(0)
        check(lib().tcmi_readset_duplicates(self.ctx.handle, self.handle, ptr(out), len(out), C.byref(n)), self.ctx.handle)
        return out[:n.value].astype(bool)

    def ref_extents(self, n_ref):
        """Uploaded under a contig layout of n_ref references: per reference the kept reads' max end in its own coordinates."""
        out = np.zeros(int(n_ref), np.int64)
        check(lib().tcmi_readset_ref_extents(self.handle, int(n_ref), ptr(out)))
        return out

    def dropped(self):
        """Uploaded under a contig layout: mapped reads whose reference has no slot (not tallied)."""
        n = C.c_int64(0)
        check(lib().tcmi_readset_dropped(self.handle, C.byref(n)))
        return n.value

    def free(self):
        if self.handle:
            lib().tcmi_readset_free(self.ctx.handle, self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """One device + stream.  Raises TcmiError(E_NODEVICE) when no gfx950 GPU is usable."""

    read_filter = None              # what set_read_filter / set_min_base_quality last set (a context made by the library starts without either)
    min_base_quality = 0
    primers = 0                     # rows of the table set_primers last set
    mate_overlap = False            # what set_mate_overlap last set
    dedup = False                   # what set_dedup last set
    read_rules = ReadRules()        # ... and the five as one value: what the context's next read set is built under

    def __init__(self, device=0, stream=None):
        """stream: a hipStream_t as an int (0 = the default stream) to run on, e.g. another Context's
        `.stream` or torch.cuda.current_stream().cuda_stream; None = a stream of its own."""
        h = C.c_void_p()
        if stream is None:
            check(lib().tcmi_ctx_create(int(device), C.byref(h)))
        else:
            check(lib().tcmi_ctx_create_on_stream(int(device), C.c_void_p(stream), C.byref(h)))
        self.handle = h
        self.device = device

    def close(self):
        if self.handle:
            lib().tcmi_ctx_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- plumbing
    def sync(self):
        check(lib().tcmi_ctx_sync(self.handle), self.handle)

    @property
    def stream(self):
        return lib().tcmi_ctx_stream(self.handle)

    def set_option(self, key, value):
        check(lib().tcmi_ctx_set_option(self.handle, key.encode(), int(value)), self.handle)

    def stat(self, key):
        v = C.c_int64(0)
        check(lib().tcmi_ctx_stat(self.handle, key.encode(), C.byref(v)), self.handle)
        return v.value

    def profile(self, on=True):
        check(lib().tcmi_profile_enable(self.handle, int(on)), self.handle)
        check(lib().tcmi_profile_reset(self.handle), self.handle)

    def profile_get(self, kernel):
        ms, n = C.c_double(0), C.c_int64(0)
        check(lib().tcmi_profile_get(self.handle, kernel, C.byref(ms), C.byref(n)), self.handle)
        return ms.value, n.value

    def set_read_filter(self, min_mapq=0, require_flags=0, exclude_flags=0):
        """Read filter (tcmi_ctx_set_read_filter; samtools view -q / -f / -F): from now on every read set this context builds from a
        device-decoded file ignores the records that fail it, as it ignores unmapped ones.  No arguments: no filter."""
        check(lib().tcmi_ctx_set_read_filter(self.handle, int(min_mapq), int(require_flags), int(exclude_flags)), self.handle)
        self.read_filter = (int(min_mapq), int(require_flags), int(exclude_flags))
        self.read_rules = dataclasses.replace(self.read_rules, read_filter=self.read_filter if any(self.read_filter) else None)

    def set_min_base_quality(self, q=0):
        """Base-quality floor (tcmi_ctx_set_min_base_quality; samtools mpileup -Q): from now on every read set this context builds
        from a device-decoded file skips the pileup tokens whose quality is below q — nothing for coverage, a base, X or I.  While
        q > 0 the flat-array entry points (upload, tally, the array Pipeline) refuse with E_UNSUPPORTED.  No argument: no floor."""
        check(lib().tcmi_ctx_set_min_base_quality(self.handle, int(q)), self.handle)
        self.min_base_quality = int(q)
        self.read_rules = dataclasses.replace(self.read_rules, min_baseq=int(q))

    def set_primers(self, rows=None, slack=0):
        """Amplicon primer mask (tcmi_ctx_set_primers; what `ivar trim` does to a BAM): rows = (start, end, reverse) on the count
        matrix's axis, 0-based and end-exclusive, reverse false for a '+' (left) primer.  From now on every read set this context
        builds from a device-decoded file skips the tokens a read has inside the primer at its head ('+' primers) or tail ('-'),
        within `slack` columns of the primer's outer end.  While a table is set the flat-array entry points refuse with
        E_UNSUPPORTED.  No rows: no table."""
        rows = list(rows or [])
        s_ = np.ascontiguousarray([r[0] for r in rows], np.int64)
        e_ = np.ascontiguousarray([r[1] for r in rows], np.int64)
        r_ = np.ascontiguousarray([int(r[2]) if isinstance(r[2], (bool, int, np.integer)) else int(r[2] == "-") for r in rows], np.int32)
        check(lib().tcmi_ctx_set_primers(self.handle, len(rows), ptr(s_), ptr(e_), ptr(r_), int(slack)), self.handle)
        self.primers = len(rows)
        self.read_rules = dataclasses.replace(self.read_rules, primers=(tuple(rows), int(slack)) if rows else None)

    def set_mate_overlap(self, on=False):
        """Mate overlap (tcmi_ctx_set_mate_overlap; what samtools mpileup does by default): from now on every read set this context
        builds from a whole device-decoded file counts the columns that the two mates of a pair share once — the mate that starts
        further right loses them, joined by name on the device.  While it is on the flat-array entry points, block ranges of a file
        and the split step refuse with E_UNSUPPORTED.  No argument: off."""
        check(lib().tcmi_ctx_set_mate_overlap(self.handle, int(bool(on))), self.handle)
        self.mate_overlap = bool(on)
        self.read_rules = dataclasses.replace(self.read_rules, mate_overlap=bool(on))

    def set_dedup(self, on=False):
        """Duplicate templates (tcmi_ctx_set_dedup; what samtools markdup / Picard MarkDuplicates do in a pass of their own): from now
        on every read set this context builds from a whole device-decoded file ignores the records of duplicate templates — found on
        the device by their unclipped 5' ends, the best by base-quality sum kept.  While it is on the flat-array entry points, block
        ranges of a file and the split step refuse with E_UNSUPPORTED.  No argument: off."""
        check(lib().tcmi_ctx_set_dedup(self.handle, int(bool(on))), self.handle)
        self.dedup = bool(on)
        self.read_rules = dataclasses.replace(self.read_rules, dedup=bool(on))

    def set_rules(self, rules=None):
        """A job's ReadRules onto this context, all five, nothing restored (a context that lives for the job); None leaves what it has."""
        if rules is not None:
            self.set_mate_overlap(rules.mate_overlap)
            self.set_dedup(rules.dedup)
            self.set_read_filter(*(rules.read_filter or ()))
            self.set_min_base_quality(rules.min_baseq)
            self.set_primers(*(rules.primers or ()))

    @contextlib.contextmanager
    def rules(self, rules):
        """with ctx.rules(r): under r inside the block, under none behind it however it ends (a context that serves other jobs afterwards)."""
        try:
            self.set_rules(rules)
            yield self
        finally:
            self.set_rules(ReadRules())

    def set_variants(self, ref=None, min_af="0.03", min_alt_depth=1, min_depth=10):
        """Variant table (tcmi_ctx_set_variants): from now on every step of this context (step, bamfile_step) also lists, per position
        of `ref` (the reference on the count matrix's axis), every non-reference allele with count >= min_alt_depth and
        count / cov >= min_af where cov >= max(min_depth, 1) — step_variants() has them.  The array Pipeline refuses while it is
        set.  ref None: no table."""
        if ref is None:
            check(lib().tcmi_ctx_set_variants(self.handle, None, 0, 0, 1, 1, 0), self.handle)
            return
        num, den = min_af_fraction(min_af)
        ref = _ref_bytes(ref)
        keep = ref if len(ref) else np.zeros(1, np.uint8)
        check(lib().tcmi_ctx_set_variants(self.handle, ptr(keep), len(ref), num, den, int(min_alt_depth), int(min_depth)), self.handle)

    def step_variants(self):
        """The variant records of the last ended step (tcmi_step_variants) as a fresh structured array (VARIANT_DTYPE); raises
        TcmiError(E_ARG) when that step computed none."""
        p, n = C.c_void_p(), C.c_int64(0)
        check(lib().tcmi_step_variants(self.handle, C.byref(p), C.byref(n)), self.handle)
        return _grab(p, VARIANT_DTYPE, n.value) if n.value else np.zeros(0, VARIANT_DTYPE)

    def variants_dev(self, d_counts, L, ld, d_ref, n_ref, min_af="0.03", min_alt_depth=1, min_depth=10, d_records=0, cap=0):
        """Device-resident table (tcmi_variants_dev): int32 [7][ld] planes and the reference at device addresses -> the number of
        records the rule yields; the first `cap` of them are written at `d_records` (device or pinned host address; 0 with cap 0:
        count only).  Raises TcmiError(E_ARG) when there are more than cap (its .n_found has the number)."""
        num, den = min_af_fraction(min_af)
        n = C.c_int64(0)
        rc = lib().tcmi_variants_dev(self.handle, C.c_void_p(int(d_counts)), int(L), int(ld), C.c_void_p(int(d_ref)) if d_ref else None, int(n_ref),
                                     num, den, int(min_alt_depth), int(min_depth), C.c_void_p(int(d_records)) if d_records else None, int(cap),
                                     C.byref(n))
        try:
            check(rc, self.handle)
        except _ffi.TcmiError as e:
            e.n_found = n.value
            raise
        return n.value

    def variants(self, counts, ref, min_af="0.03", min_alt_depth=1, min_depth=10):
        """counts [L,7] and the reference on their axis -> the table's records, a structured array (VARIANT_DTYPE) ordered by
        position, then allele A, T, C, G, X, I (tcmi_variants)."""
        counts = np.ascontiguousarray(counts, np.int32)
        ref = _ref_bytes(ref)
        num, den = min_af_fraction(min_af)
        L = len(counts)
        cap = 5 * min(L, len(ref))
        out = np.zeros(max(cap, 1), VARIANT_DTYPE)
        n = C.c_int64(0)
        check(lib().tcmi_variants(self.handle, ptr(counts), L, ptr(ref) if len(ref) else None, len(ref), num, den, int(min_alt_depth),
                                  int(min_depth), ptr(out), cap, C.byref(n)), self.handle)
        return out[:n.value].copy()

    def set_intervals(self, intervals=None, min_depth=0):
        """Amplicon table (tcmi_ctx_set_intervals): from now on every step of this context (step, bamfile_step) also computes, per
        interval [start, end) of the count matrix's axis, the coverage plane's sum, minimum with its first position, lower median and
        the positions below min_depth — step_intervals() has them.  The array Pipeline refuses while it is set.  None or empty: no
        table."""
        if intervals is None or len(intervals) == 0:
            check(lib().tcmi_ctx_set_intervals(self.handle, 0, None, None, 0), self.handle)
            return
        st, en = _intervals(intervals)
        check(lib().tcmi_ctx_set_intervals(self.handle, len(st), ptr(st), ptr(en), int(min_depth)), self.handle)

    def step_intervals(self):
        """The interval records of the last ended step (tcmi_step_intervals) as a fresh structured array (INTERVAL_DTYPE); raises
        TcmiError(E_ARG) when that step computed none."""
        p, n = C.c_void_p(), C.c_int64(0)
        check(lib().tcmi_step_intervals(self.handle, C.byref(p), C.byref(n)), self.handle)
        return _grab(p, INTERVAL_DTYPE, n.value)

    def interval_stats_dev(self, d_counts, L, ld, n, d_start, d_end, min_depth, d_records):
        """Device-resident records (tcmi_interval_stats_dev): int32 [7][ld] planes, int64 starts and ends at device addresses -> n
        records at `d_records` (device or pinned host address)."""
        check(lib().tcmi_interval_stats_dev(self.handle, C.c_void_p(int(d_counts)), int(L), int(ld), int(n), C.c_void_p(int(d_start)) if d_start else None,
                                            C.c_void_p(int(d_end)) if d_end else None, int(min_depth), C.c_void_p(int(d_records)) if d_records else None),
              self.handle)

    def interval_stats(self, counts, intervals, min_depth=0):
        """counts [L,7] and [(start, end)] on their axis -> one record per interval, a structured array (INTERVAL_DTYPE), in the order
        given (tcmi_interval_stats)."""
        counts = np.ascontiguousarray(counts, np.int32)
        st, en = _intervals(intervals)
        out = np.zeros(len(st), INTERVAL_DTYPE)
        if len(st) == 0:
            return out
        check(lib().tcmi_interval_stats(self.handle, ptr(counts), len(counts), len(st), ptr(st), ptr(en), int(min_depth), ptr(out)), self.handle)
        return out

    def amplicon_reads(self, readset, amps4, slack=0):
        """Reads per amplicon (tcmi_readset_amplicon_reads): amps4 = [(fs, le, rs, fe)] on the count matrix's axis, slack in 0..1000
        -> a structured array (AMPLICON_READS_DTYPE) of n + 2 rows: per amplicon the records contained in it alone and those of them
        that run from its left primer zone into its right one, then the ambiguous records (contained in two or more), then the
        unassigned ones; the `reads` add up to the read set's kept records.  The read set must have been decoded on the device and
        its stream must still be resident on this context (no other upload since), else TcmiError(E_UNSUPPORTED)."""
        fs, le, rs, fe = _amps4(amps4)
        out = np.zeros(len(fs) + 2, AMPLICON_READS_DTYPE)
        check(lib().tcmi_readset_amplicon_reads(self.handle, readset.handle, len(fs), ptr(fs), ptr(le), ptr(rs), ptr(fe), int(slack), ptr(out)),
              self.handle)
        return out

    def strand_counts(self, readset, cols):
        """The count matrix's planes at `cols`, split by strand (tcmi_readset_strand_counts): cols strictly ascending on the count
        matrix's axis, 1..2^20 of them -> a structured array (STRAND_DTYPE): fwd and rev as [n, 7] in plane order (the records without
        and with FLAG 0x10), pos; fwd + rev is the matrix a step tallies from the read set.  The read set must have been decoded on
        the device and its stream must still be resident on this context (no other upload since), else TcmiError(E_UNSUPPORTED)."""
        cols = np.ascontiguousarray(cols, np.int64).reshape(-1)
        out = np.zeros(len(cols), STRAND_DTYPE)
        check(lib().tcmi_readset_strand_counts(self.handle, readset.handle, len(cols), ptr(cols) if len(cols) else None, ptr(out) if len(cols) else None),
              self.handle)
        return out

    def strand_counts_of(self, readset, records=None, cols=None):
        """strand_counts at the distinct positions of variant `records` (or at `cols`, ascending), in pieces of 2^20 columns -> a
        structured array (STRAND_DTYPE), empty without columns"""
        if cols is None:
            cols = np.unique(np.ascontiguousarray(records, VARIANT_DTYPE)["pos"].astype(np.int64))
        cols = np.ascontiguousarray(cols, np.int64).reshape(-1)
        parts = [self.strand_counts(readset, cols[k:k + STRAND_MAX_COLS]) for k in range(0, len(cols), STRAND_MAX_COLS)]
        return np.concatenate(parts) if parts else np.zeros(0, STRAND_DTYPE)

    def evidence_counts(self, readset, cols):
        """Per plane of the count matrix at `cols` the tokens and the sums of their base quality, their records' MAPQ and their
        distance to the nearer end of the read's aligned part, capped at 255 (tcmi_readset_evidence_counts): cols strictly ascending
        on the count matrix's axis, 1..2^20 of them -> a structured array (EVIDENCE_DTYPE): qual, mapq, dist (int64) and n as [n, 7]
        in plane order, pos; n is the matrix a step tallies from the read set.  The read set must have been decoded on the device and
        its stream must still be resident on this context (no other upload since), else TcmiError(E_UNSUPPORTED)."""
        cols = np.ascontiguousarray(cols, np.int64).reshape(-1)
        out = np.zeros(len(cols), EVIDENCE_DTYPE)
        check(lib().tcmi_readset_evidence_counts(self.handle, readset.handle, len(cols), ptr(cols) if len(cols) else None, ptr(out) if len(cols) else None),
              self.handle)
        return out

    def evidence_counts_of(self, readset, records=None, cols=None):
        """evidence_counts at the distinct positions of variant `records` (or at `cols`, ascending), in pieces of 2^20 columns -> a
        structured array (EVIDENCE_DTYPE), empty without columns"""
        if cols is None:
            cols = np.unique(np.ascontiguousarray(records, VARIANT_DTYPE)["pos"].astype(np.int64))
        cols = np.ascontiguousarray(cols, np.int64).reshape(-1)
        parts = [self.evidence_counts(readset, cols[k:k + EVIDENCE_MAX_COLS]) for k in range(0, len(cols), EVIDENCE_MAX_COLS)]
        return np.concatenate(parts) if parts else np.zeros(0, EVIDENCE_DTYPE)

    def link_counts(self, readset, cols, k):
        """Joint token classes of the kept records at pairs of nearby columns (tcmi_readset_link_counts): cols strictly ascending on
        the count matrix's axis, k neighbours in 1..7, len(cols) * k in 1..2^17 -> a structured array (LINK_DTYPE) of len(cols) * k
        records: record i * k + d - 1 is the pair (cols[i], cols[i + d]) with j[x][y] the records of class x at a and y at b (0 no
        token, 1..4 A T C G, 5 a deleted column, 6 coverage only); b = -1 where cols has no such column.  The read set must have
        been decoded on the device and its stream must still be resident on this context, else TcmiError(E_UNSUPPORTED)."""
        cols = np.ascontiguousarray(cols, np.int64).reshape(-1)
        k = int(k)
        out = np.zeros(len(cols) * max(k, 0), LINK_DTYPE)
        check(lib().tcmi_readset_link_counts(self.handle, readset.handle, len(cols), ptr(cols) if len(cols) else None, k, ptr(out) if len(out) else None),
              self.handle)
        return out

    def link_counts_of(self, readset, records, k):
        """link_counts at the distinct positions of variant `records` -> a structured array (LINK_DTYPE), empty without records"""
        cols = np.unique(np.ascontiguousarray(records, VARIANT_DTYPE)["pos"].astype(np.int64))
        return self.link_counts(readset, cols, k) if len(cols) else np.zeros(0, LINK_DTYPE)

    def codon_counts(self, readset, c0):
        """Joint token classes of the kept records at the three columns of codons (tcmi_readset_codon_counts): c0 the codons' first
        columns, strictly ascending on the count matrix's axis (they may differ by 1 or 2: overlapping frames), 1..2^14 of them -> a
        structured array (CODON_DTYPE): j[t0][t1][t2] the records with those classes at c0, c0 + 1, c0 + 2 (0 no token, 1..4 A T C G,
        5 a deleted column, 6 coverage only), ins_inside those of them with inserted bases behind the first or second column, pos.
        The read set must have been decoded on the device and its stream must still be resident on this context, else
        TcmiError(E_UNSUPPORTED)."""
        c0 = np.ascontiguousarray(c0, np.int64).reshape(-1)
        out = np.zeros(len(c0), CODON_DTYPE)
        check(lib().tcmi_readset_codon_counts(self.handle, readset.handle, len(c0), ptr(c0) if len(c0) else None, ptr(out) if len(c0) else None),
              self.handle)
        return out

    def codon_counts_of(self, readset, records, cds):
        """codon_counts at the codons of the frames `cds` (CDS_DTYPE) that hold one of the variant `records` (codon_select), in pieces of
        2^14 codons -> a structured array (CODON_DTYPE), empty without such a codon"""
        c0 = codon_select(records, cds)
        parts = [self.codon_counts(readset, c0[k:k + CODONS_MAX]) for k in range(0, len(c0), CODONS_MAX)]
        return np.concatenate(parts) if parts else np.zeros(0, CODON_DTYPE)

    def _indel_events(self, readset, cols, cov, num, den, min_alt_depth, min_depth):
        """one tcmi_readset_indel_events call of at most 2^20 columns, with room for what a file usually has; a call that says it
        found more is made again with room for exactly that"""
        totals = np.zeros(len(cols), INDEL_TOTALS_DTYPE)
        n, tl = C.c_int64(0), C.c_int64(0)
        head = (self.handle, readset.handle, len(cols), ptr(cols), ptr(cov), num, den, int(min_alt_depth), int(min_depth))
        cap, tcap = 4096, 65536
        for _ in range(2):
            events = np.zeros(cap, INDEL_EVENT_DTYPE)
            text = C.create_string_buffer(tcap)
            rc = lib().tcmi_readset_indel_events(*head, ptr(events), cap, C.byref(n), C.cast(text, C.c_void_p), tcap, C.byref(tl), ptr(totals))
            if rc != _ffi.E_ARG or (n.value <= cap and tl.value <= tcap):
                break
            cap, tcap = max(n.value, 1), max(tl.value, 1)
        check(rc, self.handle)
        return events[:n.value].copy(), text.raw[:tl.value], totals

    def indel_events(self, readset, cols, cov, min_af="0.03", min_alt_depth=1, min_depth=10):
        """The insertions and deletions of the kept records at `cols` (tcmi_readset_indel_events): cols strictly ascending on the
        count matrix's axis, cov the matrix's coverage there -> (events, text, totals): events a structured array
        (INDEL_EVENT_DTYPE) in the order (pos, kind, len, bases) — kind 1 an insertion behind the base at pos, its bases
        text[text_off : text_off + len], kind 2 a deletion whose first base is pos — of those that pass the variant table's rule; text
        bytes; totals (INDEL_TOTALS_DTYPE) the events of each kind per column, reported or not: ins_total is the matrix's I plane.
        Large queries are taken in pieces of 2^20 columns.  The read set must have been decoded on the device and its stream must
        still be resident on this context (no other upload since), else TcmiError(E_UNSUPPORTED)."""
        cols = np.ascontiguousarray(cols, np.int64).reshape(-1)
        cov = np.ascontiguousarray(cov, np.int32).reshape(-1)
        if len(cols) != len(cov):
            raise ValueError("indel_events: %d columns, %d coverages" % (len(cols), len(cov)))
        num, den = min_af_fraction(min_af)
        ev, tx, tot, off = [], [], [], 0
        for k in range(0, len(cols), INDEL_MAX_COLS):
            e, t, s = self._indel_events(readset, cols[k:k + INDEL_MAX_COLS], cov[k:k + INDEL_MAX_COLS], num, den, min_alt_depth, min_depth)
            e = e.copy()
            e["text_off"][e["kind"] == INDEL_INS] += off
            off += len(t)
            ev.append(e), tx.append(t), tot.append(s)
        if not ev:
            return np.zeros(0, INDEL_EVENT_DTYPE), b"", np.zeros(0, INDEL_TOTALS_DTYPE)
        return np.concatenate(ev), b"".join(tx), np.concatenate(tot)

    def indel_events_of(self, readset, records, **rule):
        """indel_events at the distinct positions of the '*' and '+' rows of variant `records`, with their coverage"""
        cols, cov = indel_columns(records)
        return self.indel_events(readset, cols, cov, **rule)

    def set_layout(self, shift=None, slot_len=None):
        """Contig layout (tcmi_ctx_set_layout): reference t's reads pile up at pos + shift[t] (< 0: dropped), in a slot of
        slot_len[t] positions.  No arguments: back to reference 0 only."""
        shift = np.ascontiguousarray([] if shift is None else shift, np.int64)
        slot_len = np.ascontiguousarray([] if slot_len is None else slot_len, np.int64)
        if len(shift) != len(slot_len):
            raise ValueError("shift and slot_len differ in length")
        check(lib().tcmi_ctx_set_layout(self.handle, len(shift), ptr(shift) if len(shift) else None,
                                        ptr(slot_len) if len(slot_len) else None), self.handle)

    # ---- stage A
    def upload(self, reads):
        """reads: dict of flat arrays (tcmi_reads layout) or BamFile -> ReadSet in HBM."""
        r, keep = _reads_struct(reads)
        h = C.c_void_p()
        check(lib().tcmi_readset_upload(self.handle, C.byref(r), C.byref(h)), self.handle)
        return ReadSet(self, h, keep)

    def upload_batch(self, reads_list, stride):
        """Several BAMs in one read set: BAM b's positions are shifted by b * stride (multiple of 256)."""
        structs, keep = [], []
        for r in reads_list:
            st, k = _reads_struct(r)
            structs.append(st)
            keep.append(k)
        arr = (C.POINTER(_ffi.Reads) * len(structs))(*[C.pointer(s) for s in structs])
        h = C.c_void_p()
        check(lib().tcmi_readset_upload_batch(self.handle, arr, len(structs), int(stride), C.byref(h)), self.handle)
        return ReadSet(self, h, (keep, structs))

    def upload_bamfile(self, dbam, blocks=None):
        """DeviceBam -> ReadSet: BGZF inflate, record index and packing all on the device.  blocks = (first, count): only the
        records that start in that range of the file's BGZF blocks (ranks that share one file take a range each)."""
        h, n = C.c_void_p(), C.c_int64(0)
        first, count = (0, -1) if blocks is None else blocks
        check(lib().tcmi_readset_from_bamfile_blocks(self.handle, dbam.handle, int(first), int(count), C.byref(h), C.byref(n)), self.handle)
        rs = ReadSet(self, h, None)
        return rs

    def bamfile_step(self, dbam, ref_len, mincov, include_ambig, want_counts=True):
        """DeviceBam -> (ReadSet, plain, alt, flags, counts or None) with ONE wait of the host (tcmi_bamfile_step): decode, pack,
        tally and call queued back to back; a file the one-pass packer does not take goes through upload_bamfile + step."""
        h, L = C.c_void_p(), C.c_int64(0)
        p, a, f, c = (C.c_void_p() for _ in range(4))
        ld = C.c_int64(0)
        check(lib().tcmi_bamfile_step(self.handle, dbam.handle, int(ref_len), int(mincov), int(bool(include_ambig)), C.byref(h), C.byref(L),
                                      C.byref(p), C.byref(a), C.byref(f), C.byref(c) if want_counts else None, C.byref(ld)), self.handle)
        n = L.value
        plain, alt, flags = _grab(p, np.uint8, n), _grab(a, np.uint8, n), _grab(f, np.uint8, n)
        counts = None
        if want_counts:
            counts = np.ascontiguousarray(_grab(c, np.int32, 7 * ld.value).reshape(7, ld.value)[:, :n].T)
        return ReadSet(self, h, None), plain, alt, flags, counts

    def readset_modal_tokens(self, readset, positions, min_base_quality=13, flag_filter=0x4 | 0x100 | 0x200 | 0x400,
                             ignore_orphans=True, max_depth=8000, ignore_overlaps=True):
        """modal_tokens() for a read set the device decoded: the reads of each candidate column are examined by a HIP kernel in
        the still-resident inflated stream.  Raises TcmiError(E_UNSUPPORTED) when that stream is gone or a token does not fit."""
        positions = np.ascontiguousarray(sorted(int(p) for p in positions), np.int64)
        n = len(positions)
        if n == 0:
            return {}
        off, cnt, st = np.zeros(n + 1, np.int64), np.zeros(n, np.int64), C.c_int32(0)
        buf = _token_buffer(lambda buf, cap: lib().tcmi_readset_modal_tokens(
            self.handle, readset.handle, n, ptr(positions), int(min_base_quality), int(flag_filter), int(bool(ignore_orphans)), int(max_depth),
            int(bool(ignore_overlaps)), C.cast(buf, C.c_void_p), cap, ptr(off), ptr(cnt), C.byref(st)), self.handle)
        if st.value & 2:
            raise _ffi.TcmiError(_ffi.E_UNSUPPORTED, "overlapping mates with a deletion on an insert-candidate column")
        return _token_dict(positions, buf, off, cnt)

    def tally(self, reads, L=None, ref_len=0):
        """reads -> int32 [L,7] (coverage,A,T,C,G,X,I); L defaults to max(ref_len, read extent)."""
        r, keep = _reads_struct(reads)
        if L is None:
            L = reads_extent(reads, ref_len)
        counts = np.zeros((int(L), 7), np.int32)
        check(lib().tcmi_tally(self.handle, C.byref(r), int(L), ptr(counts)), self.handle)
        del keep
        return counts

    def tally_dev(self, readset, L, ld, d_counts, zero=True):
        """Device-resident tally into int32 [7][ld] planes at device address `d_counts` (e.g. a torch
        tensor's data_ptr()), on this context's stream."""
        check(lib().tcmi_tally_dev(self.handle, readset.handle, int(L), int(ld), C.c_void_p(int(d_counts)), int(bool(zero))),
              self.handle)

    def call_dev(self, d_counts, L, ld, mincov, include_ambig, d_plain, d_alt, d_flags):
        """Device-resident call: counts planes -> three uint8[ld] record planes (device addresses)."""
        check(lib().tcmi_call_dev(self.handle, C.c_void_p(int(d_counts)), int(L), int(ld), int(mincov), int(bool(include_ambig)),
                                  C.c_void_p(int(d_plain)), C.c_void_p(int(d_alt)), C.c_void_p(int(d_flags)), None, None),
              self.handle)

    # ---- stage B, position-local
    def call(self, counts, mincov, include_ambig, want_events=False):
        """counts [L,7] -> (plain, alt, flags) uint8 [L] (+ ascending 0-based event indices)."""
        counts = np.ascontiguousarray(counts, np.int32)
        L = len(counts)
        plain, alt, flags = (np.empty(L, np.uint8) for _ in range(3))
        ev = np.empty(L, np.int32) if want_events else None
        n_ev = C.c_int64(0)
        check(lib().tcmi_call(self.handle, ptr(counts), L, int(mincov), int(bool(include_ambig)), ptr(plain),
                              ptr(alt), ptr(flags), ptr(ev), C.byref(n_ev)), self.handle)
        if want_events:
            return plain, alt, flags, ev[:n_ev.value].copy()
        return plain, alt, flags

    # ---- whole resident step: zero + tally + call + records to pinned host memory
    def step(self, readset, L, mincov, include_ambig, want_counts=True):
        self.step_begin(readset, L, mincov, include_ambig, want_counts)
        return self.step_end()

    def step_begin(self, readset, L, mincov, include_ambig, want_counts=True):
        """Enqueue the step on this context's stream and return at once."""
        check(lib().tcmi_step_begin(self.handle, readset.handle, int(L), int(mincov), int(bool(include_ambig)),
                                    int(bool(want_counts))), self.handle)
        self._step = (int(L), bool(want_counts))

    def step_end(self):
        """Wait for the stream; -> (plain, alt, flags, counts or None) as fresh numpy arrays."""
        L, want_counts = self._step
        p, a, f, c = (C.c_void_p() for _ in range(4))
        ld = C.c_int64(0)
        check(lib().tcmi_step_end(self.handle, C.byref(p), C.byref(a), C.byref(f), C.byref(c), C.byref(ld)),
              self.handle)
        plain, alt, flags = _grab(p, np.uint8, L), _grab(a, np.uint8, L), _grab(f, np.uint8, L)
        counts = None
        if want_counts:
            planes = _grab(c, np.int32, 7 * ld.value).reshape(7, ld.value)
            counts = np.ascontiguousarray(planes[:, :L].T)
        return plain, alt, flags, counts


# --------------------------------------------------------------------------- host-only entry points
def reads_extent(reads, ref_len=0):
    r, keep = _reads_struct(reads)
    out = C.c_int64(0)
    check(lib().tcmi_reads_extent(C.byref(r), int(ref_len), C.byref(out)))
    del keep
    return out.value


class WalkKeyError(KeyError):
    """The reference raises KeyError here (Sequences.py:47): a deletion walk ran past the last position."""


def _check_walk(rc, err, key_error=WalkKeyError):
    """A walk's return code -> what the reference raises there (key_error(err), ZeroDivisionError), else check()."""
    if rc == _ffi.E_KEYERROR:
        raise key_error(err)
    if rc == _ffi.E_ZERODIV:
        raise ZeroDivisionError("division by zero")
    check(rc)


def consensus_walk(plain, alt, flags, orf_start, orf_end, orf_is_plus, ins_pos, ins_shift, ins_seqs,
                   include_ins):
    """Sequential part of BuildConsensus (Sequences.py:179-322 + ORFs.py) over call records.
    -> (consensus str, new_start int64[n_orf], new_end int64[n_orf])."""
    plain, alt, flags = (np.ascontiguousarray(x, np.uint8) for x in (plain, alt, flags))
    L = len(plain)
    os_, oe = np.ascontiguousarray(orf_start, np.int64), np.ascontiguousarray(orf_end, np.int64)
    op = np.ascontiguousarray(orf_is_plus, np.uint8)
    ip = np.ascontiguousarray(ins_pos, np.int64)
    ish = np.ascontiguousarray(ins_shift, np.int32)
    blob = "".join(ins_seqs).encode("ascii")
    off = np.zeros(len(ins_seqs) + 1, np.int64)
    if len(ins_seqs):
        off[1:] = np.cumsum([len(s) for s in ins_seqs])
    cap = L + len(blob) + 1
    out = C.create_string_buffer(cap)
    n_out, err = C.c_int64(0), C.c_int64(0)
    ns, ne = np.zeros(len(os_), np.int64), np.zeros(len(os_), np.int64)
    rc = lib().tcmi_consensus_walk(ptr(plain), ptr(alt), ptr(flags), L, len(os_), ptr(os_), ptr(oe), ptr(op),
                                   len(ip), ptr(ip), ptr(ish), blob, ptr(off), int(bool(include_ins)),
                                   C.cast(out, C.c_void_p), cap, C.byref(n_out), ptr(ns), ptr(ne), C.byref(err))
    _check_walk(rc, err.value)
    return out.raw[:n_out.value].decode("ascii"), ns, ne


class Pipeline:
    """Native batch runner (tcmi_pipeline): many resident BAMs -> consensus sequences, GPU steps
    queued ahead on one stream, walks on `walkers` host threads."""

    def __init__(self, device=0, slots=4, walkers=4):
        h = C.c_void_p()
        check(lib().tcmi_pipeline_create(int(device), int(slots), int(walkers), C.byref(h)))
        self.handle, self.slots = h, int(slots)
        self.ctx = _borrowed_context(lib().tcmi_pipeline_ctx(h, 0), device)        # slot 0's context, owned by the pipeline

    def slot_context(self, k):
        return _borrowed_context(lib().tcmi_pipeline_ctx(self.handle, k), self.ctx.device)

    def set_orfs(self, start, end, is_plus):
        s_, e_ = np.ascontiguousarray(start, np.int64), np.ascontiguousarray(end, np.int64)
        p_ = np.ascontiguousarray(is_plus, np.uint8)
        check(lib().tcmi_pipeline_set_orfs(self.handle, len(s_), ptr(s_), ptr(e_), ptr(p_)))

    def run(self, readsets, L, mincov, include_ambig, host_reads=None, extra=4096, batch=1, pos_stride=0, out=None):
        """-> (list of consensus bytes, int32 status array).  Raises on the first failed item.
        batch > 1: every read set holds `batch` BAMs (Context.upload_batch at `pos_stride`); the outputs
        (and host_reads) are then per BAM, item-major.
        out: a caller-owned uint8 array of >= n * (L + 1 + extra) bytes — the walkers write every consensus into it
        at multiples of that stride and the call returns (out, lengths, status) without building Python objects
        (a long queue otherwise spends its time in page faults of the fresh buffer and in 30 KB copies)."""
        n_items = len(readsets)
        rs = (C.c_void_p * n_items)(*[r.handle for r in readsets])
        n = n_items * int(batch)
        keep, hr = [], None
        if host_reads is not None:
            by_id = {}                                   # the same reads object may back many items: convert it once
            ptrs = []
            for r in host_reads:
                if r is None:
                    ptrs.append(None)
                    continue
                if id(r) not in by_id:
                    st, k = _reads_struct(r)
                    by_id[id(r)] = (st, k, C.pointer(st))
                ptrs.append(by_id[id(r)][2])
            hr = (C.POINTER(_ffi.Reads) * n)(*ptrs)
            keep.append(by_id)
        stride = int(L) + 1 + int(extra)
        own = out is None
        if own:
            out = np.empty(n * stride, np.uint8)
        elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < n * stride:
            raise ValueError("out must be a contiguous uint8 array of at least %d bytes" % (n * stride))
        lens = np.zeros(n, np.int64)
        status = np.zeros(n, np.int32)
        rc = lib().tcmi_pipeline_run_batched(self.handle, n_items, rs, int(batch), int(pos_stride), hr, int(L), int(mincov),
                                             int(bool(include_ambig)), ptr(out), stride, ptr(lens), ptr(status))
        self.last_status = status
        check(rc)
        if not own:
            return out, lens, status
        return [out[i * stride:i * stride + int(lens[i])].tobytes() for i in range(n)], status

    def close(self):
        if self.handle:
            lib().tcmi_pipeline_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Walker:
    """consensus_walk with the GFF rows fixed and no inserts: the arrays are converted once, so a
    call is one ctypes crossing (the GIL is released meanwhile: walks of different BAMs can run
    on several host threads)."""

    def __init__(self, orf_start, orf_end, orf_is_plus, include_ins=True):
        self.os = np.ascontiguousarray(orf_start, np.int64)
        self.oe = np.ascontiguousarray(orf_end, np.int64)
        self.op = np.ascontiguousarray(orf_is_plus, np.uint8)
        self.off = np.zeros(1, np.int64)
        self.include_ins = int(bool(include_ins))
        self._fn = lib().tcmi_consensus_walk

    def __call__(self, plain, alt, flags):
        L = len(plain)
        out = C.create_string_buffer(L + 1)
        n_out, err = C.c_int64(0), C.c_int64(0)
        n = len(self.os)
        ns, ne = np.empty(n, np.int64), np.empty(n, np.int64)
        rc = self._fn(ptr(plain), ptr(alt), ptr(flags), L, n, ptr(self.os), ptr(self.oe), ptr(self.op),
                      0, None, None, b"", ptr(self.off), self.include_ins, C.cast(out, C.c_void_p), L + 1,
                      C.byref(n_out), ptr(ns), ptr(ne), C.byref(err))
        _check_walk(rc, err.value)
        return out.raw[:n_out.value], ns, ne


# pysam's defaults for AlignmentFile.pileup() (Events.py:66 passes none): SURVEY §8-Q8
DEFAULT_MIN_BASE_QUALITY = 13
DEFAULT_FLAG_FILTER = 0x4 | 0x100 | 0x200 | 0x400
DEFAULT_MAX_DEPTH = 8000


def modal_tokens(reads, positions, min_base_quality=DEFAULT_MIN_BASE_QUALITY, flag_filter=DEFAULT_FLAG_FILTER,
                 ignore_orphans=True, max_depth=DEFAULT_MAX_DEPTH, ignore_overlaps=True, layout=None):
    """For each 1-based position: (modal upper-cased token or None, n_tokens) under pysam's default pileup arguments
    (Events.py:66).  Overlapping mates with a deletion / ref-skip on the column are resolved too: the sweep probes the other mate
    on the next query base's reference position itself, so status bit 1 never comes back from it (the check below is a guard).
    layout = (shift, slot_len): positions on a contig layout's axis (tcmi_modal_tokens_layout)."""
    positions = np.ascontiguousarray(sorted(int(p) for p in positions), np.int64)
    n = len(positions)
    if n == 0:
        return {}
    r, keep = _reads_struct(reads)
    off, cnt, deep = np.zeros(n + 1, np.int64), np.zeros(n, np.int64), C.c_int32(0)
    if layout is not None:
        sh, sl = (np.ascontiguousarray(x, np.int64) for x in layout)

    def attempt(buf, cap):
        tail = (int(min_base_quality), int(flag_filter), int(bool(ignore_orphans)), int(max_depth), int(bool(ignore_overlaps)),
                C.cast(buf, C.c_void_p), cap, ptr(off), ptr(cnt), C.byref(deep))
        if layout is None:
            return lib().tcmi_modal_tokens(C.byref(r), n, ptr(positions), *tail)
        return lib().tcmi_modal_tokens_layout(C.byref(r), len(sh), ptr(sh), ptr(sl), n, ptr(positions), *tail)
    buf = _token_buffer(attempt)
    del keep
    if deep.value & 2:
        raise _ffi.TcmiError(_ffi.E_UNSUPPORTED, "overlapping mates with a deletion on an insert-candidate column: pysam's overlap "
                                                  "quality tweak there is not modelled")
    return _token_dict(positions, buf, off, cnt)


def _header_refs(fn, h, n_ref):
    """(names, lengths) of every reference of a BAM header (`references` / `lengths` keep pysam's first-reference view)."""
    names, lens = [], []
    for i in range(n_ref):
        name, ln = C.c_char_p(), C.c_int64(0)
        check(fn(h, i, C.byref(name), C.byref(ln)))
        names.append((name.value or b"").decode())
        lens.append(ln.value)
    return tuple(names), tuple(lens)


class BamFile:
    """A BAM decoded by libtcmi (tcmi_bam_load): pysam.AlignmentFile's role for this path.  read_filter = (min_mapq,
    require_flags, exclude_flags): the records that fail it are removed after the load (tcmi_bam_filter) — n_reads and the arrays
    are the passing records', n_records stays the file's count, n_removed the difference."""

    def __init__(self, path, threads=0, read_filter=None):
        h = C.c_void_p()
        check(lib().tcmi_bam_load(str(path).encode(), int(threads), C.byref(h)))
        self.handle = h
        n0, gone = C.c_int64(0), C.c_int64(0)
        check(lib().tcmi_bam_info(h, C.byref(n0), None, None, None, None, None, None))
        if read_filter is not None:
            check(lib().tcmi_bam_filter(h, *(int(x) for x in read_filter), C.byref(gone)))
        self.n_records, self.n_removed = n0.value, gone.value
        self.filename = str(path)
        n_ref, name, ln = C.c_int32(0), C.c_char_p(), C.c_int64(0)
        check(lib().tcmi_bam_header(h, C.byref(n_ref), C.byref(name), C.byref(ln)))
        self.nreferences = n_ref.value
        self.references = ((name.value or b"").decode(),) if n_ref.value else ()
        self.lengths = (ln.value,) if n_ref.value else ()
        self.all_references, self.all_lengths = _header_refs(lib().tcmi_bam_ref, h, n_ref.value)
        v = [C.c_int64(0), C.c_int32(0)] + [C.c_int64(0) for _ in range(5)]
        check(lib().tcmi_bam_info(h, *[C.byref(x) for x in v]))
        (self.n_reads, self.sorted, self.file_bytes, self.inflated_bytes, self.n_blocks, self.n_cigar,
         self.n_qual) = (x.value for x in v)
        self.text = (lib().tcmi_bam_text(h) or b"").decode("utf-8", "replace")

    def as_struct(self):
        r = _ffi.Reads()
        check(lib().tcmi_bam_reads(self.handle, C.byref(r)))
        return r, self

    def arrays(self):
        """numpy views (owned by this object) in the tcmi_reads layout."""
        r, _ = self.as_struct()
        n = self.n_reads

        def view(p, cnt):
            if cnt == 0:
                return np.zeros(0, np.ctypeslib.as_array(p, shape=(1,)).dtype)
            return np.ctypeslib.as_array(p, shape=(cnt,))
        cig_off = view(r.cigar_off, n + 1)
        seq_off = view(r.seq_off, n + 1)
        name_off = view(r.name_off, n + 1)
        return {"n_reads": n, "pos": view(r.pos, n), "flag": view(r.flag, n), "l_qseq": view(r.l_qseq, n),
                "next_tid": view(r.next_tid, n), "next_pos": view(r.next_pos, n), "tlen": view(r.tlen, n), "name_off": name_off,
                "names": np.ctypeslib.as_array(C.cast(r.names, C.POINTER(C.c_uint8)), shape=(max(1, int(name_off[n]) if n else 1),)),
                "tid": view(r.tid, n), "cigar_off": cig_off, "cigar": view(r.cigar, max(1, self.n_cigar)),
                "seq_off": seq_off, "seq": view(r.seq, max(1, int(seq_off[n]) if n else 1)),
                "qual": view(r.qual, max(1, self.n_qual)), "mapq": self.mapq(), "_owner": self}

    def mapq(self):
        """MAPQ of every read, uint8 [n_reads] (a copy; struct tcmi_reads carries none)."""
        p = C.POINTER(C.c_uint8)()
        check(lib().tcmi_bam_mapq(self.handle, C.byref(p)))
        return np.ctypeslib.as_array(p, shape=(self.n_reads,)).copy() if self.n_reads else np.zeros(0, np.uint8)

    def close(self):
        if self.handle:
            lib().tcmi_bam_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LazyBam:
    """The decoded BAM for the few callers that need reads on the host (insert tokens, Events.py:47-82): decoded by the
    host reader on first use.  The tally itself never needs it — the device decodes the file."""

    def __init__(self, path, threads=0, read_filter=None):
        self.filename, self._threads, self._bam, self.read_filter = str(path), threads, None, read_filter

    def get(self):
        if self._bam is None:
            self._bam = BamFile(self.filename, threads=self._threads, read_filter=self.read_filter)
        return self._bam

    def close(self):
        if self._bam is not None:
            self._bam.close()
            self._bam = None


class DeviceBam:
    """A BAM file headed for the device decoder (tcmi_bamfile): the HOST side only reads the bytes into pinned memory,
    walks the BGZF block headers and parses the BAM header; Context.upload_bamfile() inflates, indexes and packs it with
    HIP kernels.  Raises TcmiError(E_UNSUPPORTED) there when the file needs the host reader (BamFile)."""

    def __init__(self, path):
        h = C.c_void_p()
        check(lib().tcmi_bamfile_read(str(path).encode(), C.byref(h)))
        self.handle = h
        self.filename = str(path)
        fb, ib, nb, ln = (C.c_int64(0) for _ in range(4))
        n_ref, name = C.c_int32(0), C.c_char_p()
        check(lib().tcmi_bamfile_info(h, C.byref(fb), C.byref(ib), C.byref(nb), C.byref(n_ref), C.byref(name), C.byref(ln)))
        self.file_bytes, self.inflated_bytes, self.n_blocks = fb.value, ib.value, nb.value
        self.nreferences = n_ref.value
        self.references = ((name.value or b"").decode(),) if n_ref.value else ()
        self.lengths = (ln.value,) if n_ref.value else ()
        self.all_references, self.all_lengths = _header_refs(lib().tcmi_bamfile_ref, h, n_ref.value)
        self.text = (lib().tcmi_bamfile_text(h) or b"").decode("utf-8", "replace")

    def to_device(self, ctx):
        """The compressed bytes into HBM, to stay (tcmi_bamfile_to_device): uploads of this file then start from device memory."""
        check(lib().tcmi_bamfile_to_device(ctx.handle, self.handle), ctx.handle)
        return self

    def decode_to_host(self, ctx):
        """(for tests / tools) -> (inflated stream uint8, record offsets uint64), both produced by the device."""
        stream = np.empty(max(1, self.inflated_bytes), np.uint8)
        cap = self.inflated_bytes // 36 + 16
        rec = np.empty(cap, np.uint64)
        n = C.c_int64(0)
        check(lib().tcmi_bamfile_decode_to_host(ctx.handle, self.handle, ptr(stream), stream.size, ptr(rec), cap, C.byref(n)), ctx.handle)
        return stream[:self.inflated_bytes], rec[:n.value].copy()

    def close(self):
        if self.handle:
            lib().tcmi_bamfile_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FileRunner:
    """BAM files -> consensus FASTA text (TrueConsense.py:212-264 for many inputs; BASELINE configs[1] / [3]): the native
    runner tcmi_filerunner (csrc/pipeline.cpp).

    Stages per BAM, each on its own threads so that consecutive BAMs overlap:
      read    HOST: file bytes into pinned memory, BGZF block table, BAM header (`decoders` files in flight)
      gpu     H2D of the compressed file, HIP: BGZF inflate + record chain + pack, tally + call, records to pinned host
              memory (`gpu_streams` contexts, each with a stream and a device arena of its own: the kernels of one BAM
              fill the gaps of another's)
      walk    HOST: insert tokens if any candidate, sequential consensus walk, FASTA text (`walkers` threads)
    A file the device decoder does not take (records straddling BGZF blocks, long reads) is decoded by the host reader
    (tcmi_bam_load, `decode_threads` threads) and packed from its flat arrays.  `seconds` accumulates each stage's busy time."""

    def __init__(self, ctx, gff_rows, mincov, include_ambig=True, decoders=2, decode_threads=8, walkers=2, gpu_streams=2, rules=None,
                 variants=None, intervals=None):
        """rules: the ReadRules of the runner's files, set on every context of the runner (Context.set_rules).  variants: the keyword
        arguments of Context.set_variants (ref, min_af, min_alt_depth, min_depth), set on every context likewise: run_files(table=...)
        then writes each sample's variant table.  intervals = ([(start, end)], min_depth) (Context.set_intervals), likewise:
        run_files(stats=True) then returns every sample's interval records."""
        device = ctx.device if isinstance(ctx, Context) else int(ctx)
        self.mincov, self.amb = int(mincov), bool(include_ambig)
        h = C.c_void_p()
        check(lib().tcmi_filerunner_create(int(device), int(decoders), max(1, int(gpu_streams)), int(walkers), int(decode_threads), C.byref(h)))
        self.handle = h
        self.n_ctx = max(1, int(gpu_streams))
        s_ = np.ascontiguousarray([r["start"] for r in gff_rows], np.int64)
        e_ = np.ascontiguousarray([r["end"] for r in gff_rows], np.int64)
        p_ = np.ascontiguousarray([r.get("strand") == "+" for r in gff_rows], np.uint8)
        check(lib().tcmi_filerunner_set_orfs(h, len(s_), ptr(s_), ptr(e_), ptr(p_)))
        self.device_decode = True       # BGZF inflate + record index on the GPU; files it does not take go to the host reader
        self.seconds = {"decode": 0.0, "upload": 0.0, "step": 0.0, "walk": 0.0}
        self.decoded_on = {"device": 0, "host": 0}
        self._device = device
        # every context the same: the runner's host-reader fallbacks take the filter from them, and under a floor a file that leaves
        # the device path is refused, never tallied without it
        self.variant_records = 0        # records of the tables run_files wrote
        for c in self.contexts:
            c.set_rules(rules)
            if variants:
                c.set_variants(**variants)
            if intervals:
                c.set_intervals(*intervals)
        self.n_intervals = len(intervals[0]) if intervals else 0

    @property
    def contexts(self):
        return [_borrowed_context(lib().tcmi_filerunner_ctx(self.handle, k), self._device) for k in range(self.n_ctx)]

    def mate_overlap_totals(self):
        """The mate join's counters summed over the files this runner's contexts decoded (ReadSet.mate_overlap's keys)."""
        keys = (("pairs", "mate_pairs"), ("clipped_reads", "mate_clipped_reads"), ("clipped_columns", "mate_clipped_columns"), ("ambiguous", "mate_ambiguous"))
        return {k: sum(c.stat(s) for c in self.contexts) for k, s in keys}

    def dedup_totals(self):
        """The duplicate rule's counters summed over the files this runner's contexts decoded (ReadSet.dedup's keys)."""
        keys = (("templates", "dedup_templates"), ("duplicate_templates", "duplicate_templates"), ("duplicate_records", "duplicate_records"),
                ("duplicate_sets", "duplicate_sets"))
        return {k: sum(c.stat(s) for c in self.contexts) for k, s in keys}

    def _account(self, status, sec, on):
        """What a run of the native runner reported: every sample's code, the stages' busy seconds, where the files were decoded."""
        self.last_status = status
        for k, v in zip(("decode", "upload", "step", "walk"), sec):
            self.seconds[k] += v
        self.decoded_on["device"] += on[0]
        self.decoded_on["host"] += on[1]

    def _text_run(self, fn, c_items, names, ref_len, max_inserted, *mode):
        """run / run_resident: fn(handle, n, items, names, ref_len, mincov, include_ambig, *mode, out ...) -> list of FASTA texts."""
        n = len(c_items)
        names = names or ["S%d" % i for i in range(n)]
        if n == 0:
            return []
        c_names = (C.c_char_p * n)(*[str(x).encode() for x in names])
        stride = int(ref_len) + int(max_inserted) + max(len(x) for x in names) + 64
        # (positions beyond ref_len that the reads reach lengthen the consensus: the runner reports a too small stride)
        out = np.empty(n * stride, np.uint8)
        lens = np.zeros(n, np.int64)
        status = np.zeros(n, np.int32)
        sec = (C.c_double * 4)()
        on = (C.c_int64 * 2)()
        rc = fn(self.handle, n, c_items, c_names, int(ref_len), self.mincov, int(self.amb), *mode, ptr(out), stride, ptr(lens), ptr(status), sec, on)
        self._account(status, sec, on)
        check(rc)
        return [out[i * stride:i * stride + int(lens[i])].tobytes().decode("ascii") for i in range(n)]

    def run(self, paths, names=None, ref_len=0, max_inserted=4096):
        """-> list of FASTA texts, in input order."""
        c_paths = (C.c_char_p * len(paths))(*[str(p).encode() for p in paths])
        return self._text_run(lib().tcmi_filerunner_run, c_paths, names, ref_len, max_inserted, int(bool(self.device_decode)))

    def run_resident(self, dbams, names=None, ref_len=0, max_inserted=4096):
        """... of DeviceBam objects read before (and, after DeviceBam.to_device, resident in HBM): no read stage, no PCIe copy of
        the file inside the run.  -> list of FASTA texts, in input order."""
        c_files = (C.c_void_p * len(dbams))(*[d.handle for d in dbams])
        return self._text_run(lib().tcmi_filerunner_run_resident, c_files, names, ref_len, max_inserted)

    def set_outputs(self, ref_id, ref_seq, vcf_head, gff_head, gff_row_columns):
        """What the native VCF / GFF writers need besides a sample's walk (run_files): the reference's first record, the complete
        VCF header text, the GFF header text, and per GFF row [source, type, score, strand, phase, attributes]."""
        flat = [str(c).encode() for row in gff_row_columns for c in row]
        arr = (C.c_char_p * max(1, len(flat)))(*flat)
        check(lib().tcmi_filerunner_set_outputs(self.handle, str(ref_id).encode(), str(ref_seq).encode(), str(vcf_head).encode(),
                                                str(gff_head).encode(), len(gff_row_columns), arr))

    def run_files(self, paths, names, fasta, vcf=None, gff=None, doc=None, ref_len=0, table=None, stats=False):
        """BAM files -> per sample its consensus FASTA and (lists, entries may be None) VCF, corrected GFF, coverage TSV and — table,
        with the runner's `variants` setting — variant table, all written by the native runner's walker threads.  Raises what the reference raises (KeyError, ZeroDivisionError) for the first
        sample that fails; last_status has every sample's code.  stats (with the runner's `intervals` setting): -> the samples'
        interval records, a structured array [n samples, n intervals] (INTERVAL_DTYPE)."""
        n = len(paths)
        if stats and not self.n_intervals:
            raise ValueError("run_files(stats=True) needs the runner's intervals= setting")
        if n == 0:
            return np.zeros((0, self.n_intervals), INTERVAL_DTYPE) if stats else None
        def arr(xs):
            if xs is None:
                return None
            return (C.c_char_p * n)(*[None if x is None else str(x).encode() for x in xs])
        status = np.zeros(n, np.int32)
        sec = (C.c_double * 4)()
        on = (C.c_int64 * 2)()
        recs = np.zeros((n, self.n_intervals), INTERVAL_DTYPE) if stats else None
        if stats:
            n_var = np.zeros(n, np.int64)
            rc = lib().tcmi_filerunner_run_files_stats(self.handle, n, arr(paths), arr(names), arr(fasta), arr(vcf), arr(gff), arr(doc), arr(table),
                                                       int(ref_len), self.mincov, int(self.amb), int(bool(self.device_decode)), ptr(status), sec, on,
                                                       ptr(n_var), self.n_intervals, ptr(recs))
            self.variant_records += int(n_var.sum())
        elif table is None:
            rc = lib().tcmi_filerunner_run_files(self.handle, n, arr(paths), arr(names), arr(fasta), arr(vcf), arr(gff), arr(doc), int(ref_len),
                                                 self.mincov, int(self.amb), int(bool(self.device_decode)), ptr(status), sec, on)
        else:
            n_var = np.zeros(n, np.int64)
            rc = lib().tcmi_filerunner_run_files_table(self.handle, n, arr(paths), arr(names), arr(fasta), arr(vcf), arr(gff), arr(doc), arr(table),
                                                       int(ref_len), self.mincov, int(self.amb), int(bool(self.device_decode)), ptr(status), sec, on,
                                                       ptr(n_var))
            self.variant_records += int(n_var.sum())
        self._account(status, sec, on)
        _check_walk(rc, (lib().tcmi_last_error(None) or b"").decode("utf-8", "replace"), KeyError)
        return recs

    def close(self):
        if self.handle:
            lib().tcmi_filerunner_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
