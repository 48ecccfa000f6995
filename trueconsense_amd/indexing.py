"""Stage A host side — same surface as TrueConsense/indexing.py.

BuildIndex (indexing.py:75-154) keeps its signature and its return value (a DataFrame indexed
1..L with columns coverage,A,T,C,G,X,I) but the pileup and the per-token loop
(indexing.py:100-132) run as one HIP tally kernel over the decoded reads.
"""
from __future__ import annotations

from . import _state
from ._ffi import COLS
from . import _ffi
from .engine import BamFile, DeviceBam, LazyBam
from .io import fasta, gff


def Readbam(f):
    """indexing.py:6-19 — the BAM as the later stages see it (plays pysam.AlignmentFile's role downstream): decoded on the
    host only when somebody asks for reads (insert tokens)."""
    return f if isinstance(f, (BamFile, LazyBam)) or hasattr(f, "modal_token") else LazyBam(f)    # (modal_token: tokens resolved beforehand, e.g. gathered from several GPUs)


def Gffindex(file):
    """indexing.py:22-36 — object with `.df` (DataFrame) and `.header.raw_text`."""
    return gff.read_gff(file)


def read_override_index(f):
    """indexing.py:39-52."""
    import pandas as pd                                 # (where a DataFrame is the interface: imported when it is asked for)
    return pd.read_csv(f, sep=",", compression="gzip", index_col=0)


def Override_index_positions(index, override_data):
    """indexing.py:55-72."""
    index.loc[override_data.index, :] = override_data[:]
    return index


def device_readset(ctx, path, blocks=None, need=None):
    """The device path, or why not: the file at `path` (blocks = (first, count): that range of its BGZF blocks) decoded and packed by
    ctx's device decoder -> ReadSet; None when the decoder declines the file (E_UNSUPPORTED) and the host reader may take it.  Under
    a base-quality floor, a primer table, the mate-overlap rule or the duplicate rule (ctx.read_rules, in that order) the host reader may not: the refusal is raised with its
    reason; likewise when the caller names a flag that `need`s the device path (--amplicon-reads counts in the decoded stream)."""
    d = DeviceBam(path)
    try:
        return ctx.upload_bamfile(d, blocks)
    except _ffi.TcmiError as e:
        if e.code != _ffi.E_UNSUPPORTED:
            raise
        r = ctx.read_rules
        for flag, why in ((r.min_baseq and "--min-baseq %d" % r.min_baseq, "the host packer knows no base-quality floor"),
                          (r.primers and "--primers", "the host packer knows no primer mask"),
                          (r.mate_overlap and "--mate-overlap", "the host packer joins no mates"),
                          (r.dedup and "--dedup", "the host packer finds no duplicate templates"),
                          (need, "it counts the records in the stream the device decoded")):
            if flag:                                # (the first in this order: the floor, the table, the mate rule, the duplicate rule, the caller's flag)
                raise _ffi.TcmiError(_ffi.E_UNSUPPORTED, "%s needs the device path (%s), which %s left: %s" % (flag, why, path, e)) from e
        return None
    finally:
        d.close()


def build_counts(bamfile, ref, ctx=None, on_readset=None, need_device=None):
    """BAM (+ reference FASTA, for its length) -> int32 [L,7] count matrix on the GPU path.  A path (or LazyBam) is decoded
    ON THE DEVICE (BGZF inflate, record chain, pack: csrc/bam_device.hip, pack_device.hip); files the device decoder
    declines, and BamFile objects, go through the host reader's flat arrays.  A read filter is the context's
    (Context.set_read_filter): the host reader's fallback applies the same one (a LazyBam's own, if it has one); a BamFile is
    taken as it is.  Under a base-quality floor (Context.set_min_base_quality) there is no fallback: the host packer knows no
    floor, and a file the device decoder declines is refused with its reason.  on_readset(ctx, read set): called behind the step,
    while the read set's decoded stream is still resident (Context.amplicon_reads); need_device: the flag on whose behalf a file that
    leaves the device path — a file the decoder declines, a BamFile — is refused instead (device_readset's `need`)."""
    ref_length = fasta.first_length(ref) if isinstance(ref, str) else int(ref)
    ctx = ctx or _state.default_context()
    if not isinstance(bamfile, BamFile):
        path = bamfile.filename if isinstance(bamfile, LazyBam) else str(bamfile)
        rs = device_readset(ctx, path, need=need_device)
        if rs is not None:
            try:
                build_counts.last_reads, build_counts.last_filtered = int(rs.n_reads), int(rs.filtered)
                build_counts.last_primer_masked = int(rs.primer_masked_reads)
                build_counts.last_mate_overlap = dict(rs.mate_overlap)
                build_counts.last_dedup = dict(rs.dedup)
                counts = ctx.step(rs, max(ref_length, rs.max_end, 1), 0, True, want_counts=True)[3]
                if on_readset is not None:
                    on_readset(ctx, rs)
                return counts
            finally:
                rs.free()
        flt = ctx.read_rules.read_filter
        if isinstance(bamfile, LazyBam) and bamfile.read_filter is None:
            bamfile.read_filter = flt
        bamfile = bamfile.get() if isinstance(bamfile, LazyBam) else BamFile(path, read_filter=flt)
    if need_device:
        raise _ffi.TcmiError(_ffi.E_UNSUPPORTED, "%s needs the device path: reads decoded on the host have no record stream on the device" % need_device)
    build_counts.last_reads, build_counts.last_filtered = int(bamfile.n_records), int(bamfile.n_removed)
    return ctx.tally(bamfile, ref_len=ref_length)


build_counts.last_reads = 0         # alignment records of the file the last call read (the command line's --stats)
build_counts.last_filtered = 0      # ... of which failed the read filter
build_counts.last_primer_masked = 0 # piled-up reads with a non-empty primer mask (Context.set_primers)
build_counts.last_dedup = {}        # the duplicate rule's counters, likewise (Context.set_dedup; ReadSet.dedup)
build_counts.last_mate_overlap = {} # the mate join's counters of the last device-decoded file (Context.set_mate_overlap; ReadSet.mate_overlap)


def BuildIndex(bamfile, ref):
    """indexing.py:75-154."""
    counts = build_counts(bamfile, ref)
    import pandas as pd
    df = pd.DataFrame(counts.astype("int64"), columns=list(COLS), index=range(1, len(counts) + 1))
    df.index.name = None
    return df
