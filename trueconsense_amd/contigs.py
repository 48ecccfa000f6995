"""--per-contig: one consensus per record of a multi-record reference, from ONE decode of the BAM.

Contract: every contig c of the FASTA gets exactly what the single-contig command line gives on c's share of the inputs (the reads
mapped to c with their tid rewritten to 0 and one @SQ, the FASTA record c alone, the GFF rows whose seqid is c), run with
`-name {name}_{c}`.  Mechanism: a contig layout (tcmi_ctx_set_layout) maps reference t onto the positions
[shift[t], shift[t] + slot[t]) of ONE count matrix.  A BAM sorted by (tid, pos) stays sorted on that axis, so the decode, the
packer, the tally and the call run once over all contigs; each contig's results are its slice.

Slots are laid out in BAM header order (that keeps the sort order), one per header reference that the FASTA names:
slot[t] = round_up(max(FASTA length, @SQ LN) + GUARD, 256).  GUARD positions take reads that overhang the contig's end (the
single-contig path grows its matrix for them); a read that ends beyond its slot is refused, never tallied into the next slot.
Reads on references the FASTA does not name are dropped like unmapped reads.
"""
from __future__ import annotations

import gzip
import re
import struct
import sys
from datetime import date

import numpy as np

from . import _ffi, _state
from .cli_args import amplicon_intervals, amplicons_of, rules_of, variants_of
from .cli_tables import (StreamCounts, codon_frames, codon_part_of_columns, dedup_stats, mate_stats, part_of_columns, write_amplicon_reads,
                         write_amplicon_table, write_codon_table, write_tables)
from .engine import BamFile, ReadRules, modal_tokens
from .Events import _parse_token, candidates_from_flags
from .io import fasta
from .indexing import Gffindex, device_readset
from .io.gff import GFF3_COLUMNS, GFFDataFrame
from .Outputs import _VCF_HEAD, _gff_line, vcf_text
from .Sequences import consensus_from_records

GUARD = 4096            # positions behind a contig's end that its slot keeps for reads overhanging it
SLOT_ALIGN = 256
AXIS_LIMIT = 1 << 29    # TCMI_F_EVPOS: the positions of one count matrix stay below this


class ContigError(Exception):
    """An input the per-contig path refuses (the command line prints it and exits 1)."""


def bam_header_refs(path):
    """(names, lengths) of the @SQ references of a BAM file's binary header, read through gzip on the host: no GPU, no decode
    of the alignment records (BGZF is a series of gzip members)."""
    with gzip.open(path, "rb") as fh:
        def take(n):
            b = fh.read(n)
            if len(b) != n:
                raise ContigError("%s: truncated BAM header" % path)
            return b
        if take(4) != b"BAM\1":
            raise ContigError("%s: not a BAM file" % path)
        (l_text,) = struct.unpack("<i", take(4))
        take(l_text)
        (n_ref,) = struct.unpack("<i", take(4))
        names, lens = [], []
        for _ in range(n_ref):
            (l_name,) = struct.unpack("<i", take(4))
            names.append(take(l_name).rstrip(b"\0").decode())
            lens.append(struct.unpack("<i", take(4))[0])
    return names, lens


def layout_for(records, header_names, header_lengths):
    """FASTA records + BAM header -> (shift[n_hdr], slot[n_hdr], axis length).  Raises ContigError for a FASTA record that names
    no @SQ of the BAM, or an axis beyond 2^29 positions."""
    index = {n: t for t, n in enumerate(header_names)}
    for rid, _ in records:
        if rid not in index:
            raise ContigError('FASTA record "%s" names no reference of the BAM header' % rid)
    flen = {rid: len(seq) for rid, seq in records}
    shift = np.full(len(header_names), -1, np.int64)
    slot = np.zeros(len(header_names), np.int64)
    at = 0
    for t, name in enumerate(header_names):
        if name not in flen:
            continue
        n = max(flen[name], int(header_lengths[t])) + GUARD
        n = (n + SLOT_ALIGN - 1) // SLOT_ALIGN * SLOT_ALIGN
        shift[t], slot[t] = at, n
        at += n
    if at >= AXIS_LIMIT:
        raise ContigError("the contigs' slots take %d positions, more than 2^29" % at)
    return shift, slot, at


def _gff_of(gffobj, seqid):
    """The GFF as the split file (this contig's rows only) reads: its rows, and its columns built from those rows alone."""
    rows = [r for r in gffobj.rows if r.get("seqid") == seqid]
    cols = list(GFF3_COLUMNS)
    for r in rows:
        for k in r:
            if k not in cols:
                cols.append(k)
    return GFFDataFrame(gffobj.header, rows, cols)


_SLOT_OVF = re.compile(r"read (\d+) on reference (\d+) ends past the end of its contig's slot")


def _name_slot_overrun(err, host, header_names):
    """The library's refusal of a read past its slot, worded with the read's and the contig's names."""
    m = _SLOT_OVF.search(str(err))
    if not m:
        return err
    i, t = int(m.group(1)), int(m.group(2))
    a = host.arrays()
    read = bytes(a["names"][int(a["name_off"][i]):int(a["name_off"][i + 1])]).decode("ascii", "replace") if i < a["n_reads"] else "#%d" % i
    contig = header_names[t] if 0 <= t < len(header_names) else "#%d" % t
    return ContigError('read "%s" on contig "%s" ends past the end of the contig\'s slot (its length + %d positions)' % (read, contig, GUARD))


def axis_reference(records, header_names, shift, axis_len):
    """The reference on the layout's axis (what the variant table reads): every kept contig's sequence at its shift, zero bytes
    elsewhere — guard columns and the slots' padding give no record."""
    index = {n: t for t, n in enumerate(header_names)}
    ref = np.zeros(max(int(axis_len), 1), np.uint8)
    for rid, seq in records:
        s = int(shift[index[rid]])
        ref[s:s + len(seq)] = np.frombuffer(seq.encode("latin-1"), np.uint8)
    return ref


def step_contigs(ctx, path, shift, slot, axis_len, mincov, include_ambig, header_names, threads=0, want_counts=True, rules=ReadRules(),
                 info=None, variants=None, intervals=None, on_readset=None, need_device=None):
    """One decode + pack + tally + call of the whole file under the layout -> (plain, alt, flags, int32 [axis_len, 7] counts,
    per-reference extents, mapped reads dropped, host BamFile or None); counts None unless `want_counts`.  The device decoder
    first; a file it declines goes through the host reader (same layout).  rules: the ReadRules the context is under for this call
    (Context.rules).  Its read_filter: extents, `dropped` and the host BamFile see the passing records only; info (a dict) receives
    "reads" (the file's records) and "reads_filtered".  Its min_baseq: the base-quality floor of the count matrix; above 0 a file the
    device decoder declines is refused (the host packer knows no floor).  Its primers = (rows on the AXIS, slack)
    (io.primers.rows_for_layout shifts a BED's rows): likewise; info then receives "reads_primer_masked" too.
    variants = the keyword arguments of Context.set_variants (ref: the reference on the axis, axis_reference): the step also lists
    the variant table's records, which info receives as "variant_table".  intervals = ([(start, end)] on the axis, min_depth)
    (Context.set_intervals): the step also computes the amplicon table's records, which info receives as "amplicon_table".
    on_readset(ctx, read set): called behind the step — info's tables are filled, the layout is still set — while the read set's
    decoded stream is resident; need_device: the flag on whose behalf a file the device decoder declines is refused then (reads
    decoded on the host leave no stream on the device), as indexing.build_counts takes them.  The rules' mate_overlap (pairs never
    cross contigs): info then receives the join's counters as "mate_overlap" (ReadSet.mate_overlap); its dedup (a key holds its
    reference): likewise "dedup" (ReadSet.dedup)."""
    n_ref = len(shift)
    ctx.set_layout(shift, slot)
    if variants:
        ctx.set_variants(**variants)
    if intervals:
        ctx.set_intervals(*intervals)
    host = None
    with ctx.rules(rules):
        try:
            rs = device_readset(ctx, path, need=need_device)    # (the floor it refuses under is the one just set)
            if rs is None:
                host = BamFile(path, threads=threads, read_filter=rules.read_filter)
                try:
                    rs = ctx.upload(host)
                except _ffi.TcmiError as e:
                    raise _name_slot_overrun(e, host, header_names) from e
            try:
                ext, dropped = rs.ref_extents(n_ref), rs.dropped()
                if info is not None:
                    info.update(reads=host.n_records if host is not None else rs.n_reads, reads_filtered=host.n_removed if host is not None else rs.filtered)
                    if rules.primers:                               # (only under a table: the dict of before otherwise)
                        info["reads_primer_masked"] = rs.primer_masked_reads
                    if rules.mate_overlap:
                        info["mate_overlap"] = dict(rs.mate_overlap)
                    if rules.dedup:
                        info["dedup"] = dict(rs.dedup)
                plain, alt, flags, counts = ctx.step(rs, max(axis_len, 1), mincov, include_ambig, want_counts=want_counts)
                if variants and info is not None:
                    info["variant_table"] = ctx.step_variants()
                if intervals and info is not None:
                    info["amplicon_table"] = ctx.step_intervals()
                if on_readset is not None:                          # (the layout is still set: the read set's shifts are the tables')
                    on_readset(ctx, rs)
            finally:
                rs.free()
        finally:
            ctx.set_layout()
            if variants:
                ctx.set_variants()
            if intervals:
                ctx.set_intervals()
    return plain, alt, flags, counts, ext, dropped, host


def run(a):
    """The whole --per-contig flow of the command line: every output is computed before the first file is written.
    -> {"contigs": n, "dropped_reads": mapped reads on BAM references the FASTA does not name, "reads", "reads_filtered"}."""
    seen, got = {}, {}
    name, mincov, amb = a.samplename, a.coverage_level, a.noambiguity is False
    records = fasta.read_records(a.reference)
    hdr_names, hdr_lens = bam_header_refs(a.input)
    shift, slot, axis_len = layout_for(records, hdr_names, hdr_lens)
    index = {n: t for t, n in enumerate(hdr_names)}
    gffobj = Gffindex(a.features)
    ctx = _state.default_context()
    rules = rules_of(a, (hdr_names, shift))
    seen["primers"] = len(rules.primers[0]) if rules.primers else 0
    want_counts = a.variants is not None or a.depth_of_coverage is not None     # (the VCF's DP and the TSV read the counts)
    amps = amplicons_of(a, (hdr_names, shift))      # (each contig's amplicons shifted by its slot; none left: an argument error)
    seen["amplicons"] = len(amps) if amps else 0
    want = StreamCounts(a, (hdr_names, shift))      # (likewise, for --amplicon-reads; one call each over all contigs' columns on the shifted axis)
    if want.codons:                                 # (each contig's CDS rows shifted by its slot; the table's invariant reads the counts)
        want.frames = codon_frames(gffobj.rows, (hdr_names, shift))
        want_counts = True
    axis_ref = axis_reference(records, hdr_names, shift, axis_len) if a.variant_table is not None else None
    var = dict(variants_of(a), ref=axis_ref) if axis_ref is not None else None
    plain, alt, flags, counts, ext, dropped, host = step_contigs(ctx, a.input, shift, slot, axis_len, mincov, amb, hdr_names,
                                                                 threads=a.threads, want_counts=want_counts, rules=rules, info=seen, variants=var,
                                                                 intervals=(amplicon_intervals(amps), mincov) if amps else None,
                                                                 on_readset=lambda c, rs: got.update(want.count(c, rs, seen.get("variant_table"))),
                                                                 need_device=want.need)
    seen.update(mate_stats(a.mate_overlap, seen.pop("mate_overlap", None)))
    seen.update(dedup_stats(a.dedup, seen.pop("dedup", None)))
    seen.update(want.stats(got))
    seen.setdefault("reads_primer_masked", 0)
    table = seen.pop("variant_table", None)
    arecs = seen.pop("amplicon_table", None)
    seen["amplicons_below"] = 0 if arecs is None else int((arecs["below"] > 0).sum())

    # every contig's slice of the call records (the call is position-local: a slice's records are the split run's)
    per = []
    for rid, seq in records:
        t = index[rid]
        s = int(shift[t])
        L = max(len(seq), int(ext[t]), 1)
        per.append((rid, seq, s, counts[s:s + L] if want_counts else None, plain[s:s + L], alt[s:s + L], flags[s:s + L]))

    # insert candidates of all contigs, resolved in one sweep over the reads on the axis (Events.py:47-82 per contig); the
    # device sweep does not take a layout, so the host reader decodes the file for it (as the single-contig path's LazyBam does)
    cand = [(k, s + p) for k, (_, _, s, _, _, _, f) in enumerate(per) for p in candidates_from_flags(f)]
    toks = {}
    if cand:
        if host is None:
            host = BamFile(a.input, threads=a.threads, read_filter=rules.read_filter)
        toks = {p: t for p, (t, _) in modal_tokens(host, [g for _, g in cand], layout=(shift, slot)).items()}

    today = date.today().strftime("%Y%m%d")
    fa, vcf, gff_out, doc = [], [], [], []
    for k, (rid, seq, s, c, plain, alt, flags) in enumerate(per):
        ins = {}
        for kk, g in cand:
            if kk != k:
                continue
            bases, size = _parse_token(toks.get(g))
            if bases is not None and size is not None:
                ins[g - s] = {size: bases}
        hasins, insertpositions = (True, ins) if ins else (False, None)
        cname = "%s_%s" % (name, rid)
        gdict = _gff_of(gffobj, rid).index_dict(seqid=cname)
        consensus, newgff = consensus_from_records(plain, alt, flags, gdict, insertpositions, True)
        fa.append(">%s mincov=%s\n%s\n" % (cname, mincov, consensus))
        if a.output_gff is not None:
            gff_out.extend(_gff_line(row) for row in newgff.values())
        if a.variants is not None:
            noins = consensus_from_records(plain, alt, flags, gdict, insertpositions, False)[0]
            text = vcf_text(today, sys.argv[1:], a.reference, rid, list(seq), noins, _state.IndexDict(c), mincov, hasins,
                            insertpositions)
            vcf.append("".join(ln for ln in text.splitlines(True) if not ln.startswith("#")))
        if a.depth_of_coverage is not None:
            doc.append("".join("%s\t%d\t%d\n" % (rid, i + 1, v) for i, v in enumerate(c[:, 0].tolist())))

    if a.output_gff is not None:
        with open(a.output_gff, "w") as out:
            out.write(gffobj.header.raw_text)
            out.writelines(gff_out)
    if a.variants is not None:
        head = _VCF_HEAD.format(date=today, argv=" ".join(sys.argv[1:]), ref=a.reference, contig=records[0][0])
        contig_line = "##contig=<ID=%s>\n" % records[0][0]
        head = head.replace(contig_line, "".join("##contig=<ID=%s>\n" % rid for rid, _ in records))
        with open(a.variants, "w") as out:
            out.write(head + "".join(vcf))
    if a.depth_of_coverage is not None:
        with open(a.depth_of_coverage, "w") as out:
            out.write("".join(doc))
    # one file per table, the contigs in axis order; rows carry the contig's name and its own positions, from the counts of its own
    # columns: no pair across two contigs.  The reference ends with the contig: a deletion that runs past its end reads N there.
    parts = [part_of_columns(table, got, s, s + len(seq), rid, axis_ref[:s + len(seq)], s)
             for rid, seq, s, *_ in (sorted(per, key=lambda x: x[2]) if table is not None else ())]
    seen.update(write_tables(a, parts, want))
    if want.codons:                                 # (its keys only with the flag)
        seen.update(write_codon_table(a, [codon_part_of_columns(got, *want.frames, counts, s, s + len(seq), rid, axis_ref[:s + len(seq)], s)
                                          for rid, seq, s, *_ in sorted(per, key=lambda x: x[2])], want))
    if arecs is not None:                           # one table: REGION is the contig, positions are the contig's own
        write_amplicon_table(a.amplicon_table, [(name, arecs)], amps)
    if want.areads:                                 # one file: REGION is each amplicon's contig
        write_amplicon_reads(a.amplicon_reads, name, got["amplicon_reads"], want.areads[0])
    with open(a.output, "w") as out:
        out.write("".join(fa))
    return dict({"contigs": len(records), "dropped_reads": int(dropped)}, **seen)
