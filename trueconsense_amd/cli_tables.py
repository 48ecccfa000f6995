"""The command line's tables: what is counted behind the step (StreamCounts) and written from it.  TablePart is one part of the
tables that hang on the variant table's records — a sample, or a contig of the axis (part_of_columns) — and write_tables their one
writer, for every runner; beside them the codon table's sibling (CodonPart, codon_part_of_columns, write_codon_table: it hangs on
the GFF's reading frames and the count matrix as well), the amplicon tables' writers and the --stats keys of the counts."""
from __future__ import annotations

import os
from typing import NamedTuple

from . import engine
import numpy as np

from .cli_args import amplicon_reads_of, codons_of, evidence_of, links_of, strand_of, variants_of


class StreamCounts:
    """What the command line counts behind the step, in the record stream the device decoder leaves resident: --amplicon-reads,
    --variant-strand and --variant-links of the parsed namespace (layout: amplicon_reads_of's).  False when none is asked for.  A
    further count of this kind is one more line in each method here, and one _sum_to_root call in distributed.consensus_split_bamfile."""
    KEYS = ("amplicon_reads", "variant_strand", "variant_links")    # count's keys; the order of consensus_split_bamfile's extra parts
    # (--indel-table's "indel_events" is no such part: its lists have no fixed length, and -i --gpus N is refused with it)
    indels = None                                                   # --indel-table's file
    # (nor is --variant-evidence's "variant_evidence": its sums would reduce like the strand counts, but the split's keywords are fixed)
    evidence = None                                                 # --variant-evidence's (file, thresholds)
    # (nor is --codon-table's "codon_counts", for the same reason)
    codons = None                                                   # --codon-table's file
    frames = None                                                   # ... and its reading frames on the axis: codon_frames' (cds, names), set by the runner

    def __init__(self, a, layout=None):
        self.areads, self.srule, self.links = amplicon_reads_of(a, layout), strand_of(a), links_of(a)
        self.indels = getattr(a, "indel_table", None)
        self.evidence = evidence_of(a)
        self.codons = codons_of(a)
        self.lists_records = bool(self.srule or self.links or self.indels or self.evidence or self.codons)     # must the step list the variant table's records?
        self.variants = variants_of(a) if self.lists_records else None
        # the flag named when the file leaves the device path (indexing.device_readset's `need`)
        self.need = "--variant-strand" if self.srule else "--variant-links" if self.links else "--indel-table" if self.indels else \
            "--variant-evidence" if self.evidence else "--amplicon-reads" if self.areads else "--codon-table" if self.codons else None

    def __bool__(self):
        return self.need is not None

    def count(self, ctx, rs, records=None):
        """The counts asked for on read set rs, resident on ctx, under KEYS; records: the variant table's records of the step (fetched
        from the context when not given)."""
        got = {}
        if self.areads:
            got["amplicon_reads"] = ctx.amplicon_reads(rs, *self.areads[1:])
        if self.lists_records and records is None:
            records = ctx.step_variants()
        if self.srule:
            got["variant_strand"] = ctx.strand_counts_of(rs, records)
        if self.links:
            got["variant_links"] = ctx.link_counts_of(rs, records, self.links[1])
        if self.indels:
            got["indel_events"] = ctx.indel_events_of(rs, records, **self.variants)
        if self.evidence:
            got["variant_evidence"] = ctx.evidence_counts_of(rs, records)
        if self.codons:
            got["codon_counts"] = ctx.codon_counts_of(rs, records, (self.frames or codon_frames(()))[0])
        return got

    def split_kwargs(self, ref):
        """distributed.consensus_split_bamfile's keyword arguments of the counts, the file being aligned to the sequence `ref`"""
        var = dict(self.variants, ref=ref) if self.lists_records else None
        return dict(amplicon_reads=self.areads[1:] if self.areads else None, variant_strand=var if self.srule else None,
                    variant_links=(var, self.links[1]) if self.links else None)

    def from_parts(self, parts):
        """rank 0's return_parts tuple of consensus_split_bamfile(**split_kwargs) -> (count's dict, the records the root listed or None)"""
        got = dict(zip([k for k, on in zip(self.KEYS, (self.areads, self.srule, self.links)) if on], parts[3:]))
        records = None
        for k in self.KEYS[1:]:
            if k in got:
                records, got[k] = got[k]
        return got, records

    def stats(self, got=None):
        """the --stats keys of --amplicon-reads (write_tables returns those of the tables on the variant table's records)"""
        r = got["amplicon_reads"]["reads"] if got and "amplicon_reads" in got else (0, 0)
        return {"amplicon_reads_ambiguous": int(r[-2]), "amplicon_reads_unassigned": int(r[-1])}


class TablePart(NamedTuple):
    """One part of the tables on the variant table's records: a sample, or one contig of the axis.  records: the variant table's
    records of the part; region, ref (the reference on the records' axis), pos_offset: what the engine.*_text functions take; strand,
    links, evidence: StreamCounts.count's arrays at the part's columns; indels: its (events, text, totals).  None: not asked for."""
    records: object
    region: str
    ref: object
    pos_offset: int = 0
    strand: object = None
    links: object = None
    indels: object = None
    evidence: object = None


def part_of_columns(table, got, lo, hi, region, ref, pos_offset):
    """The part of the axis' columns [lo, hi) — a contig's own, without its slot's guard columns: the records `table` and every count of
    `got` (StreamCounts.count's dict) cut by its position key, "pos", the link counts by "a", so no link row crosses two parts."""
    def cut(x, key="pos"):
        return None if x is None else x[(x[key] >= lo) & (x[key] < hi)]
    ind = got.get("indel_events")
    return TablePart(cut(table), region, ref, pos_offset, cut(got.get("variant_strand")), cut(got.get("variant_links"), "a"),
                     None if ind is None else (cut(ind[0]), ind[1], cut(ind[2])), cut(got.get("variant_evidence")))


def link_stats(text=""):
    """the --stats counters of --variant-links' rows (no rows: zeros)"""
    out = {"variant_link_rows": text.count("\n")}
    out.update({"variant_links_" + w.lower(): text.count("\t%s\n" % w) for w in engine.LINK_PHASES})
    return out


def evidence_stats(text=""):
    """the --stats counters of --variant-evidence's rows (no rows: zeros)"""
    words = [ln.rsplit("\t", 1)[-1].split(",") for ln in text.splitlines()]
    return {"variant_evidence_" + w.lower(): sum(w in row for row in words) for w in engine.EVIDENCE_NAMES}


def _write(path, header, text_of, parts):
    """One table's file: the header line, then text_of(part) for every part in order -> the rows' text.  The whole text is built before
    the file is opened: a part whose counts do not add up to its records (TcmiError) leaves the file unwritten."""
    text = "".join(text_of(p) for p in parts)
    with open(path, "w") as out:
        out.write(header + text)
    return text


def write_tables(a, parts, want):
    """--variant-table — with the strand columns under --variant-strand —, --variant-links, --indel-table and --variant-evidence, in that
    order: parts = [TablePart], one per sample or per contig in axis order (link rows never pair two parts), want = StreamCounts(a).
    -> their --stats keys (zeros for what was not asked for; no --variant-table: nothing written, all zeros)."""
    stats = dict(variant_records=0, variant_strand_bias=0, variant_strand_low=0, **link_stats(), **evidence_stats())
    if a.variant_table is None:
        return stats
    stats["variant_records"] = sum(len(p.records) for p in parts)
    if want.srule:
        text = _write(a.variant_table, engine.VARIANTS_STRAND_HEADER,
                      lambda p: engine.variants_strand_text(p.records, p.strand, p.region, p.ref, p.pos_offset, **want.srule), parts)
        stats["variant_strand_bias"], stats["variant_strand_low"] = text.count("\tBIAS\n"), text.count("\tLOW\n")
    else:
        _write(a.variant_table, engine.VARIANTS_HEADER, lambda p: engine.variants_text(p.records, p.region, p.ref, p.pos_offset), parts)
    if want.links:
        path, k, rule = want.links
        stats.update(link_stats(_write(path, engine.VARIANTS_LINKS_HEADER,
                                       lambda p: engine.variants_links_text(p.records, p.links, k, p.region, p.ref, p.pos_offset, **rule), parts)))
    if want.indels:
        _write(want.indels, engine.INDELS_HEADER, lambda p: engine.indels_text(*p.indels, p.records, p.region, p.ref, p.pos_offset), parts)
    if want.evidence:
        path, rule = want.evidence
        stats.update(evidence_stats(_write(path, engine.VARIANTS_EVIDENCE_HEADER,
                                           lambda p: engine.variants_evidence_text(p.records, p.evidence, p.region, p.ref, p.pos_offset, **rule), parts)))
    return stats


class CodonPart(NamedTuple):
    """One part of the codon table: a sample, or one contig of the axis.  counts: StreamCounts.count's "codon_counts" at the part's
    codons; frames, names: its reading frames on the axis (codon_frames); region, ref, pos_offset: as TablePart's; matrix: the count
    matrix [L, 7] on the counts' axis, which the counts must add up to."""
    counts: object
    frames: object
    names: list
    region: str
    ref: object
    pos_offset: int
    matrix: object


def codon_frames(rows, layout=None):
    """The GFF's reading frames on the axis -> (engine.CDS_DTYPE array, their names): every row (io.gff's dicts) of type CDS with
    strand + or - is one frame, its phase column '.' read as 0; a row with another strand, phase or without columns is no frame.
    layout = (the BAM header's names, their shifts): each contig takes its own rows by seqid, shifted by its slot (a seqid the layout
    drops or does not know: no frame); without one every CDS row counts, the GFF being the one reference's.  A frame's name is the
    row's Name, else ID, else gene attribute, else CDS_{start}_{end}."""
    shift_of = None if layout is None else {n: int(s) for n, s in zip(*layout)}
    cds, names = [], []
    for r in rows:
        strand, phase = r.get("strand"), r.get("phase")
        if r.get("type") != "CDS" or strand not in ("+", "-") or phase not in (".", "0", "1", "2"):
            continue
        sh = 0 if shift_of is None else shift_of.get(r.get("seqid"), -1)
        start, end = int(r["start"]) - 1 + sh, int(r["end"]) + sh          # (GFF: 1-based, closed)
        if sh < 0 or start < sh or end < start or end >= 1 << 29:
            continue
        cds.append((start, end, 1 if strand == "+" else -1, 0 if phase == "." else int(phase)))
        names.append(next((str(r[k]) for k in ("Name", "ID", "gene") if isinstance(r.get(k), str) and r[k]), "CDS_%d_%d" % (r["start"], r["end"])))
    return np.array(cds, engine.CDS_DTYPE), names


def codon_part_of_columns(got, frames, names, matrix, lo, hi, region, ref, pos_offset):
    """The codon table's part of the axis' columns [lo, hi) — a contig's own: the counts of `got` (StreamCounts.count's dict) and the
    frames that start there."""
    counts = got.get("codon_counts")
    counts = np.zeros(0, engine.CODON_DTYPE) if counts is None else counts[(counts["pos"] >= lo) & (counts["pos"] < hi)]
    keep = [k for k in range(len(frames)) if lo <= int(frames["start"][k]) < hi]
    return CodonPart(counts, frames[keep], [names[k] for k in keep], region, ref, pos_offset, matrix)


def write_codon_table(a, parts, want):
    """--codon-table: parts = [CodonPart], one per sample or per contig in axis order, want = StreamCounts(a).  Like _write, the whole
    text is built before the file is opened: a part whose counts do not add up to the matrix (TcmiError) leaves the file unwritten.
    -> its --stats keys (zeros, and nothing written, without the flag)."""
    stats = dict(codon_frames=0, codon_codons=0, codon_rows=0, codon_rows_multi=0)
    if not want.codons:
        return stats
    text = _write(want.codons, engine.CODONS_HEADER,
                  lambda p: engine.codons_text(p.counts, p.frames, p.names, p.matrix, p.region, p.ref, p.pos_offset, **want.variants), parts)
    rows = [ln.split("\t") for ln in text.splitlines()]
    stats.update(codon_frames=sum(len(p.frames) for p in parts), codon_codons=sum(len(p.counts) for p in parts), codon_rows=len(rows),
                 codon_rows_multi=sum(int(r[10]) >= 2 for r in rows))
    return stats


def mate_stats(on, counters):
    """The --stats keys of --mate-overlap from a read set's counters (ReadSet.mate_overlap; None: none were fetched)."""
    c = counters or {}
    return {"mate_overlap": bool(on), "mate_pairs": int(c.get("pairs", 0)), "reads_mate_clipped": int(c.get("clipped_reads", 0)),
            "columns_mate_clipped": int(c.get("clipped_columns", 0)), "mate_ambiguous": int(c.get("ambiguous", 0))}


def dedup_stats(on, counters):
    """The --stats keys of --dedup from a read set's counters (ReadSet.dedup; None: none were fetched)."""
    c = counters or {}
    return {"dedup": bool(on), "dedup_templates": int(c.get("templates", 0)), "duplicate_templates": int(c.get("duplicate_templates", 0)),
            "duplicate_records": int(c.get("duplicate_records", 0)), "duplicate_sets": int(c.get("duplicate_sets", 0))}


def amplicon_reads_text(sample, counts, amps):
    """One sample's rows of --amplicon-reads: counts = Context.amplicon_reads' n + 2 rows (or an [n + 2, 2] array), amps their n
    amplicons.  REGION is the amplicon's contig; then the two rows of the records inside several amplicons and inside none."""
    rows = [(int(r[0]), int(r[1])) for r in counts]
    if len(rows) != len(amps) + 2:
        raise ValueError("amplicon_reads_text: %d amplicons, %d rows of counts" % (len(amps), len(rows)))
    text = ["%s\t%s\t%s\t%s\t%d\t%d\n" % (sample, m.chrom, m.name, m.pool, r, f) for m, (r, f) in zip(amps, rows)]
    text += ["%s\t*\t%s\t*\t%d\t0\n" % (sample, what, rows[len(amps) + k][0]) for k, what in enumerate(("*ambiguous", "*unassigned"))]
    return "".join(text)


def write_amplicon_reads(path, sample, counts, amps):
    """--amplicon-reads: the header line, then amplicon_reads_text's rows."""
    _write(path, engine.AMPLICON_READS_HEADER, lambda c: amplicon_reads_text(sample, c, amps), [counts])


def amplicon_rows(records, sample, amps):
    """One sample's rows of the amplicon table: records[i] belongs to amps[i]; REGION is the amplicon's contig and the positions are
    the contig's own (tcmi_amplicons_text, one call per contig)."""
    from itertools import groupby
    text, i = [], 0
    for (chrom, sh), grp in groupby(amps, key=lambda x: (x[0].chrom, x[1])):
        grp = list(grp)
        text.append(engine.amplicons_text(records[i:i + len(grp)], sample, chrom, [m.name for m, _ in grp], [m.pool for m, _ in grp],
                                          [m.start + sh for m, _ in grp], sh))
        i += len(grp)
    return "".join(text)


def write_amplicon_table(path, samples, amps):
    """--amplicon-table: the header line, then for every (sample name, its records) the sample's rows."""
    _write(path, engine.AMPLICONS_HEADER, lambda s: amplicon_rows(s[1], s[0], amps), samples)


def join_amplicon_parts(path, parts, n_samples, per_sample):
    """--batch --gpus N: part k (a child's table) holds the rows of samples k, k + N, ... — `per_sample` lines each; -> FILE with
    every sample's rows in manifest order, and the parts removed."""
    rows = []
    for part in parts:
        with open(part) as fh:
            lines = fh.read().split("\n")[1:]
        rows.append(lines)
    n = len(parts)
    with open(path, "w") as out:
        out.write(engine.AMPLICONS_HEADER)
        for i in range(n_samples):
            k, j = i % n, i // n
            for line in rows[k][j * per_sample:(j + 1) * per_sample]:
                out.write(line + "\n")
    for part in parts:
        os.remove(part)
