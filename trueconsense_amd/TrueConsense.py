"""Command line — same flags, checks and exit codes as TrueConsense/TrueConsense.py:25-264.

    python -m trueconsense_amd.TrueConsense -i x.bam -ref r.fa -gff r.gff -cov 30 -name S -o out.fa
        [-vcf out.vcf] [-doc cov.tsv] [-ogff out.gff] [-t N] [-noambig] [--index-override f.csv.gz]

Additive flags (not in the reference): --device N (GPU ordinal), --stats FILE (JSON timings), the read filter
--min-mapq N / --require-flags F / --exclude-flags F (samtools view -q / -f / -F: a record that fails is ignored as an unmapped
one is; the reference tallies every mapped record), the variant table --variant-table FILE [--min-af F] [--min-alt-depth N]
[--variant-min-depth N] (per position every non-reference allele at or above a frequency, from the count matrix the consensus is
called from; --batch: the manifest's 7th column), the amplicon table --amplicon-table FILE [--amplicon-scheme BED]
[--amplicon-region insert|unique|full] (per amplicon of the primer scheme the mean, median and minimum depth of its columns and
how many lie below -cov, from the same matrix; --batch: one file for all samples), the reads per amplicon --amplicon-reads FILE
[--amplicon-reads-slack N] (per amplicon of the scheme the alignment records whose two ends lie inside it and inside no other, and
how many of them run from its left primer into its right one; records inside several amplicons or inside none are counted as such;
counted on the device in the decoded record stream; not with --batch), the links between the variant table's rows --variant-links FILE
[--link-neighbours K] [--link-min-depth N] [--link-ratio F] (for every two rows at most K distinct positions apart how many alignment
records carry both alleles, one of them or neither, and the phase CIS / TRANS / MIXED / NONE / LOW; counted likewise; needs
--variant-table; not with --batch or --index-override), the indel table --indel-table FILE (one row per insertion or deletion at the
variant table's '+' and '*' positions, with its length, its bases and the records that carry it, under --min-af / --min-alt-depth /
--variant-min-depth; counted likewise; needs --variant-table; not with --batch, --index-override or -i --gpus N), the evidence table
--variant-evidence FILE [--evidence-min-qual Q] [--evidence-min-mapq Q] [--evidence-min-enddist N] (the variant table's rows with the
mean base quality, mapping quality and distance to the read's end of the reference's and the allele's tokens, and EVIDENCE = PASS or
LOWQ, LOWMQ, END; counted likewise; needs --variant-table; not with --batch, --index-override or -i --gpus N), and

    python -m trueconsense_amd.TrueConsense --batch MANIFEST -ref r.fa -gff r.gff -cov 30 [-noambig] [-t N]

for many samples against one reference in one process: MANIFEST holds one sample per line, tab-separated:
input BAM, sample name, consensus FASTA and — optional, "-" or empty for "not wanted" — VCF, corrected GFF, coverage TSV
(the -i / -name / -o / -vcf / -ogff / -doc of the single-sample form).  The samples go through the native file runner
(csrc/pipeline.cpp): reading, GPU work and the host walk of consecutive samples overlap, all four outputs are written natively.
"""
from __future__ import annotations

import argparse
import json
import multiprocessing
import os
import pathlib
import sys
import time

from . import _state
from .Coverage import BuildCoverage
from .func import MyHelpFormatter, color
from .indexing import Gffindex, Override_index_positions, build_counts, read_override_index
from .Outputs import WriteOutputs
from .version import __version__


def _file_arg(parser, suffixes, what, missing_exit, multi_suffix=False):
    """argparse `type=` callable: the path must exist (else print + exit with the reference's code,
    TrueConsense.py:26-73) and carry one of `suffixes` (else parser.error, exit code 2)."""
    def check(fname):
        if not os.path.isfile(fname):
            print(f'"{fname}" is not a file. Exiting...')
            sys.exit(missing_exit)
        p = pathlib.Path(fname)
        ext = "".join(p.suffixes) if multi_suffix else p.suffix
        ok = all(sfx in ext for sfx in suffixes) if multi_suffix else ext in suffixes
        if not ok:
            parser.error(f"{what[0]} {color.YELLOW}({fname}){color.END} doesn't seem to be {what[1]}.")
        return fname
    return check


def _range_arg(parser, flag, hi):
    """argparse `type=` callable: an integer in 0..hi, decimal or 0x... (else parser.error, exit code 2)."""
    def check(text):
        try:
            v = int(text, 0)
        except ValueError:
            try:
                v = int(text, 10)
            except ValueError:
                v = -1
        if not 0 <= v <= hi:
            parser.error(f"{flag} takes an integer from 0 to {hi} (decimal or 0x...), not {color.YELLOW}{text}{color.END}.")
        return v
    return check


def _min_af_arg(parser, flag="--min-af"):
    """argparse `type=` callable of --min-af (and --strand-ratio): text -> fractions.Fraction, exact ("0.03", "3e-2" and "3/100" are one value); refused
    (parser.error, exit code 2) unless 0 <= F <= 1 with a reduced denominator of at most 10^6."""
    def check(text):
        from fractions import Fraction
        from .engine import min_af_fraction
        try:
            return Fraction(*min_af_fraction(text.strip()))
        except ValueError as e:
            parser.error(f"{flag} takes a frequency from 0 to 1 (a decimal or a fraction n/d, d up to 1000000): {color.YELLOW}{e}{color.END}.")
    return check


def _link_ratio_arg(parser):
    """argparse `type=` callable of --link-ratio: parsed as --min-af is, then refused (parser.error, exit code 2) unless 1/2 < F <= 1."""
    inner = _min_af_arg(parser, "--link-ratio")

    def check(text):
        f = inner(text)
        if not 2 * f > 1:
            parser.error(f"--link-ratio takes a ratio above 1/2 and up to 1, not {color.YELLOW}{text}{color.END}.")
        return f
    return check


def _neighbours_arg(parser):
    """argparse `type=` callable of --link-neighbours: an integer in 1..7 (else parser.error, exit code 2)."""
    def check(text):
        try:
            v = int(text, 10)
        except ValueError:
            v = 0
        if not 1 <= v <= 7:
            parser.error(f"--link-neighbours takes an integer from 1 to 7, not {color.YELLOW}{text}{color.END}.")
        return v
    return check


def _count_arg(parser, flag, lo):
    """argparse `type=` callable: an integer in lo..2^31-1 (else parser.error, exit code 2)."""
    def check(text):
        try:
            v = int(text, 10)
        except ValueError:
            v = lo - 1
        if not lo <= v <= 2 ** 31 - 1:
            parser.error(f"{flag} takes an integer from {lo} to {2 ** 31 - 1}, not {color.YELLOW}{text}{color.END}.")
        return v
    return check


def variants_of(a):
    """The parsed namespace's table thresholds as keyword arguments of Context.variants / set_variants."""
    return dict(min_af=a.min_af, min_alt_depth=a.min_alt_depth, min_depth=a.variant_min_depth)


def write_variant_table(path, parts):
    """--variant-table: the header line, then for every (records, region, reference on the records' axis, pos_offset) its rows."""
    from .engine import VARIANTS_HEADER, variants_text
    text = VARIANTS_HEADER + "".join(variants_text(recs, region, ref, off) for recs, region, ref, off in parts)
    with open(path, "w") as out:
        out.write(text)


def strand_of(a):
    """The parsed namespace's --variant-strand thresholds as keyword arguments of engine.variants_strand_text, or None without the flag."""
    if not getattr(a, "variant_strand", False):
        return None
    return dict(min_strand_depth=int(a.strand_min_depth), strand_ratio=a.strand_ratio)


def write_variant_strand_table(path, parts, rule):
    """--variant-table under --variant-strand: the longer header line, then for every (records, their strand counts, region, reference
    on the records' axis, pos_offset) its rows.  Nothing is written when a part's counts do not add up to its records (TcmiError).
    -> (rows with STRAND = BIAS, rows with LOW)."""
    from .engine import VARIANTS_STRAND_HEADER, variants_strand_text
    text = "".join(variants_strand_text(recs, strand, region, ref, off, **rule) for recs, strand, region, ref, off in parts)
    with open(path, "w") as out:
        out.write(VARIANTS_STRAND_HEADER + text)
    return text.count("\tBIAS\n"), text.count("\tLOW\n")


def links_of(a):
    """The parsed namespace's --variant-links settings as (file, neighbours, keyword arguments of engine.variants_links_text), or None
    without the flag."""
    if getattr(a, "variant_links", None) is None:
        return None
    return a.variant_links, int(a.link_neighbours), dict(min_depth=int(a.link_min_depth), ratio=a.link_ratio)


def write_variant_links(path, parts, links):
    """--variant-links: the header line, then for every (records, their link counts, region, reference on the records' axis,
    pos_offset) one row per pair of its records at most `neighbours` distinct positions apart.  Pairs across parts never appear.
    Nothing is written when a part's counts do not add up to its records (TcmiError).  -> {"variant_link_rows": n,
    "variant_links_cis": .., "_trans", "_mixed", "_none", "_low"}."""
    from .engine import VARIANTS_LINKS_HEADER, variants_links_text
    _, k, rule = links
    text = "".join(variants_links_text(recs, lk, k, region, ref, off, **rule) for recs, lk, region, ref, off in parts)
    with open(path, "w") as out:
        out.write(VARIANTS_LINKS_HEADER + text)
    return link_stats(text)


def link_stats(text=""):
    """the --stats counters of --variant-links' rows (no rows: zeros)"""
    from .engine import LINK_PHASES
    out = {"variant_link_rows": text.count("\n")}
    out.update({"variant_links_" + w.lower(): text.count("\t%s\n" % w) for w in LINK_PHASES})
    return out


def evidence_of(a):
    """The parsed namespace's --variant-evidence settings as (file, keyword arguments of engine.variants_evidence_text), or None without
    the flag."""
    if getattr(a, "variant_evidence", None) is None:
        return None
    return a.variant_evidence, dict(min_qual=int(a.evidence_min_qual), min_mapq=int(a.evidence_min_mapq), min_enddist=int(a.evidence_min_enddist))


def evidence_stats(text=""):
    """the --stats counters of --variant-evidence's rows (no rows: zeros)"""
    from .engine import EVIDENCE_NAMES
    words = [ln.rsplit("\t", 1)[-1].split(",") for ln in text.splitlines()]
    return {"variant_evidence_" + w.lower(): sum(w in row for row in words) for w in EVIDENCE_NAMES}


def write_variant_evidence(path, parts, rule):
    """--variant-evidence: the header line, then for every (records, their evidence counts, region, reference on the records' axis,
    pos_offset) its rows.  Nothing is written when a part's counts do not add up to its records (TcmiError).  -> {"variant_evidence_lowq":
    rows whose EVIDENCE names LOWQ, "_lowmq", "_end"}."""
    from .engine import VARIANTS_EVIDENCE_HEADER, variants_evidence_text
    text = "".join(variants_evidence_text(recs, ev, region, ref, off, **rule) for recs, ev, region, ref, off in parts)
    with open(path, "w") as out:
        out.write(VARIANTS_EVIDENCE_HEADER + text)
    return evidence_stats(text)


class StreamCounts:
    """What the command line counts behind the step, in the record stream the device decoder leaves resident: --amplicon-reads,
    --variant-strand and --variant-links of the parsed namespace (layout: amplicon_reads_of's).  False when none is asked for.  A
    further count of this kind is one more line in each method here, and one _sum_to_root call in distributed.consensus_split_bamfile."""
    KEYS = ("amplicon_reads", "variant_strand", "variant_links")    # count's keys; the order of consensus_split_bamfile's extra parts
    # (--indel-table's "indel_events" is no such part: its lists have no fixed length, and -i --gpus N is refused with it)
    indels = None                                                   # --indel-table's file
    # (nor is --variant-evidence's "variant_evidence": its sums would reduce like the strand counts, but the split's keywords are fixed)
    evidence = None                                                 # --variant-evidence's (file, thresholds)

    def __init__(self, a, layout=None):
        self.areads, self.srule, self.links = amplicon_reads_of(a, layout), strand_of(a), links_of(a)
        self.indels = getattr(a, "indel_table", None)
        self.evidence = evidence_of(a)
        self.lists_records = bool(self.srule or self.links or self.indels or self.evidence)     # must the step list the variant table's records?
        self.variants = variants_of(a) if self.lists_records else None
        # the flag named when the file leaves the device path (indexing.device_readset's `need`)
        self.need = "--variant-strand" if self.srule else "--variant-links" if self.links else "--indel-table" if self.indels else \
            "--variant-evidence" if self.evidence else "--amplicon-reads" if self.areads else None

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
        """the --stats keys of --amplicon-reads (write_variant_tables returns those of the other two)"""
        r = got["amplicon_reads"]["reads"] if got and "amplicon_reads" in got else (0, 0)
        return {"amplicon_reads_ambiguous": int(r[-2]), "amplicon_reads_unassigned": int(r[-1])}


def write_variant_tables(a, parts, want):
    """--variant-table — with the strand columns under --variant-strand — and then --variant-links: parts = [(records, their strand
    counts or None, their link counts or None, region, reference on the records' axis, pos_offset)], want = StreamCounts(a).  -> their
    --stats keys (zeros for what was not asked for; no --variant-table: nothing written, all zeros)."""
    stats = dict(variant_records=0, variant_strand_bias=0, variant_strand_low=0, **link_stats())
    if a.variant_table is None:
        return stats
    stats["variant_records"] = sum(len(p[0]) for p in parts)
    if want.srule:                                  # (the writer refuses counts that do not add up to the records)
        stats["variant_strand_bias"], stats["variant_strand_low"] = write_variant_strand_table(a.variant_table, [p[:2] + p[3:] for p in parts], want.srule)
    else:
        write_variant_table(a.variant_table, [p[:1] + p[3:] for p in parts])
    if want.links:                                  # (its writer refuses likewise)
        stats.update(write_variant_links(want.links[0], [p[:1] + p[2:] for p in parts], want.links))
    return stats


def write_indel_table(path, parts):
    """--indel-table: the header line, then for every (records, their (events, text, totals), region, reference on the records' axis,
    pos_offset) one row per reported insertion or deletion.  Nothing is written when a part's insertions do not add up to its '+' rows
    (TcmiError)."""
    from .engine import INDELS_HEADER, indels_text
    text = "".join(indels_text(*found, recs, region, ref, off) for recs, found, region, ref, off in parts)
    with open(path, "w") as out:
        out.write(INDELS_HEADER + text)


def _names_a_table(line):
    """does this manifest line's 7th column name a variant table ("-" or empty: none)?"""
    f = line.rstrip("\n").split("\t")
    return len(f) > 6 and f[6] not in ("", "-")


def read_manifest(a):
    """--batch: the manifest's samples as [BAM, name, FASTA, VCF, GFF, TSV, variant table] (None: not wanted).  A malformed line, a
    missing BAM, or table thresholds without any 7th column print why and exit, as the flags' own checks do."""
    rows = []
    with open(a.batch) as fh:
        for ln, line in enumerate(fh, 1):
            line = line.rstrip("\n")
            if not line or line.startswith("#"):
                continue
            f = line.split("\t")
            if len(f) < 3:
                print(f'{a.batch}:{ln}: need at least "BAM<TAB>name<TAB>FASTA". Exiting...')
                sys.exit(1)
            f += [""] * (7 - len(f))
            if not os.path.isfile(f[0]):
                print(f'"{f[0]}" is not a file. Exiting...')
                sys.exit(-1)
            rows.append([f[0], f[1], f[2]] + [None if x in ("", "-") else x for x in f[3:7]])
    if a.variant_thresholds_given and not any(r[6] for r in rows):
        print("--min-af / --min-alt-depth / --variant-min-depth need a variant table: no line of the manifest has a 7th column. Exiting...")
        sys.exit(1)
    return rows


def _scheme_amplicons(a, layout, flag, region):
    """--amplicon-scheme's amplicons for `flag` (--amplicon-table, --amplicon-reads) -> [(Amplicon, the shift of its contig's slot,
    (fs, le, rs, fe) in the contig's own coordinates)].  Without a layout the amplicons on the BAM's reference name (--batch: the one
    -ref names), shift 0; layout = (the BAM header's reference names, shift): those on contigs the layout holds.  None left, or a
    scheme that does not parse: an argument error (exit 1)."""
    from .io import primers as pb
    try:
        rows = pb.read_scheme(a.amplicon_scheme)
        amps = pb.amplicons(rows, region)
        zones = dict(zip(((m.chrom, m.name) for m in amps), pb.amplicon_zones(rows)))
    except (OSError, pb.PrimerBedError) as e:
        print(f"--amplicon-scheme: {e}. Exiting...")
        sys.exit(1)
    if layout is not None:
        out = pb.amplicons_for_layout(amps, *layout)
        where = "a contig of the layout"
    else:
        from .contigs import bam_header_refs
        names = bam_header_refs(a.input)[0] if getattr(a, "input", None) else []
        if not names:
            from .io import fasta
            names = [fasta.read_first_record(a.reference)[0]]
        out = [(m, 0) for m in amps if m.chrom == names[0]]
        where = 'the reference "%s"' % names[0]
    if not out:
        print(f"{flag}: no amplicon of {a.amplicon_scheme} is on {where}. Exiting...")
        sys.exit(1)
    if len(out) > 65536:
        print(f"{flag}: {a.amplicon_scheme} has {len(out)} amplicons, more than 65536. Exiting...")
        sys.exit(1)
    return [(m, sh, zones[(m.chrom, m.name)]) for m, sh in out]


def amplicons_of(a, layout=None):
    """The parsed namespace's --amplicon-scheme / --amplicon-region -> [(Amplicon, the shift of its contig's slot on the count matrix's
    axis)], or None without --amplicon-table.  Without a layout the amplicons on the BAM's reference name (--batch: the one -ref
    names), shift 0; layout = (the BAM header's reference names, shift): those on contigs the layout holds.  None left, or a scheme
    that does not parse: an argument error (exit 1)."""
    if not getattr(a, "amplicon_table", None):
        return None
    return [(m, sh) for m, sh, _ in _scheme_amplicons(a, layout, "--amplicon-table", a.amplicon_region)]


def amplicon_reads_of(a, layout=None):
    """The parsed namespace's --amplicon-reads -> ([Amplicon] in amplicons_of's order, [(fs, le, rs, fe)] on the count matrix's axis as
    Context.amplicon_reads takes them, slack), or None without the flag.  The amplicons are chosen as amplicons_of chooses them."""
    if not getattr(a, "amplicon_reads", None):
        return None
    got = _scheme_amplicons(a, layout, "--amplicon-reads", "full")
    return [m for m, _, _ in got], [tuple(v + sh for v in z) for _, sh, z in got], int(a.amplicon_reads_slack)


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
    from .engine import AMPLICON_READS_HEADER
    with open(path, "w") as out:
        out.write(AMPLICON_READS_HEADER + amplicon_reads_text(sample, counts, amps))


def amplicon_intervals(amps):
    """amplicons_of's list -> [(start, end)] on the count matrix's axis, as Context.set_intervals / interval_stats take them."""
    return [(m.start + sh, m.end + sh) for m, sh in amps]


def amplicon_rows(records, sample, amps):
    """One sample's rows of the amplicon table: records[i] belongs to amps[i]; REGION is the amplicon's contig and the positions are
    the contig's own (tcmi_amplicons_text, one call per contig)."""
    from itertools import groupby
    from .engine import amplicons_text
    text, i = [], 0
    for (chrom, sh), grp in groupby(amps, key=lambda x: (x[0].chrom, x[1])):
        grp = list(grp)
        text.append(amplicons_text(records[i:i + len(grp)], sample, chrom, [m.name for m, _ in grp], [m.pool for m, _ in grp],
                                   [m.start + sh for m, _ in grp], sh))
        i += len(grp)
    return "".join(text)


def write_amplicon_table(path, samples, amps):
    """--amplicon-table: the header line, then for every (sample name, its records) the sample's rows."""
    from .engine import AMPLICONS_HEADER
    text = AMPLICONS_HEADER + "".join(amplicon_rows(recs, name, amps) for name, recs in samples)
    with open(path, "w") as out:
        out.write(text)


def join_amplicon_parts(path, parts, n_samples, per_sample):
    """--batch --gpus N: part k (a child's table) holds the rows of samples k, k + N, ... — `per_sample` lines each; -> FILE with
    every sample's rows in manifest order, and the parts removed."""
    from .engine import AMPLICONS_HEADER
    rows = []
    for part in parts:
        with open(part) as fh:
            lines = fh.read().split("\n")[1:]
        rows.append(lines)
    n = len(parts)
    with open(path, "w") as out:
        out.write(AMPLICONS_HEADER)
        for i in range(n_samples):
            k, j = i % n, i // n
            for line in rows[k][j * per_sample:(j + 1) * per_sample]:
                out.write(line + "\n")
    for part in parts:
        os.remove(part)


def read_filter_of(a):
    """The parsed namespace's read filter -> (min_mapq, require_flags, exclude_flags), or None when none was asked for."""
    f = (a.min_mapq, a.require_flags, a.exclude_flags)
    return f if any(f) else None


def primers_of(a, layout=None):
    """The parsed namespace's --primers / --primer-slack -> (rows on the count matrix's axis, slack) as Context.set_primers takes
    them, or None when no BED was given.  Without a layout the rows whose chrom is the BAM's reference name are used (none: an argument
    error); layout = (the BAM header's reference names, shift): every row shifted by its contig's slot, rows naming no contig ignored."""
    if not getattr(a, "primers", None):
        return None
    from .io import primers as pb
    try:
        bed = pb.read_bed(a.primers)
    except (OSError, pb.PrimerBedError) as e:
        print(f"--primers: {e}. Exiting...")
        sys.exit(1)
    if layout is not None:
        return pb.rows_for_layout(bed, *layout), int(a.primer_slack)
    from .contigs import bam_header_refs
    names = bam_header_refs(a.input)[0] if getattr(a, "input", None) else []
    if not names:                                   # (--batch: every sample on the reference the FASTA names)
        from .io import fasta
        names = [fasta.read_first_record(a.reference)[0]]
    rows = pb.rows_for_reference(bed, names[0])
    if not rows:
        print(f'--primers: no row of {a.primers} is on the reference "{names[0]}". Exiting...')
        sys.exit(1)
    return rows, int(a.primer_slack)


def rules_of(a, layout=None):
    """The parsed namespace's read rules -> engine.ReadRules (layout: primers_of's)."""
    from .engine import ReadRules
    return ReadRules(read_filter_of(a), a.min_baseq, primers_of(a, layout), a.mate_overlap, getattr(a, "dedup", False))


def GetArgs(givenargs):
    """Same flags, defaults, required-ness and exit codes as TrueConsense.py:25-209; table-driven."""
    parser = argparse.ArgumentParser(
        prog="TrueConsense", usage="%(prog)s [required options] [optional arguments]",
        description="TrueConsense: Creating biologically valid consensus sequences from reference-based alignments",
        formatter_class=MyHelpFormatter, add_help=False)
    bam_t = _file_arg(parser, (".bam",), ("Input file", "a BAM-file"), -1)
    fasta_t = _file_arg(parser, (".fasta", ".fa"), ("Reference file", "a Fasta-file"), 1)
    gff_t = _file_arg(parser, (".gff",), ("Given file", "a GFF file"), 1)
    csvgz_t = _file_arg(parser, (".csv", ".gz"), ("Given file", "a compressed csv file"), 1, multi_suffix=True)
    threads = min(multiprocessing.cpu_count(), 128)
    #          flags                          keyword arguments
    required = [
        (("--input", "-i"), dict(type=bam_t, metavar="File", help="alignment to call the consensus from (BAM)")),
        (("--output", "-o"), dict(type=str, default=os.getcwd() + "consensus.fasta", metavar="File",
                                  help="where the consensus FASTA goes")),
        (("--reference", "-ref"), dict(type=fasta_t, metavar="File", help="reference sequence (FASTA)")),
        (("--features", "-gff"), dict(type=gff_t, metavar="File", help="genome features of the reference (GFF)")),
        (("--coverage-level", "-cov"), dict(type=int, default=30, metavar="100",
                                            help="minimum coverage for a position to be called")),
        (("--samplename", "-name"), dict(metavar="Text", help="sample name, used in the FASTA header")),
    ]
    optional = [
        (("--variants", "-vcf"), dict(type=str, metavar="File", help="also write a VCF")),
        (("--depth-of-coverage", "-doc"), dict(type=str, metavar="File", help="also write position<TAB>coverage (TSV)")),
        (("--output-gff", "-ogff"), dict(type=str, metavar="File", help="also write the corrected GFF")),
        (("--threads", "-t"), dict(default=threads, metavar="N", type=int, help="host threads (BAM decoding, packing)")),
        (("--noambiguity", "-noambig"), dict(action="store_true", help="no IUPAC ambiguity codes in the consensus")),
        (("--index-override",), dict(type=csvgz_t, metavar="File",
                                     help="gzipped CSV (position,coverage,A,T,C,G,X,I) whose rows replace the tallied\n"
                                          "counts at those positions; use with caution")),
        (("--version", "-v"), dict(action="version", version=__version__, help="print the version and exit")),
        (("--help", "-h"), dict(action="help", default=argparse.SUPPRESS, help="print this help and exit")),
    ]
    additive = [
        (("--device",), dict(type=int, default=None, metavar="N", help="GPU ordinal (default: 0)")),
        (("--stats",), dict(type=str, default=None, metavar="File", help="write stage timings as JSON")),
    ]
    additive.append((("--batch",), dict(type=str, default=None, metavar="File",
                                        help="many samples: a tab-separated manifest (BAM, name, FASTA[, VCF, GFF, TSV] per line)\n"
                                             "instead of -i / -name / -o / -vcf / -ogff / -doc")))
    additive.append((("--gpus",), dict(type=int, default=1, metavar="N",
                                       help="GPUs of this node to use: with --batch the manifest's samples are dealt to N processes,\n"
                                            "one per GPU (independent files, no exchange); with -i ONE BAM file is shared — every GPU\n"
                                            "takes a range of its BGZF blocks, one reduce of the count matrix")))
    additive.append((("--per-contig",), dict(action="store_true",
                                             help="one consensus per record of -ref (a multi-record reference, e.g. a segmented virus):\n"
                                                  "records named {name}_{record}, all in -o; -vcf / -ogff / -doc cover every record")))
    additive.append((("--min-mapq",), dict(type=_range_arg(parser, "--min-mapq", 255), default=0, metavar="N",
                                           help="ignore alignment records with MAPQ below N (samtools view -q)")))
    additive.append((("--require-flags",), dict(type=_range_arg(parser, "--require-flags", 0xFFFF), default=0, metavar="F",
                                                help="ignore records that lack any of these FLAG bits (samtools view -f; decimal or 0x...)")))
    additive.append((("--exclude-flags",), dict(type=_range_arg(parser, "--exclude-flags", 0xFFFF), default=0, metavar="F",
                                                help="ignore records with any of these FLAG bits, e.g. 0x400 duplicates, 0x900 secondary\n"
                                                     "and supplementary (samtools view -F; decimal or 0x...)")))
    additive.append((("--min-baseq",), dict(type=_range_arg(parser, "--min-baseq", 255), default=0, metavar="N",
                                            help="skip pileup tokens (a read on a column) whose base quality is below N in the count matrix\n"
                                                 "(samtools mpileup -Q; qualities as the file stores them); needs the device decoder")))
    additive.append((("--mate-overlap",), dict(action="store_true",
                                               help="count the columns that the two mates of a read pair share once in the count matrix: the\n"
                                                    "mate that starts further right loses them (samtools mpileup's default; by position, qualities\n"
                                                    "are not summed), joined by read name on the device; needs the device decoder; not with\n"
                                                    "-i --gpus N")))
    additive.append((("--dedup",), dict(action="store_true",
                                        help="ignore duplicate templates in the count matrix (samtools markdup, Picard MarkDuplicates): of the\n"
                                             "fragments with one unclipped 5' end and strand, and of the proper pairs with the same two, the one\n"
                                             "with the highest sum of base qualities >= 15 is kept, found on the device; nothing is written back;\n"
                                             "needs the device decoder; not with -i --gpus N, not with --amplicon-reads")))
    additive.append((("--primers",), dict(type=str, default=None, metavar="File",
                                          help="BED of the amplicon scheme's primers (chrom, start, end, name, pool, strand): a read's tokens\n"
                                               "inside the primer at its head ('+') or tail ('-') stay out of the count matrix\n"
                                               "(ivar trim, samtools ampliconclip); needs the device decoder")))
    additive.append((("--primer-slack",), dict(type=_range_arg(parser, "--primer-slack", 1000), default=0, metavar="N",
                                               help="a read may start up to N columns in front of a primer (end behind it) and still be masked")))
    additive.append((("--variant-table",), dict(type=str, default=None, metavar="File",
                                                help="also write per position every non-reference allele (A, T, C, G, * deletion, + insertion\n"
                                                     "mark) at or above --min-af, tab-separated: REGION POS REF ALT ALT_DP TOTAL_DP ALT_FREQ\n"
                                                     "(ivar variants), from the count matrix the consensus is called from")))
    additive.append((("--min-af",), dict(type=_min_af_arg(parser), default=None, metavar="F",
                                         help="minimum allele frequency of the variant table, 0..1, a decimal or n/d (default 0.03)")))
    additive.append((("--min-alt-depth",), dict(type=_count_arg(parser, "--min-alt-depth", 1), default=None, metavar="N",
                                                help="minimum reads with the allele (default 1)")))
    additive.append((("--variant-min-depth",), dict(type=_count_arg(parser, "--variant-min-depth", 0), default=None, metavar="N",
                                                    help="minimum coverage of a position of the variant table (ivar variants -m; default 10;\n"
                                                         "independent of -cov)")))
    additive.append((("--variant-strand",), dict(action="store_true",
                                                 help="the variant table's rows also say how the allele's reads split by strand (FLAG 0x10):\n"
                                                      "REF_FWD REF_REV ALT_FWD ALT_REV TOTAL_FWD TOTAL_REV and STRAND = PASS, BIAS or LOW, counted\n"
                                                      "in the records the device decoded; needs --variant-table and the device decoder; not with\n"
                                                      "--batch or --index-override")))
    additive.append((("--strand-min-depth",), dict(type=_count_arg(parser, "--strand-min-depth", 1), default=None, metavar="N",
                                                   help="STRAND is LOW when either strand covers the position with fewer than N reads (default 10)")))
    additive.append((("--strand-ratio",), dict(type=_min_af_arg(parser, "--strand-ratio"), default=None, metavar="F",
                                               help="STRAND is BIAS when the allele's frequency on one strand is below F times its frequency on\n"
                                                    "the other, 0..1, a decimal or n/d (default 1/10)")))
    additive.append((("--variant-links",), dict(type=str, default=None, metavar="File",
                                                help="also write, for every two rows of the variant table at most K distinct positions apart, how\n"
                                                     "many alignment records carry both alleles, one of them or neither: REGION POS_A REF_A ALT_A\n"
                                                     "POS_B REF_B ALT_B SPAN BOTH ONLY_A ONLY_B NEITHER PHASE (CIS, TRANS, MIXED, NONE or LOW),\n"
                                                     "counted in the records the device decoded; needs --variant-table and the device decoder;\n"
                                                     "not with --batch or --index-override; '+' rows are not linked")))
    additive.append((("--link-neighbours",), dict(type=_neighbours_arg(parser), default=None, metavar="K",
                                                  help="link a row's position with the next K distinct positions of the table, 1..7 (default 2)")))
    additive.append((("--link-min-depth",), dict(type=_count_arg(parser, "--link-min-depth", 1), default=None, metavar="N",
                                                 help="PHASE is LOW when fewer than N records have a token at both positions (default 10)")))
    additive.append((("--link-ratio",), dict(type=_link_ratio_arg(parser), default=None, metavar="F",
                                             help="PHASE is CIS when BOTH is at least F of the rarer allele's records among those that span\n"
                                                  "both positions, TRANS when at most 1 - F; above 1/2 up to 1, a decimal or n/d (default 9/10)")))
    additive.append((("--indel-table",), dict(type=str, default=None, metavar="File",
                                              help="also write every insertion and every deletion at the variant table's '+' and '*' positions as\n"
                                                   "one row: REGION POS TYPE (INS / DEL) LEN SEQ COUNT TOTAL_DP FREQ (ivar variants' +ACG / -3),\n"
                                                   "under --min-af / --min-alt-depth / --variant-min-depth, counted in the records the device\n"
                                                   "decoded; needs --variant-table and the device decoder; not with --batch, --index-override\n"
                                                   "or -i --gpus N")))
    additive.append((("--variant-evidence",), dict(type=str, default=None, metavar="File",
                                                   help="also write the variant table's rows with what says whether an allele can be trusted: REF_QUAL\n"
                                                        "ALT_QUAL (mean base quality, ivar variants'), REF_MAPQ ALT_MAPQ (mean mapping quality of the\n"
                                                        "records), REF_ENDDIST ALT_ENDDIST (mean distance to the nearer end of the read's aligned\n"
                                                        "part, capped at 255) and EVIDENCE = PASS or LOWQ, LOWMQ, END, counted in the records the\n"
                                                        "device decoded; needs --variant-table and the device decoder; not with --batch,\n"
                                                        "--index-override or -i --gpus N")))
    additive.append((("--evidence-min-qual",), dict(type=_range_arg(parser, "--evidence-min-qual", 255), default=None, metavar="Q",
                                                    help="EVIDENCE names LOWQ when the allele's mean base quality is below Q; 0: off (default 20)")))
    additive.append((("--evidence-min-mapq",), dict(type=_range_arg(parser, "--evidence-min-mapq", 255), default=None, metavar="Q",
                                                    help="EVIDENCE names LOWMQ when the mean MAPQ of the allele's records is below Q; 0: off (default 20)")))
    additive.append((("--evidence-min-enddist",), dict(type=_range_arg(parser, "--evidence-min-enddist", 255), default=None, metavar="N",
                                                       help="EVIDENCE names END when the allele sits on average fewer than N bases from its reads'\n"
                                                            "nearer end; 0: off (default 5)")))
    additive.append((("--amplicon-table",), dict(type=str, default=None, metavar="File",
                                                 help="also write per amplicon of the scheme the depth of its columns, tab-separated: SAMPLE REGION\n"
                                                      "AMPLICON POOL START END LEN MEAN MEDIAN MIN MIN_POS BELOW (BELOW: columns under -cov), from\n"
                                                      "the count matrix the consensus is called from; --batch: one file, every sample's rows")))
    additive.append((("--amplicon-scheme",), dict(type=str, default=None, metavar="File",
                                                  help="BED of the scheme's primers, named {amplicon}_LEFT / _RIGHT[_alt] (default: the file of --primers)")))
    additive.append((("--amplicon-region",), dict(choices=("insert", "unique", "full"), default=None,
                                                  help="the columns of an amplicon: between its primers (insert, the default), the insert\n"
                                                       "outside every other amplicon (unique), or primers included (full)")))
    additive.append((("--amplicon-reads",), dict(type=str, default=None, metavar="File",
                                                 help="also write per amplicon of the scheme the alignment records that lie inside it and inside no\n"
                                                      "other, tab-separated: SAMPLE REGION AMPLICON POOL READS FULL_LENGTH (FULL_LENGTH: those that start\n"
                                                      "in its left primer and end in its right one), then the records inside several amplicons\n"
                                                      "(*ambiguous) and inside none (*unassigned); needs the device decoder; not with --batch")))
    additive.append((("--amplicon-reads-slack",), dict(type=_range_arg(parser, "--amplicon-reads-slack", 1000), default=None, metavar="N",
                                                       help="a read may reach up to N columns beyond an amplicon's outer primer ends and still lie\n"
                                                            "inside it (default 5)")))
    # (is this the --batch form?  asked of a small parser of its own: "--batch=FILE" and argparse's abbreviations count too)
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--batch", default=None)
    batch = pre.parse_known_args(givenargs)[0].batch is not None
    for title, rows, req in (("Required arguments", required, True), ("Optional arguments", optional, False),
                             ("MI355X arguments (additive)", additive, False)):
        group = parser.add_argument_group(title)
        for flags, kw in rows:
            if req:
                kw["required"] = not (batch and flags[0] in ("--input", "--output", "--samplename"))
            group.add_argument(*flags, **kw)
    a = parser.parse_args(givenargs)
    from fractions import Fraction
    a.variant_thresholds_given = any(v is not None for v in (a.min_af, a.min_alt_depth, a.variant_min_depth))
    # the flags that count behind the step, with their dependant options: their refusals exit 1 with one line, nothing written
    for flag, on, deps in (("--variant-strand", a.variant_strand, ("strand_min_depth", "strand_ratio")),
                           ("--variant-links", a.variant_links is not None, ("link_neighbours", "link_min_depth", "link_ratio")),
                           ("--indel-table", a.indel_table is not None, ()),
                           ("--variant-evidence", a.variant_evidence is not None, ("evidence_min_qual", "evidence_min_mapq", "evidence_min_enddist"))):
        names = " / ".join("--" + d.replace("_", "-") for d in deps)
        for bad, why in ((not on and any(getattr(a, d) is not None for d in deps), f"{names} need {flag}."),
                         (on and a.batch is not None, f"{flag} goes with a single sample (-i): --batch is refused, its file runner has no hook behind its steps."),
                         (on and a.batch is None and a.variant_table is None, f"{flag} needs --variant-table."),
                         (on and a.index_override is not None, f"{flag} does not go with --index-override: the overridden matrix no longer equals the reads."),
                         (on and flag == "--indel-table" and a.batch is None and a.gpus and a.gpus > 1,
                          f"{flag} does not go with -i --gpus N: the ranks' event lists would have to be merged on rank 0, which is not built."),
                         (on and flag == "--variant-evidence" and a.batch is None and a.gpus and a.gpus > 1,
                          f"{flag} does not go with -i --gpus N: the ranks' sums would have to be added up on rank 0, which is not built.")):
            if bad:
                print(f"{why} Exiting...")
                sys.exit(1)
    if a.mate_overlap and a.batch is None and a.gpus and a.gpus > 1:
        parser.error("--mate-overlap does not go with -i --gpus N: a record's mate may lie in another rank's block range.")
    if a.dedup and a.batch is None and a.gpus and a.gpus > 1:
        parser.error("--dedup does not go with -i --gpus N: a template's other records may lie in another rank's block range.")
    if a.dedup and a.amplicon_reads is not None:
        parser.error("--dedup does not go with --amplicon-reads: that count asks only which records are kept and would count the duplicates.")
    if a.batch is not None and a.variant_table is not None:
        parser.error("--variant-table goes with a single sample (-i); with --batch the manifest's 7th column names each sample's table.")
    if a.batch is None and a.variant_table is None and a.variant_thresholds_given:
        parser.error("--min-af / --min-alt-depth / --variant-min-depth need --variant-table.")
    if a.amplicon_table is None and (a.amplicon_region is not None or (a.amplicon_scheme is not None and a.amplicon_reads is None)):
        parser.error("--amplicon-scheme / --amplicon-region need --amplicon-table.")
    if a.amplicon_reads is None and a.amplicon_reads_slack is not None:
        parser.error("--amplicon-reads-slack needs --amplicon-reads.")
    if a.amplicon_reads is not None:
        if a.batch is not None:
            parser.error("--amplicon-reads goes with a single sample (-i): --batch is refused, its file runner keeps the read sets inside its native threads.")
        if a.amplicon_scheme is None and not a.primers:
            parser.error("--amplicon-reads needs the scheme's BED: --amplicon-scheme, or --primers.")
    if a.amplicon_table is not None:
        if a.amplicon_scheme is None and not a.primers:
            parser.error("--amplicon-table needs the scheme's BED: --amplicon-scheme, or --primers.")
        if a.coverage_level < 0:
            parser.error("--amplicon-table counts the columns below -cov, which cannot be negative.")
    if a.amplicon_table is not None or a.amplicon_reads is not None:
        a.amplicon_scheme = a.primers if a.amplicon_scheme is None else a.amplicon_scheme
    for key, default in dict(strand_min_depth=10, strand_ratio=Fraction(1, 10), link_neighbours=2, link_min_depth=10, link_ratio=Fraction(9, 10),
                             amplicon_reads_slack=5, amplicon_region="insert", evidence_min_qual=20, evidence_min_mapq=20, evidence_min_enddist=5, min_af=Fraction(3, 100), min_alt_depth=1, variant_min_depth=10).items():
        if getattr(a, key) is None:                 # (None until here: the checks above ask whether the option was given)
            setattr(a, key, default)
    return a


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


def _spawn(cmds, envs):
    """Start the children BEFORE this process touches a GPU (never re-exec a process that did), wait for all, -> worst exit code.
    The children are polled together: once one of them has failed the others get a short grace (they may be waiting for it in a
    collective) and are then terminated, so nobody sits out a collective's time-out."""
    import subprocess
    procs = [subprocess.Popen(c, env=e) for c, e in zip(cmds, envs)]
    rcs = [None] * len(procs)
    failed_at = None
    while any(r is None for r in rcs):
        for i, p in enumerate(procs):
            if rcs[i] is None:
                rcs[i] = p.poll()
                if rcs[i] not in (None, 0) and failed_at is None:
                    failed_at = time.monotonic()
        if failed_at is not None and time.monotonic() - failed_at > float(os.environ.get("TCMI_SPAWN_GRACE", "20")):
            for i, p in enumerate(procs):
                if rcs[i] is None:
                    p.terminate()
            for i, p in enumerate(procs):
                if rcs[i] is None:
                    try:
                        rcs[i] = p.wait(timeout=10)
                    except subprocess.TimeoutExpired:
                        p.kill()
                        rcs[i] = p.wait()
            break
        time.sleep(0.02)
    return max((abs(r) for r in rcs), default=0)


def _child_argv(a, single, tables=True):
    """The command line of a --gpus child, built from the PARSED namespace (argparse takes abbreviations, so the spelling the user typed
    cannot be filtered by name): the reference's flags as they were understood, never --gpus / --batch / --device / --stats — the
    caller adds its own — plus an explicit `--gpus 1`, so that a child can never deal itself out again.  tables: the child writes a
    variant table (a --batch shard with a 7th column somewhere); one that writes none gets no thresholds, which alone are an error."""
    out = ["-ref", a.reference, "-gff", a.features, "-cov", str(a.coverage_level), "-t", str(a.threads)]
    if a.noambiguity:
        out.append("-noambig")
    if a.min_mapq:                                  # (the read filter, only where one was asked for)
        out += ["--min-mapq", str(a.min_mapq)]
    for flag, v in (("--require-flags", a.require_flags), ("--exclude-flags", a.exclude_flags)):
        if v:
            out += [flag, "0x%x" % v]
    if a.min_baseq:                                 # (the base-quality floor, likewise)
        out += ["--min-baseq", str(a.min_baseq)]
    if a.mate_overlap:                              # (the mate-overlap rule, likewise: a --batch child's file runner takes it)
        out += ["--mate-overlap"]
    if a.dedup:                                     # (the duplicate rule, likewise)
        out += ["--dedup"]
    if a.primers:                                   # (the primer mask, likewise: both flags or neither)
        out += ["--primers", a.primers, "--primer-slack", str(a.primer_slack)]
    if tables and (a.variant_thresholds_given or a.variant_table):     # (the table's thresholds, likewise; --batch children find their tables in the manifest)
        out += ["--min-af", str(a.min_af), "--min-alt-depth", str(a.min_alt_depth), "--variant-min-depth", str(a.variant_min_depth)]
    if a.amplicon_table:                            # (the amplicon table's scheme; its FILE is the caller's: a --batch child writes a part)
        out += ["--amplicon-scheme", a.amplicon_scheme, "--amplicon-region", a.amplicon_region]
    elif single and a.amplicon_reads:               # (--amplicon-reads alone: the scheme, no region)
        out += ["--amplicon-scheme", a.amplicon_scheme]
    if single:
        if a.amplicon_reads:
            out += ["--amplicon-reads", a.amplicon_reads, "--amplicon-reads-slack", str(a.amplicon_reads_slack)]
        if a.variant_table:
            out += ["--variant-table", a.variant_table]
        if a.variant_strand:
            out += ["--variant-strand", "--strand-min-depth", str(a.strand_min_depth), "--strand-ratio", str(a.strand_ratio)]
        if a.variant_links:
            out += ["--variant-links", a.variant_links, "--link-neighbours", str(a.link_neighbours), "--link-min-depth", str(a.link_min_depth),
                    "--link-ratio", str(a.link_ratio)]
        if a.amplicon_table:
            out += ["--amplicon-table", a.amplicon_table]
        out += ["-i", a.input, "-o", a.output, "-name", a.samplename]
        for flag, v in (("-vcf", a.variants), ("-doc", a.depth_of_coverage), ("-ogff", a.output_gff)):
            if v is not None:
                out += [flag, v]
    return out + ["--gpus", "1"]


def run_gpus(a):
    """--gpus N: N processes, one per GPU.  --batch: the manifest's samples dealt round-robin (BASELINE configs[3]: independent files,
    no collective); -i: ONE BAM file shared by the GPUs (configs[4]: trueconsense_amd.split_main)."""
    import socket
    import tempfile
    n = int(a.gpus)
    pkg_parent = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base_env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"),
                    PYTHONPATH=os.pathsep.join([pkg_parent] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    one_gpu = os.environ.get("TCMI_SPLIT_ONE_GPU") == "1"              # (rehearsal on a one-GPU box: every child on GPU 0)
    if a.batch:
        rows = [ln for ln in open(a.batch).read().split("\n") if ln.strip() and not ln.startswith("#")]
        # the thresholds without any table: checked once, over the whole manifest, before anything is dealt out (a shard may well name none)
        if a.variant_thresholds_given and not any(_names_a_table(ln) for ln in rows):
            print("--min-af / --min-alt-depth / --variant-min-depth need a variant table: no line of the manifest has a 7th column. Exiting...")
            return 1
        amps = amplicons_of(a)                      # (an unusable scheme ends the run here, before anything is dealt out)
        with tempfile.TemporaryDirectory(prefix="tcmi_gpus_") as tmp:
            cmds, envs, parts = [], [], []
            for k in range(n):
                mine = rows[k::n]
                if not mine:
                    continue
                shard = os.path.join(tmp, "shard%d.tsv" % k)
                with open(shard, "w") as fh:
                    fh.write("\n".join(mine) + "\n")
                cmd = [sys.executable, "-m", "trueconsense_amd.TrueConsense", "--batch", shard, "--device", str(0 if one_gpu else k)] + \
                    _child_argv(a, False, tables=any(_names_a_table(ln) for ln in mine))
                if a.stats:
                    cmd += ["--stats", "%s.gpu%d" % (a.stats, k)]
                if amps:                            # every child a part file of its own beside FILE
                    parts.append("%s.part%d" % (a.amplicon_table, k))
                    cmd += ["--amplicon-table", parts[-1]]
                cmds.append(cmd)
                envs.append(base_env)
            rc = _spawn(cmds, envs)
            if amps and rc == 0:                    # (all children have exited with status 0: the parts are whole)
                join_amplicon_parts(a.amplicon_table, parts, len(rows), len(amps))
            return rc
    if a.index_override:
        print("--index-override goes with one GPU. Exiting...")
        return 1
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmds, envs = [], []
    for k in range(n):
        cmds.append([sys.executable, "-m", "trueconsense_amd.split_main"] + _child_argv(a, True))
        envs.append(dict(base_env, RANK=str(k), LOCAL_RANK=str(k), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port)))
    return _spawn(cmds, envs)


def run_batch(a):
    """--batch: the manifest's samples through the native file runner, four output files each."""
    from datetime import date
    from .engine import FileRunner
    from .io import fasta
    from .Outputs import gff_row_columns, vcf_header
    if a.index_override:
        print("--index-override goes with a single sample (-i), not with --batch. Exiting...")
        sys.exit(1)
    rows = read_manifest(a)
    tables = [r[6] for r in rows] if any(r[6] for r in rows) else None
    IndexGff = Gffindex(a.features)
    gffrows = list(IndexGff.index_dict(seqid="S").values())       # (the runner puts each sample's name there: TrueConsense.py:240)
    refID, refseq = fasta.read_first_record(a.reference)
    rules = rules_of(a)
    amps = amplicons_of(a)
    n_below = 0
    t0 = time.perf_counter()
    cores = max(1, min(int(a.threads), os.cpu_count() or 1))
    runner = FileRunner(int(os.environ.get("TCMI_DEVICE", "0")), gffrows, a.coverage_level, a.noambiguity is False,
                        decoders=min(4, max(1, cores // 4)), decode_threads=max(1, cores // 2), walkers=min(4, max(1, cores // 4)),
                        gpu_streams=(8 if len(rows) > 16 else 3) if len(rows) > 2 else 1, rules=rules,
                        variants=dict(variants_of(a), ref=refseq) if tables else None,
                        intervals=(amplicon_intervals(amps), a.coverage_level) if amps else None)
    runner.set_outputs(refID, refseq, vcf_header(date.today().strftime("%Y%m%d"), sys.argv[1:], a.reference, refID), IndexGff.header.raw_text,
                       [gff_row_columns(r) for r in gffrows])
    try:
        recs = runner.run_files([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows],
                                [r[5] for r in rows], ref_len=len(refseq), table=tables, stats=bool(amps))
        if amps:                                    # one file: every sample's rows in manifest order
            write_amplicon_table(a.amplicon_table, [(r[1], recs[i]) for i, r in enumerate(rows)], amps)
            n_below = int((recs["below"] > 0).sum())
    except Exception:                                                # every failed sample is named; the first one's error (what the reference would raise) goes on up: non-zero exit
        failed = [(rows[i][1], int(c)) for i, c in enumerate(getattr(runner, "last_status", [])) if int(c) != 0]
        for nm, code in failed:
            print(f'sample "{nm}" failed (libtcmi error {code})', file=sys.stderr)
        if failed:
            print(f"{len(failed)} of {len(rows)} samples failed", file=sys.stderr)
        raise
    finally:
        if a.stats:
            with open(a.stats, "w") as fh:
                json.dump({"seconds": {"batch": time.perf_counter() - t0}, "samples": len(rows), "min_baseq": a.min_baseq, "primers": len(rules.primers[0]) if rules.primers else 0,
                           **mate_stats(a.mate_overlap, runner.mate_overlap_totals() if a.mate_overlap else None),
                           **dedup_stats(a.dedup, runner.dedup_totals() if a.dedup else None),
                           "variant_records": int(getattr(runner, "variant_records", 0)),
                           "amplicons": len(amps) if amps else 0, "amplicons_below": n_below, "stage_busy_seconds": runner.seconds,
                           "decoded_on": runner.decoded_on, "status": [int(x) for x in getattr(runner, "last_status", [])]}, fh)
        runner.close()


def run_per_contig(a):
    """--per-contig: trueconsense_amd.contigs; a refused input or a read past its contig's slot exits 1 with nothing written."""
    from . import _ffi
    from .contigs import ContigError, run
    t0 = time.perf_counter()
    try:
        info = run(a)
    except (ContigError, _ffi.TcmiError) as e:
        print(f"{e}. Exiting...", file=sys.stderr)
        sys.exit(1)
    if a.stats:
        with open(a.stats, "w") as fh:
            json.dump(dict({"seconds": {"per_contig": time.perf_counter() - t0}, "min_baseq": a.min_baseq}, **info), fh)


def main(args=None):
    """TrueConsense.py:212-264."""
    if not args:
        args = sys.argv[1:]
    if len(args) < 1:
        print("TrueConsense was called but no arguments were given, please try again.\n"
              "Use 'TrueConsense -h' to see the help document")
        sys.exit(1)
    a = GetArgs(args)
    if a.per_contig:                                # (its refusals come before any GPU work, and before --gpus deals anything out)
        for flag, bad in (("--batch", a.batch), ("--gpus N>1", a.gpus and a.gpus > 1), ("--index-override", a.index_override)):
            if bad:
                print(f"--per-contig does not go with {flag}. Exiting...")
                sys.exit(1)
        from .contigs import ContigError, bam_header_refs, layout_for
        from .io import fasta
        try:
            layout_for(fasta.read_records(a.reference), *bam_header_refs(a.input))
        except ContigError as e:
            print(f"{e}. Exiting...")
            sys.exit(1)
    if a.gpus and a.gpus > 1:
        rc = run_gpus(a)
        if rc:
            sys.exit(rc)
        return
    if a.device is not None:
        os.environ["TCMI_DEVICE"] = str(a.device)
    if a.batch:
        return run_batch(a)
    if a.per_contig:
        return run_per_contig(a)
    t = {"start": time.perf_counter()}

    rules = rules_of(a)
    a.primer_rows = len(rules.primers[0]) if rules.primers else 0
    # (always: the process's one context may have served another call — and for this call only: the flat-array entry points of the
    # same context refuse under a floor, a table or the mate rule)
    with _state.default_context().rules(rules):
        _single_sample(a, rules.read_filter, t)


def _single_sample(a, flt, t):
    """main()'s one-sample flow behind the argument handling (TrueConsense.py:225-264)."""
    from .engine import LazyBam
    bam = LazyBam(a.input, threads=a.threads, read_filter=flt)      # reads reach the host only if an insert candidate needs its tokens
    t["bam_open"] = time.perf_counter()
    want, got = StreamCounts(a), {}
    if want:                                        # counted behind the step, on the read set the step returned, while its stream is resident
        if want.lists_records:                      # (the columns must be known then: the step computes the table's records)
            from .io import fasta
            _state.default_context().set_variants(fasta.read_first_record(a.reference)[1], **want.variants)
        try:
            counts = build_counts(bam, a.reference, on_readset=lambda ctx, rs: got.update(want.count(ctx, rs)), need_device=want.need)
        finally:
            if want.lists_records:
                _state.default_context().set_variants()
        if want.areads:
            write_amplicon_reads(a.amplicon_reads, a.samplename, got["amplicon_reads"], want.areads[0])
    else:
        counts = build_counts(bam, a.reference)     # decoded, packed and tallied on the device
    IndexGff = Gffindex(a.features)
    t["tally"] = time.perf_counter()

    if a.index_override:
        import pandas as pd
        from ._ffi import COLS
        df = pd.DataFrame(counts.astype("int64"), columns=list(COLS), index=range(1, len(counts) + 1))
        df = Override_index_positions(df, read_override_index(a.index_override))
        counts = df.values
    indexDict = _state.IndexDict(counts)
    GffHeader = IndexGff.header
    GffDict = IndexGff.index_dict(seqid=a.samplename)           # (TrueConsense.py:238-241: df["seqid"] = samplename; df.to_dict("index") — without importing pandas)

    if a.depth_of_coverage is not None:
        BuildCoverage(indexDict, a.depth_of_coverage)
    vparts = []
    if a.variant_table is not None:                 # from the counts the consensus is called from (behind --index-override)
        from .io import fasta
        refID, refseq = fasta.read_first_record(a.reference)
        recs = _state.default_context().variants(indexDict.counts, refseq, **variants_of(a))
        vparts = [(recs, got.get("variant_strand"), got.get("variant_links"), refID, refseq, 0)]
    vstats = dict(write_variant_tables(a, vparts, want), **evidence_stats())
    if want.indels:
        write_indel_table(want.indels, [(recs, got["indel_events"], refID, refseq, 0)])
    if want.evidence:
        vstats.update(write_variant_evidence(want.evidence[0], [(recs, got["variant_evidence"], refID, refseq, 0)], want.evidence[1]))

    amps, n_below = amplicons_of(a), 0
    if amps:                                        # likewise: the matrix behind the read filter, --min-baseq, --primers and --index-override
        arecs = _state.default_context().interval_stats(indexDict.counts, amplicon_intervals(amps), a.coverage_level)
        write_amplicon_table(a.amplicon_table, [(a.samplename, arecs)], amps)
        n_below = int((arecs["below"] > 0).sum())

    IncludeAmbig = a.noambiguity is False
    WriteOutputs(a.coverage_level, indexDict, GffDict, bam, IncludeAmbig, a.variants, a.samplename, a.reference,
                 a.output_gff, GffHeader, a.output)
    t["outputs"] = time.perf_counter()
    if a.stats:
        keys = list(t)
        with open(a.stats, "w") as fh:
            secs = {k: t[k] - t[keys[i - 1]] for i, k in enumerate(keys) if i}
            secs["bam_decode"] = secs["bam_open"]       # (round 1's name of the same span: the file is opened, decoded with the tally)
            json.dump({"seconds": secs, "positions": len(counts), "reads": build_counts.last_reads, "reads_filtered": build_counts.last_filtered,
                       "min_baseq": a.min_baseq, "primers": a.primer_rows, "reads_primer_masked": build_counts.last_primer_masked,
                       **mate_stats(a.mate_overlap, build_counts.last_mate_overlap), **dedup_stats(a.dedup, build_counts.last_dedup),
                       **vstats, "amplicons": len(amps) if amps else 0, "amplicons_below": n_below, **want.stats(got),
                       "bam_bytes": os.path.getsize(a.input)}, fh)


if __name__ == "__main__":
    main()
