"""The command line's arguments: what turns `argv` into settings.  No GPU and no library call — the `type=` callables, GetArgs with
its refusals and late defaults, the --batch manifest, the translators from the parsed namespace to the engine's arguments
(variants_of, rules_of, amplicons_of, ...) and the command line of a --gpus child (_child_argv)."""
from __future__ import annotations

import argparse
import multiprocessing
import os
import pathlib
import sys

from .func import MyHelpFormatter, color
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


def strand_of(a):
    """The parsed namespace's --variant-strand thresholds as keyword arguments of engine.variants_strand_text, or None without the flag."""
    if not getattr(a, "variant_strand", False):
        return None
    return dict(min_strand_depth=int(a.strand_min_depth), strand_ratio=a.strand_ratio)


def links_of(a):
    """The parsed namespace's --variant-links settings as (file, neighbours, keyword arguments of engine.variants_links_text), or None
    without the flag."""
    if getattr(a, "variant_links", None) is None:
        return None
    return a.variant_links, int(a.link_neighbours), dict(min_depth=int(a.link_min_depth), ratio=a.link_ratio)


def codons_of(a):
    """The parsed namespace's --codon-table file, or None without the flag (its thresholds are the variant table's: variants_of)."""
    return getattr(a, "codon_table", None)


def evidence_of(a):
    """The parsed namespace's --variant-evidence settings as (file, keyword arguments of engine.variants_evidence_text), or None without
    the flag."""
    if getattr(a, "variant_evidence", None) is None:
        return None
    return a.variant_evidence, dict(min_qual=int(a.evidence_min_qual), min_mapq=int(a.evidence_min_mapq), min_enddist=int(a.evidence_min_enddist))


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


def _reference_name(a):
    """The name of the reference this run is on: the BAM header's first name, else (--batch: every sample on the reference the FASTA
    names) the first record of -ref."""
    from .contigs import bam_header_refs
    names = bam_header_refs(a.input)[0] if getattr(a, "input", None) else []
    if names:
        return names[0]
    from .io import fasta
    return fasta.read_first_record(a.reference)[0]


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
        name = _reference_name(a)
        out = [(m, 0) for m in amps if m.chrom == name]
        where = 'the reference "%s"' % name
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


def amplicon_intervals(amps):
    """amplicons_of's list -> [(start, end)] on the count matrix's axis, as Context.set_intervals / interval_stats take them."""
    return [(m.start + sh, m.end + sh) for m, sh in amps]


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
    name = _reference_name(a)
    rows = pb.rows_for_reference(bed, name)
    if not rows:
        print(f'--primers: no row of {a.primers} is on the reference "{name}". Exiting...')
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
        (("--batch",), dict(type=str, default=None, metavar="File",
                            help="many samples: a tab-separated manifest (BAM, name, FASTA[, VCF, GFF, TSV] per line)\n"
                                 "instead of -i / -name / -o / -vcf / -ogff / -doc")),
        (("--gpus",), dict(type=int, default=1, metavar="N",
                           help="GPUs of this node to use: with --batch the manifest's samples are dealt to N processes,\n"
                                "one per GPU (independent files, no exchange); with -i ONE BAM file is shared — every GPU\n"
                                "takes a range of its BGZF blocks, one reduce of the count matrix")),
        (("--per-contig",), dict(action="store_true",
                                 help="one consensus per record of -ref (a multi-record reference, e.g. a segmented virus):\n"
                                      "records named {name}_{record}, all in -o; -vcf / -ogff / -doc cover every record")),
        (("--min-mapq",), dict(type=_range_arg(parser, "--min-mapq", 255), default=0, metavar="N",
                               help="ignore alignment records with MAPQ below N (samtools view -q)")),
        (("--require-flags",), dict(type=_range_arg(parser, "--require-flags", 0xFFFF), default=0, metavar="F",
                                    help="ignore records that lack any of these FLAG bits (samtools view -f; decimal or 0x...)")),
        (("--exclude-flags",), dict(type=_range_arg(parser, "--exclude-flags", 0xFFFF), default=0, metavar="F",
                                    help="ignore records with any of these FLAG bits, e.g. 0x400 duplicates, 0x900 secondary\n"
                                         "and supplementary (samtools view -F; decimal or 0x...)")),
        (("--min-baseq",), dict(type=_range_arg(parser, "--min-baseq", 255), default=0, metavar="N",
                                help="skip pileup tokens (a read on a column) whose base quality is below N in the count matrix\n"
                                     "(samtools mpileup -Q; qualities as the file stores them); needs the device decoder")),
        (("--mate-overlap",), dict(action="store_true",
                                   help="count the columns that the two mates of a read pair share once in the count matrix: the\n"
                                        "mate that starts further right loses them (samtools mpileup's default; by position, qualities\n"
                                        "are not summed), joined by read name on the device; needs the device decoder; not with\n"
                                        "-i --gpus N")),
        (("--dedup",), dict(action="store_true",
                            help="ignore duplicate templates in the count matrix (samtools markdup, Picard MarkDuplicates): of the\n"
                                 "fragments with one unclipped 5' end and strand, and of the proper pairs with the same two, the one\n"
                                 "with the highest sum of base qualities >= 15 is kept, found on the device; nothing is written back;\n"
                                 "needs the device decoder; not with -i --gpus N, not with --amplicon-reads")),
        (("--primers",), dict(type=str, default=None, metavar="File",
                              help="BED of the amplicon scheme's primers (chrom, start, end, name, pool, strand): a read's tokens\n"
                                   "inside the primer at its head ('+') or tail ('-') stay out of the count matrix\n"
                                   "(ivar trim, samtools ampliconclip); needs the device decoder")),
        (("--primer-slack",), dict(type=_range_arg(parser, "--primer-slack", 1000), default=0, metavar="N",
                                   help="a read may start up to N columns in front of a primer (end behind it) and still be masked")),
        (("--variant-table",), dict(type=str, default=None, metavar="File",
                                    help="also write per position every non-reference allele (A, T, C, G, * deletion, + insertion\n"
                                         "mark) at or above --min-af, tab-separated: REGION POS REF ALT ALT_DP TOTAL_DP ALT_FREQ\n"
                                         "(ivar variants), from the count matrix the consensus is called from")),
        (("--min-af",), dict(type=_min_af_arg(parser), default=None, metavar="F",
                             help="minimum allele frequency of the variant table, 0..1, a decimal or n/d (default 0.03)")),
        (("--min-alt-depth",), dict(type=_count_arg(parser, "--min-alt-depth", 1), default=None, metavar="N",
                                    help="minimum reads with the allele (default 1)")),
        (("--variant-min-depth",), dict(type=_count_arg(parser, "--variant-min-depth", 0), default=None, metavar="N",
                                        help="minimum coverage of a position of the variant table (ivar variants -m; default 10;\n"
                                             "independent of -cov)")),
        (("--variant-strand",), dict(action="store_true",
                                     help="the variant table's rows also say how the allele's reads split by strand (FLAG 0x10):\n"
                                          "REF_FWD REF_REV ALT_FWD ALT_REV TOTAL_FWD TOTAL_REV and STRAND = PASS, BIAS or LOW, counted\n"
                                          "in the records the device decoded; needs --variant-table and the device decoder; not with\n"
                                          "--batch or --index-override")),
        (("--strand-min-depth",), dict(type=_count_arg(parser, "--strand-min-depth", 1), default=None, metavar="N",
                                       help="STRAND is LOW when either strand covers the position with fewer than N reads (default 10)")),
        (("--strand-ratio",), dict(type=_min_af_arg(parser, "--strand-ratio"), default=None, metavar="F",
                                   help="STRAND is BIAS when the allele's frequency on one strand is below F times its frequency on\n"
                                        "the other, 0..1, a decimal or n/d (default 1/10)")),
        (("--variant-links",), dict(type=str, default=None, metavar="File",
                                    help="also write, for every two rows of the variant table at most K distinct positions apart, how\n"
                                         "many alignment records carry both alleles, one of them or neither: REGION POS_A REF_A ALT_A\n"
                                         "POS_B REF_B ALT_B SPAN BOTH ONLY_A ONLY_B NEITHER PHASE (CIS, TRANS, MIXED, NONE or LOW),\n"
                                         "counted in the records the device decoded; needs --variant-table and the device decoder;\n"
                                         "not with --batch or --index-override; '+' rows are not linked")),
        (("--link-neighbours",), dict(type=_neighbours_arg(parser), default=None, metavar="K",
                                      help="link a row's position with the next K distinct positions of the table, 1..7 (default 2)")),
        (("--link-min-depth",), dict(type=_count_arg(parser, "--link-min-depth", 1), default=None, metavar="N",
                                     help="PHASE is LOW when fewer than N records have a token at both positions (default 10)")),
        (("--link-ratio",), dict(type=_link_ratio_arg(parser), default=None, metavar="F",
                                 help="PHASE is CIS when BOTH is at least F of the rarer allele's records among those that span\n"
                                      "both positions, TRANS when at most 1 - F; above 1/2 up to 1, a decimal or n/d (default 9/10)")),
        (("--indel-table",), dict(type=str, default=None, metavar="File",
                                  help="also write every insertion and every deletion at the variant table's '+' and '*' positions as\n"
                                       "one row: REGION POS TYPE (INS / DEL) LEN SEQ COUNT TOTAL_DP FREQ (ivar variants' +ACG / -3),\n"
                                       "under --min-af / --min-alt-depth / --variant-min-depth, counted in the records the device\n"
                                       "decoded; needs --variant-table and the device decoder; not with --batch, --index-override\n"
                                       "or -i --gpus N")),
        (("--variant-evidence",), dict(type=str, default=None, metavar="File",
                                       help="also write the variant table's rows with what says whether an allele can be trusted: REF_QUAL\n"
                                            "ALT_QUAL (mean base quality, ivar variants'), REF_MAPQ ALT_MAPQ (mean mapping quality of the\n"
                                            "records), REF_ENDDIST ALT_ENDDIST (mean distance to the nearer end of the read's aligned\n"
                                            "part, capped at 255) and EVIDENCE = PASS or LOWQ, LOWMQ, END, counted in the records the\n"
                                            "device decoded; needs --variant-table and the device decoder; not with --batch,\n"
                                            "--index-override or -i --gpus N")),
        (("--evidence-min-qual",), dict(type=_range_arg(parser, "--evidence-min-qual", 255), default=None, metavar="Q",
                                        help="EVIDENCE names LOWQ when the allele's mean base quality is below Q; 0: off (default 20)")),
        (("--evidence-min-mapq",), dict(type=_range_arg(parser, "--evidence-min-mapq", 255), default=None, metavar="Q",
                                        help="EVIDENCE names LOWMQ when the mean MAPQ of the allele's records is below Q; 0: off (default 20)")),
        (("--evidence-min-enddist",), dict(type=_range_arg(parser, "--evidence-min-enddist", 255), default=None, metavar="N",
                                           help="EVIDENCE names END when the allele sits on average fewer than N bases from its reads'\n"
                                                "nearer end; 0: off (default 5)")),
        (("--codon-table",), dict(type=str, default=None, metavar="File",
                                  help="also write what the variant table's rows mean for the protein: for every codon of the GFF's\n"
                                       "CDS rows that holds a row of the table, each triplet the records carry there that passes\n"
                                       "--min-af / --min-alt-depth / --variant-min-depth: REGION FEATURE STRAND CODON POS REF_CODON\n"
                                       "REF_AA ALT_CODON ALT_AA EFFECT (SYN, MIS, STOP_GAINED, STOP_LOST, DEL, UNKNOWN) SUBS COUNT SPAN\n"
                                       "FREQ PARTIAL OTHER INS_INSIDE; two changes on the same reads are one row, counted in the\n"
                                       "records the device decoded; needs --variant-table and the device decoder; not with --batch,\n"
                                       "--index-override or -i --gpus N")),
        (("--amplicon-table",), dict(type=str, default=None, metavar="File",
                                     help="also write per amplicon of the scheme the depth of its columns, tab-separated: SAMPLE REGION\n"
                                          "AMPLICON POOL START END LEN MEAN MEDIAN MIN MIN_POS BELOW (BELOW: columns under -cov), from\n"
                                          "the count matrix the consensus is called from; --batch: one file, every sample's rows")),
        (("--amplicon-scheme",), dict(type=str, default=None, metavar="File",
                                      help="BED of the scheme's primers, named {amplicon}_LEFT / _RIGHT[_alt] (default: the file of --primers)")),
        (("--amplicon-region",), dict(choices=("insert", "unique", "full"), default=None,
                                      help="the columns of an amplicon: between its primers (insert, the default), the insert\n"
                                           "outside every other amplicon (unique), or primers included (full)")),
        (("--amplicon-reads",), dict(type=str, default=None, metavar="File",
                                     help="also write per amplicon of the scheme the alignment records that lie inside it and inside no\n"
                                          "other, tab-separated: SAMPLE REGION AMPLICON POOL READS FULL_LENGTH (FULL_LENGTH: those that start\n"
                                          "in its left primer and end in its right one), then the records inside several amplicons\n"
                                          "(*ambiguous) and inside none (*unassigned); needs the device decoder; not with --batch")),
        (("--amplicon-reads-slack",), dict(type=_range_arg(parser, "--amplicon-reads-slack", 1000), default=None, metavar="N",
                                           help="a read may reach up to N columns beyond an amplicon's outer primer ends and still lie\n"
                                                "inside it (default 5)")),
    ]
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
                           ("--variant-evidence", a.variant_evidence is not None, ("evidence_min_qual", "evidence_min_mapq", "evidence_min_enddist")),
                           ("--codon-table", a.codon_table is not None, ())):
        names = " / ".join("--" + d.replace("_", "-") for d in deps)
        for bad, why in ((not on and any(getattr(a, d) is not None for d in deps), f"{names} need {flag}."),
                         (on and a.batch is not None, f"{flag} goes with a single sample (-i): --batch is refused, its file runner has no hook behind its steps."),
                         (on and a.batch is None and a.variant_table is None, f"{flag} needs --variant-table."),
                         (on and a.index_override is not None, f"{flag} does not go with --index-override: the overridden matrix no longer equals the reads."),
                         (on and flag == "--indel-table" and a.batch is None and a.gpus and a.gpus > 1,
                          f"{flag} does not go with -i --gpus N: the ranks' event lists would have to be merged on rank 0, which is not built."),
                         (on and flag == "--variant-evidence" and a.batch is None and a.gpus and a.gpus > 1,
                          f"{flag} does not go with -i --gpus N: the ranks' sums would have to be added up on rank 0, which is not built."),
                         (on and flag == "--codon-table" and a.batch is None and a.gpus and a.gpus > 1,
                          f"{flag} does not go with -i --gpus N: the ranks' counters would have to be added up on rank 0, which is not built.")):
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
        if getattr(a, "codon_table", None):
            out += ["--codon-table", a.codon_table]
        if a.amplicon_table:
            out += ["--amplicon-table", a.amplicon_table]
        out += ["-i", a.input, "-o", a.output, "-name", a.samplename]
        for flag, v in (("-vcf", a.variants), ("-doc", a.depth_of_coverage), ("-ogff", a.output_gff)):
            if v is not None:
                out += [flag, v]
    return out + ["--gpus", "1"]
