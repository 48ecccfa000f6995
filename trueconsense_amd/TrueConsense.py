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
LOWQ, LOWMQ, END; counted likewise; needs --variant-table; not with --batch, --index-override or -i --gpus N), the codon table
--codon-table FILE (for every codon of the GFF's CDS rows that holds a row of the variant table the triplets the records carry there, with
their amino acids and EFFECT, under the variant table's thresholds: two changes on the same reads are one row; counted likewise; needs
--variant-table; not with --batch, --index-override or -i --gpus N), and

    python -m trueconsense_amd.TrueConsense --batch MANIFEST -ref r.fa -gff r.gff -cov 30 [-noambig] [-t N]

for many samples against one reference in one process: MANIFEST holds one sample per line, tab-separated:
input BAM, sample name, consensus FASTA and — optional, "-" or empty for "not wanted" — VCF, corrected GFF, coverage TSV
(the -i / -name / -o / -vcf / -ogff / -doc of the single-sample form).  The samples go through the native file runner
(csrc/pipeline.cpp): reading, GPU work and the host walk of consecutive samples overlap, all four outputs are written natively.
"""
from __future__ import annotations

import json
import os
import sys
import time

from . import _state
from .cli_args import (GetArgs, _child_argv, amplicon_intervals, amplicon_reads_of, amplicons_of, codons_of, evidence_of, links_of, primers_of,  # noqa: F401
                       read_filter_of, read_manifest, rules_of, strand_of, variants_of)
from .cli_tables import (CodonPart, StreamCounts, TablePart, amplicon_reads_text, codon_frames, dedup_stats, evidence_stats,  # noqa: F401
                         link_stats, mate_stats, write_amplicon_reads, write_amplicon_table, write_codon_table, write_tables)
from .Coverage import BuildCoverage
from .indexing import Gffindex, Override_index_positions, build_counts, read_override_index
from .launch import _spawn, run_gpus  # noqa: F401
from .Outputs import WriteOutputs


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
    IndexGff = None
    if want.codons:                                 # (the frames must be known behind the step: the GFF is read in front of it)
        IndexGff = Gffindex(a.features)
        want.frames = codon_frames(IndexGff.rows)
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
    IndexGff = IndexGff or Gffindex(a.features)
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
    parts = []
    if a.variant_table is not None:                 # from the counts the consensus is called from (behind --index-override)
        from .io import fasta
        refID, refseq = fasta.read_first_record(a.reference)
        recs = _state.default_context().variants(indexDict.counts, refseq, **variants_of(a))
        parts = [TablePart(recs, refID, refseq, 0, got.get("variant_strand"), got.get("variant_links"), got.get("indel_events"), got.get("variant_evidence"))]
    vstats = write_tables(a, parts, want)
    if want.codons:                                 # (its keys only with the flag: the dict of before otherwise)
        vstats.update(write_codon_table(a, [CodonPart(got["codon_counts"], *want.frames, refID, refseq, 0, indexDict.counts)], want))

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
