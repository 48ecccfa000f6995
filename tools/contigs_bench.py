"""--per-contig cost: file -> FASTA text in M positions/s, one context, files in the page cache (PCIe and the host walk included).

    python tools/contigs_bench.py [--reads 1000000] [--reps 20] [--only a,b,c]

  (a) the bench's reads (1 M x 150 bp over the 29 903-bp bench genome) dealt over 8 contigs with influenza-like lengths
      (2341, 2341, 2233, 1778, 1565, 1413, 1027, 890, scaled to the same 29 903 positions): a read belongs to the contig its
      start lies in (reads that cross a boundary overhang their contig's end, inside the guard); the per-contig flow under an
      8-contig layout (trueconsense_amd.contigs.step_contigs, then each contig's slice walked to its FASTA record)
  (b) the same reads as one contig, the default path: tcmi_bamfile_step (the one-sync path) + the walk
  (c) the same single-contig file under a one-contig layout: the per-contig flow on one contig (the cost of the layout lookup
      and of the two-call path it takes)

The steps are identical in their walk and text; only the decode + pack + tally + call differ.  For kernel times run one mode under
`rocprofv3 --kernel-trace --stats -- python tools/contigs_bench.py --only c --reps 5`.  One JSON line per mode.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from trueconsense_amd import contigs, engine, synthetic as sy  # noqa: E402
from trueconsense_amd.io import bamwriter  # noqa: E402
from trueconsense_amd.Sequences import consensus_from_records  # noqa: E402

FLU = (2341, 2341, 2233, 1778, 1565, 1413, 1027, 890)
MINCOV = 30


def flu_lengths(total):
    w = np.asarray(FLU, np.float64)
    lens = np.floor(w * total / w.sum()).astype(np.int64)
    lens[0] += total - lens.sum()
    return lens.tolist()


def fasta_text(name, plain, alt, flags):
    cons = consensus_from_records(plain, alt, flags, {}, None, True)[0]
    return ">%s mincov=%d\n%s\n" % (name, MINCOV, cons)


def per_contig(ctx, path, records, hdr):
    names, lens = hdr
    shift, slot, axis = contigs.layout_for(records, names, lens)
    plain, alt, flags, _, ext, _, _ = contigs.step_contigs(ctx, path, shift, slot, axis, MINCOV, True, names, want_counts=False)
    out = []
    for t, (rid, seq) in enumerate(records):
        s, L = int(shift[t]), max(len(seq), int(ext[t]), 1)
        out.append(fasta_text("S_" + rid, plain[s:s + L], alt[s:s + L], flags[s:s + L]))
    return "".join(out)


def default_path(ctx, path, ref_len):
    d = engine.DeviceBam(path)
    rs, plain, alt, flags, _ = ctx.bamfile_step(d, ref_len, MINCOV, True, want_counts=False)
    rs.free()
    d.close()
    return fasta_text("S", plain, alt, flags)


def timed(fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="a,b,c")
    a = ap.parse_args()
    ref, _ = sy.make_reference()
    G = len(ref)
    reads = sy.make_reads(ref, a.reads, seed=1)
    n = a.reads
    seq = reads["seq"].reshape(n, -1)
    lens = flu_lengths(G)
    starts = np.concatenate(([0], np.cumsum(lens)[:-1]))
    tid = (np.searchsorted(starts, reads["pos"], side="right") - 1).astype(np.int32)
    local = (reads["pos"] - starts[tid]).astype(np.int32)
    seg = ["seg%d" % (k + 1) for k in range(8)]
    records8 = [(seg[k], ref[starts[k]:starts[k] + lens[k]]) for k in range(8)]
    with tempfile.TemporaryDirectory(prefix="contigs_bench_") as tmp, engine.Context(0) as ctx:
        one = os.path.join(tmp, "one.bam")
        eight = os.path.join(tmp, "eight.bam")
        bamwriter.write_bam_fast(one, reads["pos"], reads["flag"], seq, 150, "genome", G, level=6)
        bamwriter.write_bam_fast(eight, local, reads["flag"], seq, 150, level=6, tid=tid, refs=list(zip(seg, lens)))
        jobs = {
            "a": ("8 contigs, per-contig flow", lambda: per_contig(ctx, eight, records8, (seg, lens))),
            "b": ("1 contig, default path (tcmi_bamfile_step)", lambda: default_path(ctx, one, G)),
            "c": ("1 contig, per-contig flow (one-contig layout)", lambda: per_contig(ctx, one, [("genome", ref)], (["genome"], [G]))),
        }
        # the same consensus either way: the 8 records are the one-contig consensus cut at the contig starts (away from the cuts)
        if "a" in a.only and "c" in a.only:
            t8, t1 = jobs["a"][1](), jobs["c"][1]()
            c1 = t1.split("\n")[1]
            c8 = [ln for ln in t8.split("\n") if ln and not ln.startswith(">")]
            assert all(c8[k][200:lens[k] - 200] == c1[starts[k] + 200:starts[k] + lens[k] - 200] for k in range(8)), "contig slices differ"
        for key in a.only.split(","):
            what, fn = jobs[key]
            med, best = timed(fn, a.reps)
            print(json.dumps({"mode": key, "what": what, "reads": n, "positions": G, "ms_median": med * 1e3, "ms_best": best * 1e3,
                              "M_positions_per_s": G / med / 1e6, "reps": a.reps}))
            sys.stdout.flush()


if __name__ == "__main__":
    main()
