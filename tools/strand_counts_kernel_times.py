"""What --variant-strand (tcmi_readset_strand_counts) costs per file: the bench's file (1 M 150-bp reads on 29 903 positions, its
compressed bytes resident in HBM) `--reps` times through tcmi_bamfile_step and, behind each step, through the call on the read set the
step returned, for four queries:

    sparse   the distinct columns of the file's variant table at the default thresholds (a handful): columns and counters in LDS
    memory   513 evenly spread columns, TCMI_STRAND_LDS + 1 or more: searched and counted in memory
    staged_full / memory_least   TCMI_STRAND_LDS evenly spread columns (the largest staged query) and one more (the smallest in
             memory): the same walk and nearly the same search on both, so their difference is what LDS against memory costs

    strand_counts    strand_counts_kernel, one hipEvent bracket around its one launch (slot TCMI_K_STRAND_COUNTS)
    pk_index         the packer's record pass of THE SAME RUN (slot TCMI_K_PACK_CLASSIFY: below 16 384 BGZF blocks the bracket holds
                     pk_index alone)
    amplicon_reads   amplicon_reads_kernel on the same read set, a tiled scheme of about a hundred amplicons (slot
                     TCMI_K_AMPLICON_READS).  All three kernels read every record's fixed fields and CIGAR once: the other two are the
                     yardstick for what this pass should cost
    wall             host time of the call itself: the columns sent, the launch, the counters back, one wait

The counts of the last call are checked against the invariant: fwd + rev equals the count matrix the step tallied, on all seven
planes; both strands must hold reads.  Prints one line per query and a JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                               # noqa: E402
from trueconsense_amd import _ffi                                # noqa: E402
from trueconsense_amd import synthetic as sy                     # noqa: E402
from trueconsense_amd.engine import STRAND_LDS, Context, DeviceBam   # noqa: E402
from trueconsense_amd.io import bamwriter                        # noqa: E402

BRACKETS = (("strand_counts", _ffi.K_STRAND_COUNTS), ("pk_index", _ffi.K_PACK_CLASSIFY), ("amplicon_reads", _ffi.K_AMPLICON_READS))


def scheme(L, length=400, step=300, primer=24):
    return [(s, s + primer, s + length - primer, s + length) for s in range(30, L - length, step)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    ref, _ = sy.make_reference()
    reads = sy.make_reads(ref, a.reads, seed=1)
    L = len(ref)
    amps = scheme(L)
    out = {"reads": a.reads, "positions": L, "reps": a.reps, "lds_capacity_columns": STRAND_LDS}
    with tempfile.TemporaryDirectory() as tmp, Context(0) as ctx:
        path = os.path.join(tmp, "f.bam")
        bamwriter.write_bam_fast(path, reads["pos"], reads["flag"], reads["seq"].reshape(a.reads, -1), 150, "MN908947.3", L, level=6)
        d = DeviceBam(path).to_device(ctx)
        ctx.set_variants(ref)                                    # (the default thresholds: the step lists the table's records)
        rs = ctx.bamfile_step(d, L, 30, True, want_counts=False)[0]
        table_cols = np.unique(ctx.step_variants()["pos"].astype(np.int64))
        rs.free()
        ctx.set_variants()
        spread = lambda n: np.unique(np.linspace(0, L - 1, n).astype(np.int64))
        queries = (("sparse", table_cols), ("memory", spread(max(513, STRAND_LDS + 1))), ("staged_full", spread(STRAND_LDS)), ("memory_least", spread(STRAND_LDS + 1)))
        assert 1 <= len(queries[0][1]) <= STRAND_LDS < len(queries[1][1]) and len(queries[2][1]) == STRAND_LDS == len(queries[3][1]) - 1
        for key, cols in queries:
            wall = 0.0
            for rep in range(a.reps + 2):                        # (two untimed: the arena, the code objects, the scratch)
                if rep == 2:
                    ctx.sync()
                    ctx.profile(True)
                last = rep == a.reps + 1
                rs, _, _, _, counts = ctx.bamfile_step(d, L, 30, True, want_counts=last)
                t0 = time.perf_counter()
                got = ctx.strand_counts(rs, cols)
                if rep >= 2:
                    wall += time.perf_counter() - t0
                ctx.amplicon_reads(rs, amps, 5)
                rs.free()
            ms = {name: ctx.profile_get(k) for name, k in BRACKETS}
            ctx.profile(False)
            assert np.array_equal(got["fwd"] + got["rev"], counts[cols]), "fwd + rev differs from the count matrix the step tallied"
            assert got["fwd"][:, 0].any() and got["rev"][:, 0].any() and np.array_equal(got["pos"], cols)
            out[key] = {"columns": len(cols), "wall_ms_per_call": round(wall / a.reps * 1e3, 4)}
            for name, (t, c) in ms.items():
                out[key][name + "_ms_per_file"] = round(t / a.reps, 5)
                out[key][name + "_launch_brackets"] = c
            print("strand counts %-12s: %d columns; wall %.3f ms per call; %s; forward %d, reverse %d tokens of coverage (fwd + rev == the step's matrix)" % (
                key, len(cols), wall / a.reps * 1e3, ", ".join("%s %.4f ms (%d brackets)" % (nm, t / a.reps, c) for nm, (t, c) in ms.items()),
                int(got["fwd"][:, 0].sum()), int(got["rev"][:, 0].sum())))
        d.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
