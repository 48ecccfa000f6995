"""What --indel-table (tcmi_readset_indel_events) costs per file: the bench's file (1 M 150-bp reads on 29 903 positions, its compressed
bytes resident in HBM) `--reps` times through tcmi_bamfile_step and, behind each step, through the call on the read set the step
returned, for two queries:

    table    the distinct positions of the '*' and '+' rows of the file's variant table at the default thresholds.  A clean file has
             none: then the file is written once more with a 3-base deletion planted in every read that covers the middle of the
             reference, and that file is measured (the JSON line says which)
    spread   256 evenly spread columns

    indel_events     the three launches of a call (count, verify, gather), one hipEvent bracket around them (slot TCMI_K_INDEL_EVENTS)
    strand_counts    strand_counts_kernel on the same read set and the same columns (slot TCMI_K_STRAND_COUNTS), for scale: one walk
                     over the records where the indel call makes two, and no table
    wall             host time of the call itself: the columns sent, the launches, one wait, the events back

The totals of the last call are checked against the invariant: ins_total equals the I plane of the count matrix the step tallied.
Prints one line per query and a JSON line."""
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
from trueconsense_amd.engine import Context, DeviceBam, indel_columns   # noqa: E402
from trueconsense_amd.io import bamwriter                        # noqa: E402

BRACKETS = (("indel_events", _ffi.K_INDEL_EVENTS), ("strand_counts", _ffi.K_STRAND_COUNTS))


def table_columns(ctx, d, ref, L):
    ctx.set_variants(ref)                                        # (the default thresholds: the step lists the table's records)
    rs = ctx.bamfile_step(d, L, 30, True, want_counts=False)[0]
    cols, _ = indel_columns(ctx.step_variants())
    rs.free()
    ctx.set_variants()
    return cols


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    ref, _ = sy.make_reference()
    L = len(ref)
    out = {"reads": a.reads, "positions": L, "reps": a.reps}
    with tempfile.TemporaryDirectory() as tmp, Context(0) as ctx:
        path = os.path.join(tmp, "f.bam")
        reads = sy.make_reads(ref, a.reads, seed=1)
        bamwriter.write_bam_fast(path, reads["pos"], reads["flag"], reads["seq"].reshape(a.reads, -1), 150, "MN908947.3", L, level=6)
        d = DeviceBam(path).to_device(ctx)
        cols = table_columns(ctx, d, ref, L)
        out["file"] = "clean"
        if len(cols) == 0:                                       # nothing to ask a clean file: a deletion of three bases in every read over L / 2
            d.close()
            reads = sy.make_reads(ref, a.reads, seed=1, indel_sites=[(L // 2, "D", 3, 1.0)])
            bamwriter.write_bam(path, reads, "MN908947.3", L, level=6)
            d = DeviceBam(path).to_device(ctx)
            cols = table_columns(ctx, d, ref, L)
            out["file"] = "a 3-base deletion planted at %d in every read over it" % (L // 2 + 1)
        assert len(cols), "the variant table has no '*' or '+' row to ask about"
        queries = (("table", cols), ("spread", np.unique(np.linspace(0, L - 1, 256).astype(np.int64))))
        for key, cols in queries:
            wall = 0.0
            for rep in range(a.reps + 2):                        # (two untimed: the arena, the code objects, the scratch)
                if rep == 2:
                    ctx.sync()
                    ctx.profile(True)
                rs, _, _, _, counts = ctx.bamfile_step(d, L, 30, True, want_counts=True)
                cov = counts[cols, 0]
                t0 = time.perf_counter()
                events, text, totals = ctx.indel_events(rs, cols, cov)
                if rep >= 2:
                    wall += time.perf_counter() - t0
                ctx.strand_counts(rs, cols)
                rs.free()
            ms = {name: ctx.profile_get(k) for name, k in BRACKETS}
            ctx.profile(False)
            assert np.array_equal(totals["ins_total"], counts[cols, 6]) and (totals["del_total"] <= cov).all(), "the totals differ from the matrix the step tallied"
            out[key] = {"columns": len(cols), "events": len(events), "letters": len(text), "deletions_anchored": int(totals["del_total"].sum()),
                        "insertions_anchored": int(totals["ins_total"].sum()), "wall_ms_per_call": round(wall / a.reps * 1e3, 4)}
            for name, (t, c) in ms.items():
                out[key][name + "_ms_per_file"] = round(t / a.reps, 5)
                out[key][name + "_launch_brackets"] = c
            print("indel events %-7s: %d columns; %d events reported (%d deletions, %d insertions anchored); wall %.3f ms per call; %s" % (
                key, len(cols), len(events), out[key]["deletions_anchored"], out[key]["insertions_anchored"], wall / a.reps * 1e3,
                ", ".join("%s %.4f ms (%d brackets)" % (nm, t / a.reps, c) for nm, (t, c) in ms.items())))
        d.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
