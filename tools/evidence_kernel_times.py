"""What --variant-evidence (tcmi_readset_evidence_counts) costs per file: the bench's file (1 M 150-bp reads on 29 903 positions, its
compressed bytes resident in HBM) through tcmi_bamfile_step and, behind each step, through the call on the read set the step returned,
for three queries:

    table    the distinct positions of the file's variant table at the default thresholds (staged in LDS when at most 128)
    spread   128 evenly spread columns (staged in LDS)
    dense    every column of the reference (counted in memory)

    evidence_counts         evidence_counts_kernel, a wavefront's lanes joined per column (slot TCMI_K_EVIDENCE_COUNTS)
    strand_counts           strand_counts_kernel on the same read set and the same columns (slot TCMI_K_STRAND_COUNTS): the same walk with
                            a quarter of the counters, the yardstick
    wall                    host time of the call itself: the columns sent, the launch, one wait, the counters back

Two untimed reps first, then `--turns` turns of `--reps` reps each; a turn's figure is the mean of its brackets, the line gives the median
turn and the spread (min - max) over the turns.  n of the last call is checked against the count matrix the step tallied.  Prints one
line per query and a JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                               # noqa: E402
from trueconsense_amd import _ffi                                # noqa: E402
from trueconsense_amd import synthetic as sy                     # noqa: E402
from trueconsense_amd.engine import Context, DeviceBam           # noqa: E402
from trueconsense_amd.io import bamwriter                        # noqa: E402


def table_columns(ctx, d, ref, L):
    ctx.set_variants(ref)                                        # (the default thresholds: the step lists the table's records)
    rs = ctx.bamfile_step(d, L, 30, True, want_counts=False)[0]
    cols = np.unique(ctx.step_variants()["pos"].astype(np.int64))
    rs.free()
    ctx.set_variants()
    return cols


def turn(ctx, d, L, cols, reps):
    """reps x (step, the evidence call, the strand call) between one pair of profile switches
    -> ({name: ms per file}, wall ms per call, the last counters, the last matrix)"""
    wall = 0.0
    ctx.sync()
    ctx.profile(True)
    for _ in range(reps):
        rs, _, _, _, counts = ctx.bamfile_step(d, L, 30, True, want_counts=True)
        t0 = time.perf_counter()
        ev = ctx.evidence_counts(rs, cols)
        wall += time.perf_counter() - t0
        ctx.strand_counts(rs, cols)
        rs.free()
    ms = {"evidence_counts": ctx.profile_get(_ffi.K_EVIDENCE_COUNTS)[0] / reps, "strand_counts": ctx.profile_get(_ffi.K_STRAND_COUNTS)[0] / reps}
    ctx.profile(False)
    return ms, wall / reps * 1e3, ev, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--turns", type=int, default=5)
    a = ap.parse_args()
    ref, _ = sy.make_reference()
    L = len(ref)
    out = {"reads": a.reads, "positions": L, "reps": a.reps, "turns": a.turns}
    with tempfile.TemporaryDirectory() as tmp, Context(0) as ctx:
        path = os.path.join(tmp, "f.bam")
        reads = sy.make_reads(ref, a.reads, seed=1)
        bamwriter.write_bam_fast(path, reads["pos"], reads["flag"], reads["seq"].reshape(a.reads, -1), 150, "MN908947.3", L, level=6)
        d = DeviceBam(path).to_device(ctx)
        queries = [("table", table_columns(ctx, d, ref, L)), ("spread", np.unique(np.linspace(0, L - 1, 128).astype(np.int64))), ("dense", np.arange(L, dtype=np.int64))]
        for key, cols in queries:
            if len(cols) == 0:
                print("evidence counts %-6s: the variant table of this file has no row" % key)
                continue
            turn(ctx, d, L, cols, 2)                             # (untimed: the arena, the code objects, the scratch)
            seen, walls = {}, []
            for _ in range(a.turns):
                ms, wall, ev, counts = turn(ctx, d, L, cols, a.reps)
                for name, v in ms.items():
                    seen.setdefault(name, []).append(v)
                walls.append(wall)
                assert np.array_equal(ev["n"], counts[cols]), "n differs from the matrix the step tallied"
            out[key] = {"columns": len(cols), "tokens": int(ev["n"][:, 0].sum()), "wall_ms_per_call": round(statistics.median(walls), 4)}
            for name, v in seen.items():
                out[key][name + "_ms_per_file"] = {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}
            print("evidence counts %-6s: %d columns, %d tokens; wall %.3f ms per call; %s" % (
                key, len(cols), out[key]["tokens"], out[key]["wall_ms_per_call"],
                ", ".join("%s %.4f ms (%.4f - %.4f)" % (nm, statistics.median(v), min(v), max(v)) for nm, v in seen.items())))
        d.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
