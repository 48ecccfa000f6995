"""What --variant-links (tcmi_readset_link_counts) costs per file: the bench's file (1 M 150-bp reads on 29 903 positions, its
compressed bytes resident in HBM) `--reps` times through tcmi_bamfile_step and, behind each step, through the call on the read set the
step returned, at the distinct columns of the file's variant table at --min-af 0.03 (the command line's default), with K = 2 and K = 7
neighbours (both staged in LDS), and — to see the memory route — at 200 columns 50 apart (three a read) with K = 2:

    link_counts      link_counts_kernel, one hipEvent bracket around its one launch (slot TCMI_K_LINK_COUNTS)
    strand_counts    strand_counts_kernel on THE SAME read set and columns in the same run (slot TCMI_K_STRAND_COUNTS): both kernels
                     read every record's fixed fields, search the columns and do the same CIGAR walk, so the difference is the counting
    wall             host time of the link call itself: the columns sent, the launch, the counters back, one wait

Two untimed repetitions come first (the arena, the code objects, the scratch), then the timed ones; the brackets' means are reported.
The counts of the last call are checked against the invariant: the classes at either column of every pair add up to the count matrix
the step tallied.

--bench N: also `bench.py --gpus 1 --steps S --warmup W --no-cpu-baseline --no-cli-batch` N times, each in a process of its own, with no flag set (nothing of this
feature is launched there), and with --parent DIR (a built checkout of the parent commit) that tree's bench.py turn about with this
one's: the medians and their ratio, which must stay inside the +- 3 % the README states for run-to-run spread.
Prints one line per query and a JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                               # noqa: E402
from trueconsense_amd import _ffi                                # noqa: E402
from trueconsense_amd import synthetic as sy                     # noqa: E402
from trueconsense_amd.engine import LINKS_LDS, Context, DeviceBam    # noqa: E402
from trueconsense_amd.io import bamwriter                        # noqa: E402

BRACKETS = (("link_counts", _ffi.K_LINK_COUNTS), ("strand_counts", _ffi.K_STRAND_COUNTS))


def adds_up(links, counts):
    """the invariant of include/tcmi.h on every pair with b >= 0"""
    for r in links:
        if r["b"] < 0:
            continue
        j = r["j"].astype(np.int64)
        for col, got in ((int(r["a"]), j.sum(1)), (int(r["b"]), j.sum(0))):
            row = counts[col].astype(np.int64) if col < len(counts) else np.zeros(7, np.int64)
            if got[1:6].tolist() != row[1:6].tolist() or got[6] != row[0] - row[1:6].sum():
                return False
    return True


def bench_value(tree, steps, warmup):
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline", "--no-cli-batch"], cwd=tree,
                       capture_output=True, text=True, timeout=900)
    if r.returncode:
        raise RuntimeError("bench.py in %s failed:\n%s" % (tree, r.stderr[-2000:]))
    return float(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])["value"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--bench", type=int, default=0, metavar="N", help="also run bench.py N times (a process each) with no flag set")
    ap.add_argument("--bench-steps", type=int, default=100)
    ap.add_argument("--bench-warmup", type=int, default=10)
    ap.add_argument("--parent", default=None, metavar="DIR", help="a built checkout of the parent commit: its bench.py turn about with this one's")
    a = ap.parse_args()
    ref, _ = sy.make_reference()
    reads = sy.make_reads(ref, a.reads, seed=1)
    L = len(ref)
    out = {"reads": a.reads, "positions": L, "reps": a.reps, "lds_capacity_pairs": LINKS_LDS}
    with tempfile.TemporaryDirectory() as tmp, Context(0) as ctx:
        path = os.path.join(tmp, "f.bam")
        bamwriter.write_bam_fast(path, reads["pos"], reads["flag"], reads["seq"].reshape(a.reads, -1), 150, "MN908947.3", L, level=6)
        d = DeviceBam(path).to_device(ctx)
        ctx.set_variants(ref, min_af="0.03")                     # (the step lists the table's records)
        rs = ctx.bamfile_step(d, L, 30, True, want_counts=False)[0]
        table_cols = np.unique(ctx.step_variants()["pos"].astype(np.int64))
        rs.free()
        ctx.set_variants()
        spread = L // 3 + 50 * np.arange(200, dtype=np.int64)       # (three columns a 150-base read: pairs that records span)
        queries = (("table_k2", table_cols, 2), ("table_k7", table_cols, 7), ("memory_k2", spread, 2))
        assert 1 <= len(table_cols) and len(table_cols) * 7 <= LINKS_LDS < len(spread) * 2, (len(table_cols), LINKS_LDS)
        for key, cols, k in queries:
            wall = 0.0
            for rep in range(a.reps + 2):                        # (two untimed: the arena, the code objects, the scratch)
                if rep == 2:
                    ctx.sync()
                    ctx.profile(True)
                last = rep == a.reps + 1
                rs, _, _, _, counts = ctx.bamfile_step(d, L, 30, True, want_counts=last)
                t0 = time.perf_counter()
                got = ctx.link_counts(rs, cols, k)
                if rep >= 2:
                    wall += time.perf_counter() - t0
                ctx.strand_counts(rs, cols)
                rs.free()
            ms = {name: ctx.profile_get(kid) for name, kid in BRACKETS}
            ctx.profile(False)
            assert adds_up(got, counts), "the link counts do not add up to the count matrix the step tallied"
            spanning = int(got["j"][:, 1:, 1:].sum())
            assert spanning > 0 or key.startswith("table")      # (the table's columns may lie further apart than a read)
            out[key] = {"columns": len(cols), "neighbours": k, "pairs": len(cols) * k, "staged": len(cols) * k <= LINKS_LDS,
                        "wall_ms_per_call": round(wall / a.reps * 1e3, 4)}
            for name, (t, c) in ms.items():
                out[key][name + "_ms_per_file"] = round(t / a.reps, 5)
                out[key][name + "_launch_brackets"] = c
            print("link counts %-10s: %d columns x %d neighbours; wall %.3f ms per call; %s; %d records with a token at both columns of a pair (adds up to the step's matrix)" % (
                key, len(cols), k, wall / a.reps * 1e3, ", ".join("%s %.4f ms (%d brackets)" % (nm, t / a.reps, c) for nm, (t, c) in ms.items()), spanning))
        d.close()
    if a.bench:
        trees = [("this", ROOT)] + ([("parent", os.path.abspath(a.parent))] if a.parent else [])
        values = {name: [] for name, _ in trees}
        for turn in range(a.bench):                              # turn about, the order swapped every turn
            for name, tree in (trees if turn % 2 == 0 else trees[::-1]):
                values[name].append(bench_value(tree, a.bench_steps, a.bench_warmup))
        out["bench"] = {name: {"values": [round(v) for v in vs], "median": round(statistics.median(vs))} for name, vs in values.items()}
        line = "; ".join("%s %s M positions/s (median %.1f)" % (name, " / ".join("%.1f" % (v / 1e6) for v in vs), statistics.median(vs) / 1e6) for name, vs in values.items())
        if a.parent:
            ratio = statistics.median(values["this"]) / statistics.median(values["parent"])
            out["bench"]["this_over_parent"] = round(ratio, 4)
            line += "; this / parent = %.4f (%s +- 3 %%)" % (ratio, "inside" if abs(ratio - 1) <= 0.03 else "OUTSIDE")
        print("bench.py --gpus 1 --steps %d --warmup %d --no-cpu-baseline --no-cli-batch, no flag set: %s" % (a.bench_steps, a.bench_warmup, line))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
