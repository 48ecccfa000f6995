"""What --codon-table (tcmi_readset_codon_counts) costs per file: the bench's file (1 M 150-bp reads on 29 903 positions, its
compressed bytes resident in HBM) `--reps` times through tcmi_bamfile_step and, behind each step, through the call on the read set the
step returned, at the codons of the synthetic reference's CDS rows that hold a row of the file's variant table at --min-af 0.03 (the
command line's default: tcmi_codon_select), and beside it tcmi_readset_link_counts with K = 2 at the same table's distinct columns:

    table_codons     all of the table's codons in one call (up to TCMI_CODONS_LDS: counted in LDS, else with atomics in memory)
    staged_codons    when they are more than TCMI_CODONS_LDS: the first TCMI_CODONS_LDS of them (counted in LDS); else
    memory_codons    the same codons padded past TCMI_CODONS_LDS with codons behind every read (counted in memory)
    two_frames       the table's codons and every one of them again one column up: overlapping frames, the register of visited
                     columns reused
    table_links_k2   link_counts_kernel at the table's columns, K = 2: the closest existing kernel (the same walk, two token_at per
                     visited column pair against at most three per codon)

Both kernels are filed under TCMI_K_LINK_COUNTS, so every query is timed in a window of its own: one hipEvent bracket around the one
launch of a call.  wall is the host time of the call itself: the columns sent, the launch, the counters back, one wait.  Two untimed
repetitions come first (the arena, the code objects, the scratch), then the timed ones; the brackets' means are reported, and per
queried column (three a codon, one a column of the link query).  The counts of the last call are checked against the invariant: the
classes at each column add up to the count matrix the step tallied.

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
from trueconsense_amd.engine import CDS_DTYPE, CODONS_LDS, LINKS_LDS, Context, DeviceBam, codon_select    # noqa: E402
from trueconsense_amd.io import bamwriter                        # noqa: E402


def codons_add_up(recs, counts):
    """the invariant of include/tcmi.h on every codon"""
    for r in recs:
        j = r["j"].astype(np.int64)
        for k in range(3):
            col = int(r["pos"]) + k
            row = counts[col].astype(np.int64) if col < len(counts) else np.zeros(7, np.int64)
            got = j.sum(tuple(a for a in range(3) if a != k))
            if got[1:6].tolist() != row[1:6].tolist() or got[6] != row[0] - row[1:6].sum():
                return False
    return True


def links_add_up(links, counts):
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
    ref, orfs = sy.make_reference()
    reads = sy.make_reads(ref, a.reads, seed=1)
    L = len(ref)
    cds = np.array([(o["start"] - 1, o["end"], 1 if o["strand"] == "+" else -1, 0) for o in orfs], CDS_DTYPE)
    out = {"reads": a.reads, "positions": L, "reps": a.reps, "frames": len(cds), "lds_capacity_codons": CODONS_LDS}
    with tempfile.TemporaryDirectory() as tmp, Context(0) as ctx:
        path = os.path.join(tmp, "f.bam")
        bamwriter.write_bam_fast(path, reads["pos"], reads["flag"], reads["seq"].reshape(a.reads, -1), 150, "MN908947.3", L, level=6)
        d = DeviceBam(path).to_device(ctx)
        ctx.set_variants(ref, min_af="0.03")                     # (the step lists the table's records)
        rs = ctx.bamfile_step(d, L, 30, True, want_counts=False)[0]
        records = ctx.step_variants()
        rs.free()
        ctx.set_variants()
        table_cols = np.unique(records["pos"].astype(np.int64))
        c0 = codon_select(records, cds)
        both = np.unique(np.concatenate([c0, c0 + 1]))
        out.update(table_columns=len(table_cols), table_codons=len(c0))
        assert len(c0) >= 1 and len(table_cols) * 2 <= LINKS_LDS, (len(c0), len(table_cols))
        # the other route on the same codons: a table of more codons than are staged is cut, a shorter one padded with codons behind every read
        if len(c0) > CODONS_LDS:
            other = ("staged_codons", c0[:CODONS_LDS])
        else:
            other = ("memory_codons", np.concatenate([c0, L + 1024 + 3 * np.arange(CODONS_LDS + 1 - len(c0), dtype=np.int64)]))
        queries = (("table_codons", "codon", c0), (other[0], "codon", other[1]), ("two_frames", "codon", both), ("table_links_k2", "link", table_cols))
        for key, kind, cols in queries:
            wall = 0.0
            for rep in range(a.reps + 2):                        # (two untimed: the arena, the code objects, the scratch)
                if rep == 2:
                    ctx.sync()
                    ctx.profile(True)
                last = rep == a.reps + 1
                rs, _, _, _, counts = ctx.bamfile_step(d, L, 30, True, want_counts=last)
                t0 = time.perf_counter()
                got = ctx.codon_counts(rs, cols) if kind == "codon" else ctx.link_counts(rs, cols, 2)
                if rep >= 2:
                    wall += time.perf_counter() - t0
                rs.free()
            t, c = ctx.profile_get(_ffi.K_LINK_COUNTS)
            ctx.profile(False)
            assert c == a.reps, (c, a.reps)
            assert codons_add_up(got, counts) if kind == "codon" else links_add_up(got, counts), "the counts do not add up to the count matrix the step tallied"
            n_cols = 3 * len(cols) if kind == "codon" else len(cols)
            counted = int(got["j"].astype(np.int64).sum())
            out[key] = {"queried": len(cols), "queried_columns": n_cols, "staged": len(cols) <= CODONS_LDS if kind == "codon" else True,
                        "wall_ms_per_call": round(wall / a.reps * 1e3, 4), "kernel_ms_per_file": round(t / a.reps, 5),
                        "kernel_us_per_queried_column": round(t / a.reps / n_cols * 1e3, 4), "records_counted": counted}
            if kind == "codon":
                out[key]["ins_inside"] = int(got["ins_inside"].sum())
            print("%-15s: %d %s (%d columns); wall %.3f ms per call; kernel %.4f ms (%d brackets), %.3f us per queried column; %d records counted "
                  "(adds up to the step's matrix)" % (key, len(cols), "codons" if kind == "codon" else "columns x 2 neighbours", n_cols, wall / a.reps * 1e3,
                                                      t / a.reps, c, t / a.reps / n_cols * 1e3, counted))
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
