"""What --dedup costs in the kernels behind the decoder, on the file tests/mate_big.py generates (reads of 50M, unique names of nine
digits, every quality 30; default 1 M records, the size tools/mate_overlap_kernel_times.py uses): `--reps` times through the one-sync
packer and the plane tally with --mate-overlap alone, --dedup alone and both, IN THE SAME RUN, timed with the library's own event
brackets (tcmi_profile_get):

    mate_join       the join's table reset + mate_build_kernel + mate_probe_kernel, and under --dedup behind them, in the same bracket,
                    the duplicate table's reset + dup_ends_kernel + dup_build_kernel + dup_mark_kernel
    pack_classify   pk_index
    pack            pk_place_bq + pk_pack behind the memset of the drop plane
    tally           tally_planes_drop_kernel

then two files of forward fragments alone, in the same record layout: every record on ONE key, and as many records spread over
1 400 keys — a lane's work must not grow with its key's templates, so the first may cost more than the second only by what atomics
on one address cost.  The verdicts and counters of every configuration are checked against numpy's count of the same rule
(tests/dedup_big.py).  Prints one line per configuration.

    --rocprof DIR   instead: run this tool (--reps 5) under `rocprofv3 --kernel-trace --stats`, the program after `--`, under a time
                    limit of its own, and print the per-kernel rows of its statistics for the join's and the duplicate rule's kernels"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import dedup_big as db                                # noqa: E402
from tests import mate_big as mb                                 # noqa: E402
from trueconsense_amd import _ffi                                # noqa: E402
from trueconsense_amd.engine import Context, DeviceBam           # noqa: E402

BRACKETS = (("mate_join", _ffi.K_MATE_JOIN), ("pack_classify", _ffi.K_PACK_CLASSIFY), ("pack", _ffi.K_PACK), ("tally", _ffi.K_TALLY))
KERNELS = ("mate_build_kernel", "mate_probe_kernel", "dup_ends_kernel", "dup_build_kernel", "dup_mark_kernel")


def fragments(n, keys, seed=4):
    """n forward fragments in mate_big's record layout on `keys` distinct columns, sorted by pos"""
    rng = np.random.default_rng(seed)
    pos = np.sort(100 + np.arange(n, dtype=np.int64) % keys)
    return dict(pos=pos.astype(np.int32), flag=np.zeros(n, np.uint16), name=np.arange(n, dtype=np.int64), next_pos=np.full(n, -1, np.int32),
                base=mb.NIBBLES[rng.integers(0, 4, (n, mb.LEN))])


def timed(ctx, path, n, reps, mate, dedup, want):
    d = DeviceBam(path).to_device(ctx)
    ctx.set_mate_overlap(mate)
    ctx.set_dedup(dedup)
    try:
        for rep in range(reps + 2):                              # (two untimed: the arena, the code objects)
            if rep == 2:
                ctx.profile(True)
            t0 = ctx.stat("one_sync_taken")
            rs = ctx.upload_bamfile(d)
            assert ctx.stat("one_sync_taken") == t0 + 1 and rs.n_piled == n, (rs.n_piled, n)
            ctx.step(rs, mb.L + 2000, 30, True)
            got = dict(rs.dedup)
            dup = rs.duplicates() if dedup and rep == reps + 1 else None
            rs.free()
        ms = {nm: ctx.profile_get(k) for nm, k in BRACKETS}
        ctx.profile(False)
    finally:
        ctx.set_mate_overlap(False)
        ctx.set_dedup(False)
        d.close()
    if dedup:
        assert got == dict(want[1], on=1) and np.array_equal(dup, want[0]), (got, want[1])
    return got, ", ".join("%s %.3f ms (%d brackets)" % (k, t / max(1, reps), c) for k, (t, c) in ms.items())


def rocprof(out_dir, reads):
    os.makedirs(out_dir, exist_ok=True)
    cmd = ["timeout", "-k", "10", "420", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--",
           sys.executable, os.path.abspath(__file__), "--reps", "5", "--reads", str(reads)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    print(r.stdout[-3000:])
    if r.returncode:
        print(r.stderr[-3000:], file=sys.stderr)
        return r.returncode
    for path in sorted(glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)):
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "")
            if any(k in name for k in KERNELS):
                print("%-22s n = %4s   avg %9.1f   min %9.1f   max %9.1f  (us)" % (
                    [k for k in KERNELS if k in name][0], row.get("Calls"), float(row.get("AverageNs", 0)) / 1e3, float(row.get("MinNs", 0)) / 1e3,
                    float(row.get("MaxNs", 0)) / 1e3))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rocprof", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.rocprof:
        sys.exit(rocprof(a.rocprof, a.reads))
    rd = mb.generate(a.reads)
    n = len(rd["pos"])
    want = db.verdicts(rd)
    with tempfile.TemporaryDirectory() as tmp, Context(0) as ctx:
        path = mb.write(os.path.join(tmp, "f.bam"), rd)
        for name, mate, dedup in (("mate-overlap", True, False), ("dedup", False, True), ("mate-overlap + dedup", True, True)):
            got, line = timed(ctx, path, n, a.reps, mate, dedup, want)
            print("%-22s: %d records, %d templates, %d duplicate records in %d sets; per file: %s" % (
                name, n, got["templates"], got["duplicate_records"], got["duplicate_sets"], line))
        for name, keys in (("dedup, one key", 1), ("dedup, 1 400 keys", 1400)):
            fr = fragments(a.reads, keys)
            path = mb.write(os.path.join(tmp, "k%d.bam" % keys), fr)
            got, line = timed(ctx, path, len(fr["pos"]), a.reps, False, True, db.verdicts(fr))
            print("%-22s: %d records, %d templates, %d duplicate records in %d sets; per file: %s" % (
                name, len(fr["pos"]), got["templates"], got["duplicate_records"], got["duplicate_sets"], line))


if __name__ == "__main__":
    main()
