"""What the amplicon table (--amplicon-table; tcmi_ctx_set_intervals) costs per file: the bench's file (1 M 150-bp reads on 29 903
positions, its compressed bytes resident in HBM) `--reps` times through tcmi_bamfile_step without the counts on the host — the shape
of a --batch sample — with the setting OFF and ON IN THE SAME RUN, for three schemes:

    artic   about 100 amplicons of 400 columns, a new one every 300 (every interval is staged in LDS)
    long    about 12 amplicons of 2 500 columns, a new one every 2 400 (staged too: the capacity is 4 096 columns)
    beyond  the `long` scheme's amplicons stretched to 5 000 columns (past the capacity: the selection reads the plane again from L2)

    wall            host time per file around the whole step (decode, pack, tally, [table,] call, one wait), profiling off
    intervals       interval_stats_kernel, one hipEvent bracket around its one launch
    tally, call     the library's brackets of the kernels on either side, for scale

and what crosses PCIe for the table — 32 bytes an interval, written by the kernel into pinned memory — against the 7 * ld * 4 bytes
a download of the matrix would take.  The records of the last step are checked against the yardstick
(tests/amplicon_yardstick.py) over the same file's counts.  Prints one line per setting and a JSON line.  (The kernel's LDS and
register use are the code object's: `hipcc --offload-arch=gfx950 -O3 --offload-device-only -S csrc/intervals.hip`, the
.group_segment_fixed_size / .vgpr_count / .sgpr_count of its metadata.)"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                               # noqa: E402
from tests import amplicon_yardstick as ay                      # noqa: E402
from trueconsense_amd import _ffi                                # noqa: E402
from trueconsense_amd import synthetic as sy                     # noqa: E402
from trueconsense_amd.engine import INTERVAL_STAGE, Context, DeviceBam   # noqa: E402
from trueconsense_amd.io import bamwriter                        # noqa: E402

BRACKETS = (("tally", _ffi.K_TALLY), ("intervals", _ffi.K_INTERVALS), ("call", _ffi.K_CALL))


def scheme(L, length, step):
    return [(s, min(s + length, L)) for s in range(30, L - length // 2, step)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--min-depth", type=int, default=30)
    a = ap.parse_args()
    ref, _ = sy.make_reference()
    reads = sy.make_reads(ref, a.reads, seed=1)
    L = len(ref)
    schemes = (("off", None), ("artic", scheme(L, 400, 300)), ("long", scheme(L, 2500, 2400)), ("beyond", scheme(L, 5000, 2400)))
    out = {"reads": a.reads, "positions": L, "reps": a.reps, "min_depth": a.min_depth, "staging_capacity_columns": INTERVAL_STAGE}
    with tempfile.TemporaryDirectory() as tmp, Context(0) as ctx:
        path = os.path.join(tmp, "f.bam")
        bamwriter.write_bam_fast(path, reads["pos"], reads["flag"], reads["seq"].reshape(a.reads, -1), 150, "MN908947.3", L, level=6)
        d = DeviceBam(path).to_device(ctx)
        rs, _, _, _, counts = ctx.bamfile_step(d, L, 30, True, want_counts=True)
        rs.free()
        ld = (len(counts) + 255) // 256 * 256
        for key, iv in schemes:
            ctx.set_intervals(iv, a.min_depth)
            wall = None
            for profiled in (False, True):
                ctx.profile(profiled)
                for rep in range(a.reps + 2):                    # (two untimed: the arena, the code objects)
                    if rep == 2:
                        ctx.sync()
                        ctx.profile(profiled)
                        t0 = time.perf_counter()
                    rs = ctx.bamfile_step(d, L, 30, True, want_counts=False)[0]
                    rs.free()
                if not profiled:
                    wall = (time.perf_counter() - t0) / a.reps * 1e3
            ms = {name: ctx.profile_get(k) for name, k in BRACKETS}
            ctx.profile(False)
            out[key] = {"wall_ms_per_file": round(wall, 4)}
            for name, (t, c) in ms.items():
                out[key][name + "_ms_per_file"] = round(t / a.reps, 5)
                out[key][name + "_launch_brackets"] = c
            line = "amplicon table %-6s: wall %.3f ms per file; %s" % (key, wall, ", ".join("%s %.4f ms (%d brackets)" % (n, t / a.reps, c) for n, (t, c) in ms.items()))
            if iv:
                got = ctx.step_intervals()
                want = ay.as_array(ay.records(counts[:, 0], iv, a.min_depth))
                assert np.array_equal(got, want), "the step's records differ from the yardstick"
                out[key].update(intervals=len(iv), columns=int(iv[0][1] - iv[0][0]), pinned_bytes_per_file=32 * len(iv), matrix_download_bytes=7 * ld * 4)
                line += "; %d intervals of %d columns = %d bytes into pinned memory against %d for the matrix (yardstick: equal)" % (
                    len(iv), iv[0][1] - iv[0][0], 32 * len(iv), 7 * ld * 4)
            else:
                assert ms["intervals"][1] == 0, "the setting is off and the table's kernel was launched"
            print(line)
        ctx.set_intervals(None)
        d.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
