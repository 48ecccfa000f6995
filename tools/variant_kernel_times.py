"""What the variant table (--variant-table; tcmi_ctx_set_variants) costs per file: the bench's file (1 M 150-bp reads on 29 903
positions, its compressed bytes resident in HBM) `--reps` times through tcmi_bamfile_step without the counts on the host — the shape
of a --batch sample — with the setting OFF and ON IN THE SAME RUN:

    wall            host time per file around the whole step (decode, pack, tally, [table,] call, one wait), profiling off
    variants        var_count_kernel + var_scan_kernel + var_emit_kernel, one hipEvent bracket around the three launches
    tally, call     the library's brackets of the kernels on either side, for scale

and what crosses PCIe for the table — 16 bytes a record and the 8-byte total, written by the kernels into pinned memory — against
the 7 * ld * 4 bytes a download of the matrix would take.  The records of the last step are checked against the yardstick
(tests/variant_yardstick.py) over the same file's counts.  Prints one line per setting and a JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                               # noqa: E402
from tests import variant_yardstick as vy                       # noqa: E402
from trueconsense_amd import _ffi                                # noqa: E402
from trueconsense_amd import synthetic as sy                     # noqa: E402
from trueconsense_amd.engine import Context, DeviceBam, min_af_fraction   # noqa: E402
from trueconsense_amd.io import bamwriter                        # noqa: E402

BRACKETS = (("tally", _ffi.K_TALLY), ("variants", _ffi.K_VARIANTS), ("call", _ffi.K_CALL))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--min-af", default="0.03")
    ap.add_argument("--min-alt-depth", type=int, default=1)
    ap.add_argument("--min-depth", type=int, default=10)
    a = ap.parse_args()
    num, den = min_af_fraction(a.min_af)
    ref, _ = sy.make_reference()
    reads = sy.make_reads(ref, a.reads, seed=1)
    L = len(ref)
    out = {"reads": a.reads, "positions": L, "reps": a.reps, "min_af": "%d/%d" % (num, den)}
    with tempfile.TemporaryDirectory() as tmp, Context(0) as ctx:
        path = os.path.join(tmp, "f.bam")
        bamwriter.write_bam_fast(path, reads["pos"], reads["flag"], reads["seq"].reshape(a.reads, -1), 150, "MN908947.3", L, level=6)
        d = DeviceBam(path).to_device(ctx)
        rs, _, _, _, counts = ctx.bamfile_step(d, L, 30, True, want_counts=True)
        rs.free()
        want = vy.as_array(vy.records(counts, ref.encode(), num, den, a.min_alt_depth, a.min_depth))
        ld = (len(counts) + 255) // 256 * 256
        for on in (False, True):
            ctx.set_variants(ref if on else None, a.min_af, a.min_alt_depth, a.min_depth)
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
            key = "on" if on else "off"
            out[key] = {"wall_ms_per_file": round(wall, 4)}
            for name, (t, c) in ms.items():
                out[key][name + "_ms_per_file"] = round(t / a.reps, 5)
                out[key][name + "_launch_brackets"] = c
            line = "variant table %-3s: wall %.3f ms per file; %s" % (key, wall, ", ".join("%s %.4f ms (%d brackets)" % (n, t / a.reps, c) for n, (t, c) in ms.items()))
            if on:
                got = ctx.step_variants()
                assert np.array_equal(got, want), "the step's records differ from the yardstick"
                out[key].update(records_per_file=len(got), pinned_bytes_per_file=16 * len(got) + 8, matrix_download_bytes=7 * ld * 4)
                line += "; %d records = %d bytes into pinned memory against %d for the matrix (yardstick: equal)" % (len(got), 16 * len(got) + 8, 7 * ld * 4)
            else:
                assert ms["variants"][1] == 0, "the setting is off and a table kernel was launched"
            print(line)
        ctx.set_variants(None)
        d.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
