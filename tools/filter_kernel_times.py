"""What the read filter costs, and saves, in the kernels behind the decoder: the bench's file (1 M 150-bp reads on 29 903 positions) with
MAPQ 0 on a third of its reads, `--reps` times through tcmi_bamfile_step (pk_index, pk_place, pk_pack, the tally) and through the device
insert-token vote on three columns (ins_entries_kernel), with the filter off or on (--min-mapq 20).  Kernel times: run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/filter_kernel_times.py --filter off     (then: on)

and compare the two kernel_stats.csv (profiles/r07a_*).  Prints the records that failed, the reads kept and the wall time per file."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trueconsense_amd import synthetic as sy                     # noqa: E402
from trueconsense_amd.engine import Context, DeviceBam           # noqa: E402
from trueconsense_amd.io import bamwriter                        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filter", choices=("off", "on"), default="off")
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    ref, _ = sy.make_reference()
    reads = sy.make_reads(ref, a.reads, seed=1)
    mapq = np.where(np.random.default_rng(7).random(a.reads) < 1 / 3, 0, 60).astype(np.uint8)
    cols = [len(ref) // 4, len(ref) // 2, 3 * len(ref) // 4]
    with tempfile.TemporaryDirectory() as tmp, Context(0) as ctx:
        path = os.path.join(tmp, "f.bam")
        bamwriter.write_bam_fast(path, reads["pos"], reads["flag"], reads["seq"].reshape(a.reads, -1), 150, "MN908947.3", len(ref), level=6, mapq=mapq)
        d = DeviceBam(path).to_device(ctx)
        if a.filter == "on":
            ctx.set_read_filter(min_mapq=20)
        want = int((mapq < 20).sum()) if a.filter == "on" else 0
        for rep in range(a.reps + 2):                            # (two untimed: the arena, the code objects)
            if rep == 2:
                ctx.sync()
                t0 = time.perf_counter()
            rs = ctx.bamfile_step(d, len(ref), 30, True, want_counts=False)[0]
            toks = ctx.readset_modal_tokens(rs, cols)
            assert rs.filtered == want and rs.n_piled == a.reads - want, (rs.filtered, rs.n_piled, want)
            rs.free()
        dt = time.perf_counter() - t0
        d.close()
    print("filter %s: %d of %d records failed, %d reads kept, %.3f ms per file (step + tokens of %d columns: %s), one_sync_taken %s" %
          (a.filter, want, a.reads, a.reads - want, 1e3 * dt / a.reps, len(cols), [toks[c][1] for c in cols], "yes"))


if __name__ == "__main__":
    main()
