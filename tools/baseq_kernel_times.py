"""What the base-quality floor (--min-baseq) costs in the kernels behind the decoder: the bench's file (1 M 150-bp reads on 29 903
positions) with per-base qualities drawn from 2..41 instead of the constant 30, `--reps` times through the one-sync packer and the
plane tally at Q = 0 and at Q = 20 IN THE SAME RUN, timed with the library's own event brackets (tcmi_profile_get):

    pack_classify   pk_index
    pack            pk_place + pk_pack            (Q > 0: pk_place_bq + pk_pack, and the memset of the drop plane in front of them)
    tally           tally_planes_kernel           (Q > 0: tally_planes_drop_kernel)

For pk_place and pk_pack apart, run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/baseq_kernel_times.py --q 20 --only

Prints one line per floor: tokens kept, and the mean milliseconds per file of each bracket."""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trueconsense_amd import _ffi                                # noqa: E402
from trueconsense_amd import synthetic as sy                     # noqa: E402
from trueconsense_amd.engine import Context, DeviceBam           # noqa: E402
from trueconsense_amd.io import bamwriter                        # noqa: E402

BRACKETS = (("pack_classify", _ffi.K_PACK_CLASSIFY), ("pack", _ffi.K_PACK), ("tally", _ffi.K_TALLY))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--q", type=int, default=20, help="the floor compared with 0")
    ap.add_argument("--only", action="store_true", help="run the floor --q alone (for a profiler's per-kernel statistics)")
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    ref, _ = sy.make_reference()
    reads = sy.make_reads(ref, a.reads, seed=1)
    qual = np.random.default_rng(7).integers(2, 42, (a.reads, 150), dtype=np.uint8)
    with tempfile.TemporaryDirectory() as tmp, Context(0) as ctx:
        path = os.path.join(tmp, "f.bam")
        bamwriter.write_bam_fast(path, reads["pos"], reads["flag"], reads["seq"].reshape(a.reads, -1), 150, "MN908947.3", len(ref), level=6, qual=qual)
        d = DeviceBam(path).to_device(ctx)
        for q in ((a.q,) if a.only else (0, a.q)):
            ctx.set_min_base_quality(q)
            for rep in range(a.reps + 2):                        # (two untimed: the arena, the code objects)
                if rep == 2:
                    ctx.profile(True)
                t0 = ctx.stat("one_sync_taken")
                rs = ctx.upload_bamfile(d)
                assert ctx.stat("one_sync_taken") == t0 + 1 and rs.min_base_quality == q and rs.n_piled == a.reads
                counts = ctx.step(rs, max(len(ref), rs.max_end), 30, True, want_counts=True)[3]
                rs.free()
            ms = {name: ctx.profile_get(k) for name, k in BRACKETS}
            ctx.profile(False)
            kept = int(counts[:, 0].sum())
            assert kept == int((qual >= q).sum()), (kept, int((qual >= q).sum()))
            print("min_baseq %3d: %d of %d tokens kept; per file: %s" % (
                q, kept, qual.size, ", ".join("%s %.3f ms (%d launches)" % (n, t / max(1, a.reps), c) for n, (t, c) in ms.items())))
        ctx.set_min_base_quality(0)
        d.close()


if __name__ == "__main__":
    main()
