"""What --amplicon-reads (tcmi_readset_amplicon_reads) costs per file: the bench's file (1 M 150-bp reads on 29 903 positions, its
compressed bytes resident in HBM) `--reps` times through tcmi_bamfile_step and, behind each step, through the call on the read set the
step returned, for a tiled scheme of about a hundred amplicons (400 columns, a new one every 300):

    staged   the scheme as it is: table and counters in LDS
    memory   the same amplicons and far-away ones behind them, TCMI_AMPLICON_READS_LDS + 1 in all: table and counters in memory

    amplicon_reads   amplicon_reads_kernel, one hipEvent bracket around its one launch (slot TCMI_K_AMPLICON_READS)
    pk_index         the packer's record pass of THE SAME RUN (slot TCMI_K_PACK_CLASSIFY: below 16 384 BGZF blocks the bracket holds
                     pk_index alone).  Both kernels touch every record's fixed fields and CIGAR once: pk_index is the yardstick for what
                     this pass should cost
    wall             host time of the call itself: the table compiled and sent, the launch, the counters back, one wait

The counts of the last call are checked against a numpy count over the same reads (every read is 150M: p = pos, q = pos + 149) and
the invariant against the read set's piled-up reads.  Prints one line per route and a JSON line."""
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
from trueconsense_amd.engine import AMPLICON_READS_LDS, Context, DeviceBam   # noqa: E402
from trueconsense_amd.io import bamwriter                        # noqa: E402

BRACKETS = (("amplicon_reads", _ffi.K_AMPLICON_READS), ("pk_index", _ffi.K_PACK_CLASSIFY))
FAR = 1 << 24


def scheme(L, length=400, step=300, primer=24):
    return [(s, s + primer, s + length - primer, s + length) for s in range(30, L - length, step)]


def numpy_counts(pos, flag, amps4, slack, read_len=150):
    keep = (flag & 4) == 0
    p = pos[keep].astype(np.int64)
    q = p + read_len - 1
    a4 = np.asarray(amps4, np.int64)
    n = len(a4)
    out = np.zeros((n + 2, 2), np.int64)
    for o in range(0, len(p), 1 << 16):
        pp, qq = p[o:o + (1 << 16), None], q[o:o + (1 << 16), None]
        hit = (a4[None, :, 0] - slack <= pp) & (qq < a4[None, :, 3] + slack)
        k = hit.sum(axis=1)
        who = hit.argmax(axis=1)
        one = k == 1
        out[:n, 0] += np.bincount(who[one], minlength=n)
        full = one & (pp[:, 0] < a4[who, 1]) & (qq[:, 0] >= a4[who, 2])
        out[:n, 1] += np.bincount(who[full], minlength=n)
        out[n, 0] += int((k > 1).sum())
        out[n + 1, 0] += int((k == 0).sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--slack", type=int, default=5)
    a = ap.parse_args()
    ref, _ = sy.make_reference()
    reads = sy.make_reads(ref, a.reads, seed=1)
    L = len(ref)
    amps = scheme(L)
    routes = (("staged", amps), ("memory", amps + [(FAR + 10 * k, FAR + 10 * k + 3, FAR + 10 * k + 5, FAR + 10 * k + 8) for k in range(AMPLICON_READS_LDS + 1 - len(amps))]))
    want = numpy_counts(np.asarray(reads["pos"]), np.asarray(reads["flag"]), amps, a.slack)
    out = {"reads": a.reads, "positions": L, "reps": a.reps, "amplicons": len(amps), "slack": a.slack, "lds_capacity_amplicons": AMPLICON_READS_LDS}
    with tempfile.TemporaryDirectory() as tmp, Context(0) as ctx:
        path = os.path.join(tmp, "f.bam")
        bamwriter.write_bam_fast(path, reads["pos"], reads["flag"], reads["seq"].reshape(a.reads, -1), 150, "MN908947.3", L, level=6)
        d = DeviceBam(path).to_device(ctx)
        for key, use in routes:
            wall = 0.0
            for rep in range(a.reps + 2):                        # (two untimed: the arena, the code objects, the scratch)
                if rep == 2:
                    ctx.sync()
                    ctx.profile(True)
                rs = ctx.bamfile_step(d, L, 30, True, want_counts=False)[0]
                t0 = time.perf_counter()
                got = ctx.amplicon_reads(rs, use, a.slack)
                if rep >= 2:
                    wall += time.perf_counter() - t0
                n_piled = rs.n_piled
                rs.free()
            ms = {name: ctx.profile_get(k) for name, k in BRACKETS}
            ctx.profile(False)
            n = len(amps)
            cnt = np.stack([got["reads"], got["full"]], axis=1)
            assert cnt[:, 0].sum() == n_piled, "the reads do not add up to the read set's kept records"
            assert np.array_equal(cnt[:n], want[:n]) and np.array_equal(cnt[len(use):], want[n:]) and not cnt[n:len(use)].any(), "the counts differ from the numpy count"
            out[key] = {"table_amplicons": len(use), "wall_ms_per_call": round(wall / a.reps * 1e3, 4)}
            for name, (t, c) in ms.items():
                out[key][name + "_ms_per_file"] = round(t / a.reps, 5)
                out[key][name + "_launch_brackets"] = c
            print("amplicon reads %-6s: %d amplicons in the table; wall %.3f ms per call; %s; ambiguous %d, unassigned %d of %d kept (numpy count: equal)" % (
                key, len(use), wall / a.reps * 1e3, ", ".join("%s %.4f ms (%d brackets)" % (nm, t / a.reps, c) for nm, (t, c) in ms.items()),
                cnt[len(use), 0], cnt[len(use) + 1, 0], n_piled))
        d.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
