"""What the primer mask (--primers) costs in the kernels behind the decoder: the bench's file (1 M 150-bp reads on 29 903
positions) with per-base qualities drawn from 2..41, under an ARTIC-like table — 400-bp amplicons every 300 bp, 24-bp primers:
'+' [s, s + 24) and '-' [s + 376, s + 400) for s = 30, 330, ... —, `--reps` times through the one-sync packer and the plane tally
with no table, the table alone, Q = 20 alone and both, IN THE SAME RUN, timed with the library's own event brackets
(tcmi_profile_get):

    pack_classify   pk_index
    pack            pk_place + pk_pack            (floor or table: pk_place_bq + pk_pack, the memset of the drop plane in front of
                                                   them, and under a table pk_mask_long behind pk_place_bq)
    tally           tally_planes_kernel           (floor or table: tally_planes_drop_kernel)

The kept tokens of every configuration are checked against numpy's count of the same rule (every read is 150M: column = POS + i).
Prints one line per configuration: primers, masked reads, tokens kept, and the mean milliseconds per file of each bracket."""
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


def artic_like(ref_len, step=300, amplicon=400, primer=24, first=30):
    out = []
    for s in range(first, ref_len - amplicon, step):
        out += [(s, s + primer, False), (s + amplicon - primer, s + amplicon, True)]
    return out


def kept_mask(pos, primers, read_len=150):
    """bool [n, read_len]: the tokens the table keeps (brute force per primer: a few hundred passes over the reads' positions)"""
    p = np.asarray(pos, np.int64)
    q = p + read_len - 1
    head_end, tail_start = p.copy(), q + 1
    hit_t = np.zeros(len(p), bool)
    for s, e, rev in primers:
        if not rev:
            m = (s <= p) & (p < e)
            head_end[m] = np.maximum(head_end[m], e)
        else:
            m = (s <= q) & (q < e)
            tail_start[m] = np.where(hit_t[m], np.minimum(tail_start[m], s), s)
            hit_t |= m
    col = p[:, None] + np.arange(read_len)[None, :]
    return (col >= head_end[:, None]) & (col < tail_start[:, None]), int(((head_end > p) | (tail_start <= q)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--q", type=int, default=20, help="the floor of the two configurations that have one")
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    ref, _ = sy.make_reference()
    reads = sy.make_reads(ref, a.reads, seed=1)
    qual = np.random.default_rng(7).integers(2, 42, (a.reads, 150), dtype=np.uint8)
    primers = artic_like(len(ref))
    keep, n_masked = kept_mask(reads["pos"], primers)
    with tempfile.TemporaryDirectory() as tmp, Context(0) as ctx:
        path = os.path.join(tmp, "f.bam")
        bamwriter.write_bam_fast(path, reads["pos"], reads["flag"], reads["seq"].reshape(a.reads, -1), 150, "MN908947.3", len(ref), level=6, qual=qual)
        d = DeviceBam(path).to_device(ctx)
        for name, prim, q in (("no table", [], 0), ("table alone", primers, 0), ("floor alone", [], a.q), ("table + floor", primers, a.q)):
            ctx.set_min_base_quality(q)
            ctx.set_primers(prim)
            for rep in range(a.reps + 2):                        # (two untimed: the arena, the code objects)
                if rep == 2:
                    ctx.profile(True)
                t0 = ctx.stat("one_sync_taken")
                rs = ctx.upload_bamfile(d)
                assert ctx.stat("one_sync_taken") == t0 + 1 and rs.primers == len(prim) and rs.n_piled == a.reads
                assert rs.primer_masked_reads == (n_masked if prim else 0), (rs.primer_masked_reads, n_masked)
                counts = ctx.step(rs, max(len(ref), rs.max_end), 30, True, want_counts=True)[3]
                rs.free()
            ms = {nm: ctx.profile_get(k) for nm, k in BRACKETS}
            ctx.profile(False)
            kept = int(counts[:, 0].sum())
            want = int(((qual >= q) & (keep if prim else True)).sum())
            assert kept == want, (name, kept, want)
            print("%-13s (%3d primers, min_baseq %2d): %d reads masked, %d of %d tokens kept; per file: %s" % (
                name, len(prim), q, n_masked if prim else 0, kept, qual.size,
                ", ".join("%s %.3f ms (%d launches)" % (n, t / max(1, a.reps), c) for n, (t, c) in ms.items())))
        ctx.set_min_base_quality(0)
        ctx.set_primers()
        d.close()


if __name__ == "__main__":
    main()
