"""What --mate-overlap costs in the kernels behind the decoder: a synthetic PAIRED file — 400-bp amplicons every 300 bp on the
bench's reference, 2 x 250: the first mate on the amplicon's first 250 columns, the second on its last 250, so every pair shares 100
columns; unique names of nine digits; per-base qualities drawn from 2..41 — `--reps` times through the one-sync packer and the plane
tally with the setting off, on, and on together with the ARTIC-like primer table and a floor, IN THE SAME RUN, timed with the library's
own event brackets (tcmi_profile_get):

    mate_join       hipMemsetAsync of the table + mate_build_kernel + mate_probe_kernel
    pack_classify   pk_index
    pack            pk_place + pk_pack            (setting, floor or table: pk_place_bq + pk_pack behind the memset of the drop plane)
    tally           tally_planes_kernel           (setting, floor or table: tally_planes_drop_kernel)

and, on the same file in the same session, amplicon_reads_kernel's one pass over the same records' fixed fields — the reference for a
kernel that also reads every name and touches a table.  The kept tokens and the join's counters of every configuration are checked
against numpy's count of the same rule.  Prints one line per configuration."""
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

LEN, AMPLICON, STEP, FIRST_AT, PRIMER, NAME = 250, 400, 300, 30, 24, 9
BRACKETS = (("mate_join", _ffi.K_MATE_JOIN), ("pack_classify", _ffi.K_PACK_CLASSIFY), ("pack", _ffi.K_PACK), ("tally", _ffi.K_TALLY))


def artic_like(ref_len):
    out = []
    for s in range(FIRST_AT, ref_len - AMPLICON, STEP):
        out += [(s, s + PRIMER, False), (s + AMPLICON - PRIMER, s + AMPLICON, True)]
    return out


def paired(n, ref_len, seed=1):
    """-> dict(pos, next_pos, flag, name, base [n, LEN] nibbles, qual [n, LEN]) sorted by pos: n // 2 pairs spread over the amplicons"""
    rng = np.random.default_rng(seed)
    starts = np.arange(FIRST_AT, ref_len - AMPLICON, STEP)
    amp = np.sort(rng.integers(0, len(starts), n // 2))
    p1 = starts[amp].astype(np.int64)
    p2 = p1 + AMPLICON - LEN
    pos, npos = np.concatenate([p1, p2]), np.concatenate([p2, p1])
    flag = np.concatenate([np.full(n // 2, 99), np.full(n // 2, 147)])
    name = np.concatenate([np.arange(n // 2), np.arange(n // 2)])
    order = np.argsort(pos, kind="stable")
    return dict(pos=pos[order].astype(np.int32), next_pos=npos[order].astype(np.int32), flag=flag[order].astype(np.uint16), name=name[order],
                base=np.array([1, 8, 2, 4], np.uint8)[rng.integers(0, 4, (len(pos), LEN))], qual=rng.integers(2, 42, (len(pos), LEN), dtype=np.uint8))


def write(path, rd, ref_name, ref_len):
    """the records as a BAM file, whole records per BGZF block (bamwriter.write_bam_fast's layout, with names and mate fields)"""
    n, nb = len(rd["pos"]), LEN // 2
    rec_len = 32 + NAME + 1 + 4 + nb + LEN
    rec = np.zeros((n, 4 + rec_len), np.uint8)

    def put(col, arr, dt):
        a = np.ascontiguousarray(arr, dt).view(np.uint8).reshape(n, -1)
        rec[:, col:col + a.shape[1]] = a
    put(0, np.full(n, rec_len), "<i4")
    put(8, rd["pos"], "<i4")
    rec[:, 12], rec[:, 13] = NAME + 1, 60
    put(14, np.full(n, 4681), "<u2")
    put(16, np.full(n, 1), "<u2")
    put(18, rd["flag"], "<u2")
    put(20, np.full(n, LEN), "<u4")
    put(28, rd["next_pos"], "<i4")
    for k in range(NAME):
        rec[:, 36 + NAME - 1 - k] = 48 + (rd["name"] // 10 ** k) % 10
    put(36 + NAME + 1, np.full(n, LEN << 4), "<u4")
    s0 = 36 + NAME + 1 + 4
    rec[:, s0:s0 + nb] = (rd["base"][:, 0::2] << 4) | rd["base"][:, 1::2]
    rec[:, s0 + nb:s0 + nb + LEN] = rd["qual"]
    text = ("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:%s\tLN:%d\n" % (ref_name, ref_len)).encode()
    nm = ref_name.encode() + b"\0"
    head = b"BAM\1" + np.int32(len(text)).tobytes() + text + np.int32(1).tobytes() + np.int32(len(nm)).tobytes() + nm + np.int32(ref_len).tobytes()
    per = max(1, 0xFF00 // (4 + rec_len))
    with open(path, "wb") as fh:
        fh.write(bamwriter._bgzf_block(head, 6))
        flat, step = rec.reshape(-1), per * (4 + rec_len)
        for o in range(0, flat.size, step):
            fh.write(bamwriter._bgzf_block(flat[o:o + step].tobytes(), 6))
        fh.write(bamwriter._EOF)


def kept_tokens(rd, primers, q, mate):
    """numpy's count of the rule: the second mate of every pair loses its first 100 columns"""
    p = rd["pos"].astype(np.int64)
    last = p + LEN - 1
    head_end, tail_start = p.copy(), last + 1
    for s, e, rev in primers:
        if rev:
            m = (s <= last) & (last < e)
            tail_start[m] = np.minimum(tail_start[m], s)
        else:
            m = (s <= p) & (p < e)
            head_end[m] = np.maximum(head_end[m], e)
    clip = np.where(mate & (rd["flag"] == 147), np.maximum(0, rd["next_pos"].astype(np.int64) + LEN - p), 0)
    col = p[:, None] + np.arange(LEN)[None, :]
    keep = (col >= np.maximum(head_end, p + clip)[:, None]) & (col < tail_start[:, None]) & (rd["qual"] >= q)
    return int(keep.sum()), clip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--q", type=int, default=20, help="the floor of the configuration that has one")
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    ref, _ = sy.make_reference()
    rd = paired(a.reads, len(ref))
    n = len(rd["pos"])
    primers = artic_like(len(ref))
    starts = np.arange(FIRST_AT, len(ref) - AMPLICON, STEP)
    amps4 = [(s, s + PRIMER, s + AMPLICON - PRIMER, s + AMPLICON) for s in starts]
    with tempfile.TemporaryDirectory() as tmp, Context(0) as ctx:
        path = os.path.join(tmp, "f.bam")
        write(path, rd, "MN908947.3", len(ref))
        d = DeviceBam(path).to_device(ctx)
        for name, mate, prim, q in (("off", False, [], 0), ("on", True, [], 0), ("on + table + floor", True, primers, a.q)):
            ctx.set_mate_overlap(mate)
            ctx.set_min_base_quality(q)
            ctx.set_primers(prim)
            for rep in range(a.reps + 2):                        # (two untimed: the arena, the code objects)
                if rep == 2:
                    ctx.profile(True)
                t0 = ctx.stat("one_sync_taken")
                rs = ctx.upload_bamfile(d)
                assert ctx.stat("one_sync_taken") == t0 + 1 and rs.n_piled == n, (rs.n_piled, n)
                counts = ctx.step(rs, max(len(ref), rs.max_end), 30, True, want_counts=True)[3]
                stats = dict(rs.mate_overlap)
                if rep < a.reps + 1:
                    rs.free()
            ms = {nm: ctx.profile_get(k) for nm, k in BRACKETS}
            ctx.profile(False)
            want, clip = kept_tokens(rd, prim, q, mate)
            kept = int(counts[:, 0].sum())
            assert kept == want, (name, kept, want)
            assert stats == dict(on=int(mate), pairs=n // 2 if mate else 0, clipped_reads=int((clip > 0).sum()), clipped_columns=int(clip.sum()), ambiguous=0), stats
            print("%-18s: %d pairs, %d reads clipped, %d of %d tokens kept; per file: %s" % (
                name, stats["pairs"], stats["clipped_reads"], kept, rd["qual"].size,
                ", ".join("%s %.3f ms (%d brackets)" % (k, t / max(1, a.reps), c) for k, (t, c) in ms.items())))
            if name == "off":                                    # the reference pass over the same records, the stream still resident
                ctx.profile(True)
                for _ in range(a.reps):
                    ar = ctx.amplicon_reads(rs, amps4, 5)
                t, c = ctx.profile_get(_ffi.K_AMPLICON_READS)
                ctx.profile(False)
                assert int(ar["reads"].sum()) == n
                print("%-18s: amplicon_reads_kernel over the same %d records: %.3f ms per call (%d brackets)" % ("", n, t / max(1, c), c))
            rs.free()
        ctx.set_mate_overlap(False)
        ctx.set_min_base_quality(0)
        ctx.set_primers()
        d.close()


if __name__ == "__main__":
    main()
