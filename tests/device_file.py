"""A BAM file onto the device under settings, and buffers between guards for what a call writes back: the packers' names, the one
upload under a primer table, a base-quality floor and a read filter (the context is back at its defaults afterwards), the device
decoder against zlib, and sentinel-filled host and device buffers.  No tests in here; importing this opens no device (torch is
imported where a device buffer is made)."""
import contextlib
import gzip
import struct

import numpy as np

from oracle import c_oracle
from trueconsense_amd import engine

PACKERS = ("one_sync", "several_kernels")
NONE = (0, 0, 0)                                                                # the read filter that filters nothing
PKF_EVENT_OVF = 8                                                               # the one-sync packer's "more events than room" in one_sync_last_decline_flags


@contextlib.contextmanager
def uploaded(ctx, path, primers=(), q=0, f=NONE, slack=0, one_sync=1, blocks=None, how=None, events_may_overflow=False):
    """the file as a device-decoded read set built under the table, the floor and the filter; the context is back at its defaults
    while the read set is in use (it must remember what it was built under).
    how: a packer of PACKERS by name, and then the route is asserted: that packer built the read set (rs.route).  The one-sync packer
    sizes its event array for max(2^20, records / 2) events and hands a file beyond that to the several-kernel path (PKF_EVENT_OVF;
    tests/test_pack_capacities.py): events_may_overflow admits that one decline and no other, and rs.route says what happened."""
    if how is not None:
        one_sync = int(how == "one_sync")
    d = engine.DeviceBam(path)
    try:
        t0, d0 = ctx.stat("one_sync_taken"), ctx.stat("one_sync_declined")
        try:
            ctx.set_option("one_sync", one_sync)
            ctx.set_read_filter(*f)
            ctx.set_min_base_quality(q)
            ctx.set_primers(primers, slack)
            rs = ctx.upload_bamfile(d, blocks)
        finally:
            ctx.set_option("one_sync", 1)
            ctx.set_read_filter()
            ctx.set_min_base_quality()
            ctx.set_primers()
        try:
            if how is not None:
                taken, declined = ctx.stat("one_sync_taken") - t0, ctx.stat("one_sync_declined") - d0
                flags = ctx.stat("one_sync_last_decline_flags")
                if how == "one_sync" and events_may_overflow and not taken:
                    assert declined == 1 and flags == PKF_EVENT_OVF, (declined, flags)
                else:
                    assert (taken, declined) == (int(how == "one_sync"), 0), (how, taken, declined, flags)
                rs.route = "one_sync" if taken else "several_kernels"
            yield rs
        finally:
            rs.free()
    finally:
        d.close()


def through(ctx, how, path, primers, n_pos, q=0, f=NONE, slack=0):
    """the file under the table (and floor q, filter f) on one packer -> (counts, n_piled, max_end, the read set's table size, its
    masked reads)"""
    with uploaded(ctx, path, primers, q, f, slack, how=how) as rs:
        return ctx.step(rs, n_pos, 0, True)[3], rs.n_piled, rs.max_end, rs.primers, rs.primer_masked_reads


# ---- the device decoder against zlib -----------------------------------------------------------------------------------------------------
def host_stream_and_records(path):
    """zlib (gzip.decompress walks every member) + a Python walk of the block_size chain."""
    raw = gzip.decompress(open(path, "rb").read())
    l_text = struct.unpack_from("<i", raw, 4)[0]
    o = 8 + l_text
    n_ref = struct.unpack_from("<i", raw, o)[0]
    o += 4
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", raw, o)[0]
        o += 4 + l_name + 4
    rec = []
    while o < len(raw):
        rec.append(o)
        o += 4 + struct.unpack_from("<i", raw, o)[0]
    return np.frombuffer(raw, np.uint8), np.array(rec, np.uint64)


def check_decode(ctx, path):
    want_stream, want_rec = host_stream_and_records(path)
    d = engine.DeviceBam(path)
    assert d.inflated_bytes == len(want_stream), (d.inflated_bytes, len(want_stream))
    stream, rec = d.decode_to_host(ctx)
    assert np.array_equal(stream, want_stream), np.argwhere(stream != want_stream)[:5]
    assert np.array_equal(rec, want_rec), (len(rec), len(want_rec), np.argwhere(rec[:len(want_rec)] != want_rec[:len(rec)])[:5])
    return d


def check_counts(ctx, path, L):
    reads = c_oracle.read_bam(path)
    want = c_oracle.tally(reads, L)
    d = engine.DeviceBam(path)
    rs = ctx.upload_bamfile(d)
    assert rs.n_reads == reads["n_reads"], (rs.n_reads, reads["n_reads"])
    got = ctx.step(rs, L, 30, True)[3]
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    rs.free()
    d.close()


# ---- buffers between guards ----------------------------------------------------------------------------------------------------------------
GUARD = 64


def sentinel(n, dtype=np.int32, salt=0):
    """distinct, far from any count: int32 words at or above 2^30, bytes at or above 0x80"""
    k = np.arange(n, dtype=np.int64) + salt
    if dtype == np.uint8:
        return (0x80 | (k * 37 + 11) % 128).astype(np.uint8)
    return (0x40000000 | (k * 2654435761) % 0x3FFFFFFF).astype(np.int32)


class Guarded:
    """`n` items of `dtype` between two guards inside one torch buffer, `lead` items into it (lead: one int32 word for a pointer
    that is 4 mod 8, one byte for an odd address); body = what the items hold before the call (default: sentinel too)"""

    def __init__(self, n, dtype=np.int32, lead=0, body=None, salt=0):
        import torch
        self.n, self.lo = n, GUARD + lead
        self.init = sentinel(self.lo + n + GUARD, dtype, salt)
        if body is not None:
            self.init[self.lo:self.lo + n] = np.asarray(body, dtype).reshape(-1)
        self.t = torch.from_numpy(self.init.copy()).to("cuda")
        torch.cuda.synchronize()                                # torch's stream is not the context's
        item = self.init.itemsize
        assert self.t.data_ptr() % 64 == 0, self.t.data_ptr()
        self.ptr = self.t.data_ptr() + item * self.lo
        assert self.ptr % 8 == (4 * lead if dtype == np.int32 else lead) % 8, (self.ptr, lead)

    def read(self):
        """-> the body; both guards (and the lead) must hold the sentinel word for word"""
        a = self.t.cpu().numpy()
        assert np.array_equal(a[:self.lo], self.init[:self.lo]), "the guard in front was written"
        assert np.array_equal(a[self.lo + self.n:], self.init[self.lo + self.n:]), "the guard behind was written"
        return a[self.lo:self.lo + self.n]

    def untouched(self):
        return np.array_equal(self.read(), self.init[self.lo:self.lo + self.n])


class Matrix(Guarded):
    """int32 [7][ld] at `off` words past an 8-byte boundary"""

    def __init__(self, L, ld, off, fill=None):
        super().__init__(7 * ld, np.int32, off, fill)
        self.L, self.ld, self.off = L, ld, off
        self.before = self.init[self.lo:self.lo + 7 * ld].reshape(7, ld).copy()

    def check(self, want, zero, what=()):
        """want: int32 [L, 7] rows.  zero: the call cleared the matrix first (padding 0), else it added to what was there."""
        got = self.read().reshape(7, self.ld)
        L = self.L
        exp = np.zeros_like(self.before) if zero else self.before.copy()
        exp[:, :L] += np.ascontiguousarray(want, np.int32).T
        what = (L, self.ld, self.off, zero) + tuple(what)
        bad = np.argwhere(got[:, :L] != exp[:, :L])
        assert len(bad) == 0, (what, "planes", len(bad), bad[:6].tolist(), got[:, :L][tuple(bad[:6].T)].tolist(), exp[:, :L][tuple(bad[:6].T)].tolist())
        assert np.array_equal(got[:, L:], exp[:, L:]), (what, "padding", np.argwhere(got[:, L:] != exp[:, L:])[:6].tolist())
