"""The device-matrix ABI at a caller's strides: tcmi_tally_dev, tcmi_call_dev, tcmi_counts_upload and tcmi_counts_download take any
4-byte aligned device pointer and any leading dimension ld >= L (include/tcmi.h); the library's own routes only ever pass ld rounded up to 256 on a
pointer fresh from the allocator.  Here the matrix lies inside one torch int32 buffer

    [ guard | off | plane 0: L counts, ld - L padding | ... | plane 6 | guard ]        guard = 64 words, off in {0, 1}

filled with a sentinel pattern, and after EVERY call all of it is read back: the seven planes are the expectation, the padding is
zero (zero = 1: the memset covers it) or what it was (zero = 0), both guards and the off word hold the sentinel word for word.

What decides the kernel's path (tally_planes.hip, tcmi_launch_tally_fast): pair_ok = (ld % 2 == 0) && (d_counts % 8 == 0).  torch
hands out pointers aligned to far more than 8 bytes (asserted), the guard is 256 bytes, so
    ld even, off 0   64-bit adds over two adjacent positions (odd L: the last column has no neighbour, `two == false`)
    ld odd           pair_ok == 0 because ld % 2 == 1: the one-position epilogue of tally_planes_body.h, for every chunk
    off 1            pair_ok == 0 because the pointer is 4 mod 8: the same epilogue
    ld == L          a store one past L would land in the next plane, not in padding
Every L below comes with ld in {L, L + 1, L rounded up to even, L rounded up to 256} and off in {0, 1}.

Which kernels run: read sets from flat arrays under the default options (bit-plane kernel + tail blocks), with balance_chunks = 0 and
stage_cap = 1 (the default balancing gives a few thousand reads chunks of 64 reads, one stage each; this setting gives chunks of
several stages, and several chunks — asserted through tcmi_readset_sets), tally_variant = 1 (CIGAR-walk kernel), project_reads = 0
(both into one matrix); read sets the device decoded from a BAM file through the one-sync packer and the several-kernel packer,
without a floor and under set_min_base_quality(13) (tally_planes_drop_kernel), with reads of 520 - 700 positions
(tally_stream_kernel).  A read set is in the caller's hands only after tcmi_readset_from_bamfile has read the packer's totals back,
so the launch form that leaves them on the device (FastArgs::dev_counts, inside tcmi_bamfile_step) cannot meet a caller's ld."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import c_oracle
from tests import call_rows
from tests import fuzz_reads as fz
from tests import read_specs as rsp
from tests import synth_small as ss
from tests.device_file import PACKERS, Guarded, Matrix
from trueconsense_amd import _ffi, engine
from trueconsense_amd.io import bamwriter

pytestmark = pytest.mark.gpu

LS = (1, 2, 7, 8, 9, 255, 256, 257, 1001, 1536)
OPTIONS = {"tally_variant": 0, "project_reads": 1, "balance_chunks": 1, "stage_cap": 0, "device_pack": 1}      # a context's defaults


def geometries(L):
    return [(ld, off) for ld in sorted({L, L + 1, L + (L & 1), (L + 255) // 256 * 256}) for off in (0, 1)]


def prefill(L, ld, seed):
    """known counts below 2^20 for a whole [7][ld] matrix, padding included"""
    return np.random.default_rng(seed).integers(0, 1 << 20, (7, ld)).astype(np.int32)


@pytest.fixture(scope="module")
def ctx():
    with engine.Context(0) as c:
        yield c


class options:
    """context options for a block, the defaults afterwards"""

    def __init__(self, ctx, **kw):
        self.ctx, self.kw = ctx, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.ctx.set_option(k, OPTIONS[k])


def sets(rs):
    """-> (aligned reads, aligned chunks, general reads)"""
    v = [C.c_int64(0) for _ in range(3)]
    _ffi.check(_ffi.lib().tcmi_readset_sets(rs.handle, *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


# ------------------------------------------------------------------------------------------------------------------------ read sets
def _split(rng, total, parts):
    """`parts` positive integers that sum to `total` (total >= parts)"""
    cuts = np.sort(rng.choice(np.arange(1, total), parts - 1, replace=False)) if parts > 1 else np.zeros(0, np.int64)
    return [int(v) for v in np.diff(np.concatenate([[0], cuts, [total]]))]


@functools.lru_cache(maxsize=None)
def specs_for(L, n_plain, long_reads=False):
    """Reads inside [0, L), sorted by position -> (specs, indices of the plain `M` reads without an odd base).
      * n_plain `M` reads of up to 150 bases that start inside a window of 41 positions: a pile a few thousand deep
      * 240 reads with an insertion, a deletion, a ref-skip, a deletion followed by an insertion, or soft clips, and 1 % IUPAC codes /
        '=' among all bases: OTHER, X and I event words for the tail blocks, which also take the class-less tokens out of column A
      * a read that starts at 0, reads that end exactly on L - 1 (plain, one base long, behind a deletion, with an insertion as the
        last operation: an I event on L - 1)
      * long_reads: spans of 520, 600 and 700 positions with an insertion and a deletion, where L has room for them
    L that is no multiple of 8 puts the last chunk's 8-position grid past L: the epilogue's `gp >= a.L` decides there."""
    rng = np.random.default_rng(7000 + L)
    ref = "".join("ACGT"[int(k)] for k in rng.integers(0, 4, L))
    out = []

    def add(pos, cig, **kw):
        assert pos >= 0 and pos + fz._span(cig) <= L and all(n > 0 for n, _ in cig), (pos, cig, L)
        out.append(fz._read(rng, ref, pos, cig, 16 if rng.random() < 0.5 else 0, "r%d" % len(out), **kw))
        out[-1]["mapq"] = 60

    top = min(150, L)
    w0 = (L - top) // 2
    for _ in range(n_plain):
        ln = int(rng.integers((top + 1) // 2, top + 1))
        add(int(rng.integers(w0, min(w0 + 40, L - ln) + 1)), [(ln, "M")])
    for k in range(240):
        span = int(rng.integers(min(3, L), top + 1))
        pos = int(rng.integers(0, L - span + 1))
        shape = "IDNXS"[k % 5] if span >= 3 else "M"
        if shape == "I":
            a, b = _split(rng, span, 2)
            cig = [(a, "M"), (int(rng.integers(1, 5)), "I"), (b, "M")]
        elif shape in "DN":
            a, gap, b = _split(rng, span, 3)
            cig = [(a, "M"), (gap, shape), (b, "M")]
        elif shape == "X":                                                       # "*+..": the deletion's last column counts I, not X
            a, gap, b = _split(rng, span, 3)
            cig = [(a, "M"), (gap, "D"), (2, "I"), (b, "M")]
        elif shape == "S":
            cig = [(3, "S"), (span, "M"), (2, "S")]
        else:
            cig = [(span, "M")]
        add(pos, cig)
    add(0, [(min(L, 37), "M")])
    add(L - min(L, 41), [(min(L, 41), "M")])
    add(L - 1, [(1, "M")])
    if L >= 3:
        add(L - 3, [(1, "M"), (1, "D"), (1, "M")])
    if L >= 2:
        add(L - 2, [(2, "M"), (3, "I")])
    if long_reads:
        for span in (520, 600, 700):
            if span + 40 <= L:
                a = int(rng.integers(100, 250))
                add(int(rng.integers(0, L - span + 1)), [(a, "M"), (3, "I"), (120, "M"), (7, "D"), (span - a - 127, "M")])
    order = sorted(range(len(out)), key=lambda i: out[i]["pos"])
    specs = [out[i] for i in order]
    plain = [k for k, r in enumerate(specs) if r["cigar"].endswith("M") and r["cigar"][:-1].isdigit() and set(r["seq"]) <= set("ACGT")]
    return specs, plain


@functools.lru_cache(maxsize=None)
def flat(L):
    """-> (arrays, oracle counts, the plain reads' indices): the flat-array read set of L"""
    specs, plain = specs_for(L, 3000)
    rd = rsp.arrays(specs)
    assert c_oracle.extent(rd, 0) <= L
    want = c_oracle.tally(rd, L)
    want.setflags(write=False)
    return rd, want, plain


def take(rd, idx):
    """the reads idx (ascending) of a dict of flat arrays as a dict of its own: position, flag, CIGAR and SEQ"""
    co, so = rd["cigar_off"].astype(np.int64), rd["seq_off"].astype(np.int64)
    cig = [rd["cigar"][co[i]:co[i + 1]] for i in idx]
    seq = [rd["seq"][so[i]:so[i + 1]] for i in idx]
    idx = np.asarray(idx, np.int64)
    return {"n_reads": len(idx), "pos": rd["pos"][idx].copy(), "flag": rd["flag"][idx].copy(), "l_qseq": rd["l_qseq"][idx].copy(),
            "cigar_off": np.concatenate([[0], np.cumsum([len(c) for c in cig])]).astype(np.uint64), "cigar": np.concatenate(cig).astype(np.uint32),
            "seq_off": np.concatenate([[0], np.cumsum([len(s) for s in seq])]).astype(np.uint64), "seq": np.concatenate(seq).astype(np.uint8)}


def numpy_tally(rd, L):
    """reads of one `M` operation over A / C / G / T only -> int32 [L, 7], by neither oracle"""
    P, N = [], []
    for i in range(int(rd["n_reads"])):
        n = int(rd["cigar"][int(rd["cigar_off"][i])]) >> 4
        assert n == int(rd["l_qseq"][i]) and int(rd["cigar_off"][i + 1]) - int(rd["cigar_off"][i]) == 1
        b = rd["seq"][int(rd["seq_off"][i]):int(rd["seq_off"][i + 1])]
        N.append(np.stack([b >> 4, b & 15], 1).reshape(-1)[:n])
        P.append(int(rd["pos"][i]) + np.arange(n))
    P, N = np.concatenate(P), np.concatenate(N)
    out = np.zeros((L, 7), np.int32)
    np.add.at(out[:, 0], P, 1)
    for nibble, col in ((1, 1), (8, 2), (2, 3), (4, 4)):                         # BAM codes A C G T -> columns A, T, C, G
        np.add.at(out[:, col], P[N == nibble], 1)
    return out


def tally_into(ctx, rs, L, ld, off, want, what, accumulate_too=True):
    """zero = 1 into a matrix of sentinels, then zero = 0 onto known counts: the four assertions of the module docstring, twice"""
    m = Matrix(L, ld, off)
    ctx.tally_dev(rs, L, ld, m.ptr, zero=True)
    ctx.sync()
    m.check(want, True, what)
    if accumulate_too:
        m = Matrix(L, ld, off, prefill(L, ld, 31 * ld + off))
        ctx.tally_dev(rs, L, ld, m.ptr, zero=False)
        ctx.sync()
        m.check(want, False, what)


# ------------------------------------------------------------------------------------------------------------------------ 1. tally
@pytest.mark.parametrize("L", LS)
def test_tally_from_flat_arrays_at_every_geometry(ctx, L):
    rd, want, _ = flat(L)
    assert want[0, 0] > 0 and want[L - 1, 0] >= 3 and (L < 3 or want[:, 5].sum() > 0) and (L < 2 or want[L - 1, 6] > 0)
    assert want[:, 0].max() > 2000 and (want[:, 0] > want[:, 1:6].sum(1)).any()
    indels = any(set("IDN") & set(r["cigar"]) for r in specs_for(L, 3000)[0])
    assert indels == (L >= 2)
    for name, opt in (("default", {}), ("stages", dict(balance_chunks=0, stage_cap=1)), ("host_packer", dict(device_pack=0)),
                      ("cigar_walk", dict(tally_variant=1)), ("both_kernels", dict(project_reads=0))):
        with options(ctx, **opt):
            rs = ctx.upload(rd)
            try:
                aligned, chunks, general = sets(rs)
                assert rs.packed_on_device == (name in ("default", "stages")) and rs.max_end == L and aligned + general >= rs.n_piled > 3000, name
                if name == "cigar_walk":
                    assert aligned == 0 and general == rs.n_piled
                elif name == "both_kernels":
                    assert (general > 0) == indels and (general > 100 or L < 7) and aligned > 3000, (general, aligned)
                else:
                    assert general == 0 and (chunks >= 2 or (name == "stages" and L < 255)), (name, chunks)
                    # no stage holds more than TCMI_P_SUB = 512 reads: chunks that average more have several
                    assert name != "stages" or aligned / chunks > 512, (aligned, chunks)
                for ld, off in geometries(L):
                    tally_into(ctx, rs, L, ld, off, want, (name,), accumulate_too=name in ("default", "cigar_walk"))
            finally:
                rs.free()


@pytest.mark.parametrize("L", (9, 257, 1536))
def test_plain_reads_against_a_numpy_tally(ctx, L):
    """the one comparison that depends on neither oracle: `M` reads over A / C / G / T, counted with np.add.at per base class"""
    rd, want_all, plain = flat(L)
    sub = take(rd, plain)
    # (a base is an IUPAC code or '=' with probability 0.01, so a third of the 3 000 reads of 75 - 150 bases have none: about 1 000,
    # with a standard deviation below 30; the short reads of L = 9 nearly all)
    assert sub["n_reads"] > 800
    want = numpy_tally(sub, L)
    assert np.array_equal(want[:, 1:5].sum(1), want[:, 0]) and want[:, 0].sum() == sub["l_qseq"].sum() and (want <= want_all).all()
    rs = ctx.upload(sub)
    try:
        assert sets(rs)[2] == 0
        for ld, off in geometries(L):
            tally_into(ctx, rs, L, ld, off, want, ("numpy",))
    finally:
        rs.free()


@functools.lru_cache(maxsize=None)
def bam_reads(L):
    specs, _ = specs_for(L, 500, True)
    rd = rsp.arrays(specs)
    n_long = sum(1 for r in specs if sum(n for op, n in ss.parse_cigar(r["cigar"]) if op in (0, 2, 3, 7, 8)) > 512)
    want = {0: c_oracle.tally(rd, L), 13: rsp.oracle_counts(rd, 13, L)}
    return rd, want, n_long


@pytest.mark.parametrize("L", LS)
def test_tally_from_a_device_decoded_bam_at_every_geometry(ctx, tmp_path, L):
    rd, want, n_long = bam_reads(L)
    assert n_long == (3 if L >= 1001 else 0)
    assert 0 < want[13][:, 0].sum() < want[0][:, 0].sum() and (L < 9 or want[13][:, 5:].sum() < want[0][:, 5:].sum())
    path = str(tmp_path / "m.bam")
    bamwriter.write_bam(path, rd, ref_len=L, block=4096)
    for how in PACKERS:
        for q in (0, 13):
            try:
                ctx.set_option("one_sync", int(how == "one_sync"))
                ctx.set_min_base_quality(q)
                d = engine.DeviceBam(path)
                t0 = ctx.stat("one_sync_taken")
                rs = ctx.upload_bamfile(d)
                try:
                    assert ctx.stat("one_sync_taken") - t0 == int(how == "one_sync"), (how, ctx.stat("one_sync_last_decline_flags"))
                    aligned, chunks, general = sets(rs)
                    assert (rs.min_base_quality, rs.max_end, general, rs.n_piled - aligned) == (q, L, 0, n_long), (how, q)
                    for ld, off in geometries(L):
                        tally_into(ctx, rs, L, ld, off, want[q], (how, q), accumulate_too=ld % 2 == 1)
                finally:
                    rs.free()
                    d.close()
            finally:
                ctx.set_option("one_sync", 1)
                ctx.set_min_base_quality()


@pytest.mark.parametrize("L,ld", ((1001, 1001), (1536, 1537), (257, 257)))
def test_two_read_ranges_add_up_at_an_odd_ld(ctx, L, ld):
    """one read set split into two ranges of reads, tallied in either order with zero = 0: the whole, on top of what was there"""
    rd, want, _ = flat(L)
    n = int(rd["n_reads"])
    cut = n // 3
    parts = [ctx.upload(take(rd, range(0, cut))), ctx.upload(take(rd, range(cut, n)))]
    try:
        for off in (0, 1):
            for order in ((0, 1), (1, 0)):
                m = Matrix(L, ld, off, prefill(L, ld, 5 + off))
                for k in order:
                    ctx.tally_dev(parts[k], L, ld, m.ptr, zero=False)
                ctx.sync()
                m.check(want, False, ("ranges", order))
                m = Matrix(L, ld, off)                                           # ... and the first of the two clears the matrix
                for j, k in enumerate(order):
                    ctx.tally_dev(parts[k], L, ld, m.ptr, zero=j == 0)
                ctx.sync()
                m.check(want, True, ("ranges, zero first", order))
    finally:
        for rs in parts:
            rs.free()


def test_refusals_write_nothing(ctx):
    """ld < L, L <= 0 and null pointers: TCMI_E_ARG from all four functions, and every buffer as it was"""
    lib = _ffi.lib()
    L, ld = 257, 259
    rd, _, _ = flat(L)
    rs = ctx.upload(rd)
    m = Matrix(L, ld, 1)
    rows = np.ascontiguousarray(call_rows.lattice()[:L])
    host = np.full((L, 7), -7, np.int32)
    rec = [Guarded(L, np.uint8, 1, salt=k) for k in range(3)]
    ev, evc = Guarded(512), Guarded(2)
    vp = C.c_void_p
    P, A, F = (vp(r.ptr) for r in rec)
    try:
        calls = []
        for bad_L, bad_ld in ((L, L - 1), (0, ld), (-3, ld), (L, 0)):
            calls += [lib.tcmi_tally_dev(ctx.handle, rs.handle, bad_L, bad_ld, vp(m.ptr), 1),
                      lib.tcmi_counts_upload(ctx.handle, _ffi.ptr(rows), bad_L, bad_ld, vp(m.ptr)),
                      lib.tcmi_counts_download(ctx.handle, vp(m.ptr), bad_L, bad_ld, _ffi.ptr(host)),
                      lib.tcmi_call_dev(ctx.handle, vp(m.ptr), bad_L, bad_ld, 0, 1, P, A, F, vp(ev.ptr), vp(evc.ptr))]
        calls += [lib.tcmi_tally_dev(None, rs.handle, L, ld, vp(m.ptr), 1), lib.tcmi_tally_dev(ctx.handle, None, L, ld, vp(m.ptr), 1),
                  lib.tcmi_tally_dev(ctx.handle, rs.handle, L, ld, None, 1),
                  lib.tcmi_counts_upload(None, _ffi.ptr(rows), L, ld, vp(m.ptr)), lib.tcmi_counts_upload(ctx.handle, None, L, ld, vp(m.ptr)),
                  lib.tcmi_counts_upload(ctx.handle, _ffi.ptr(rows), L, ld, None),
                  lib.tcmi_counts_download(None, vp(m.ptr), L, ld, _ffi.ptr(host)), lib.tcmi_counts_download(ctx.handle, None, L, ld, _ffi.ptr(host)),
                  lib.tcmi_counts_download(ctx.handle, vp(m.ptr), L, ld, None),
                  lib.tcmi_call_dev(None, vp(m.ptr), L, ld, 0, 1, P, A, F, None, None), lib.tcmi_call_dev(ctx.handle, None, L, ld, 0, 1, P, A, F, None, None),
                  lib.tcmi_call_dev(ctx.handle, vp(m.ptr), L, ld, 0, 1, None, A, F, None, None), lib.tcmi_call_dev(ctx.handle, vp(m.ptr), L, ld, 0, 1, P, None, F, None, None),
                  lib.tcmi_call_dev(ctx.handle, vp(m.ptr), L, ld, 0, 1, P, A, None, None, None),
                  # int32 buffers that are not aligned to 4 bytes
                  lib.tcmi_tally_dev(ctx.handle, rs.handle, L, ld, vp(m.ptr + 2), 1), lib.tcmi_call_dev(ctx.handle, vp(m.ptr + 1), L, ld, 0, 1, P, A, F, None, None),
                  lib.tcmi_call_dev(ctx.handle, vp(m.ptr), L, ld, 0, 1, P, A, F, vp(ev.ptr + 2), vp(evc.ptr)),
                  lib.tcmi_call_dev(ctx.handle, vp(m.ptr), L, ld, 0, 1, P, A, F, vp(ev.ptr), vp(evc.ptr + 3)),
                  # the two event buffers come together or not at all
                  lib.tcmi_call_dev(ctx.handle, vp(m.ptr), L, ld, 0, 1, P, A, F, vp(ev.ptr), None),
                  lib.tcmi_call_dev(ctx.handle, vp(m.ptr), L, ld, 0, 1, P, A, F, None, vp(evc.ptr))]
        assert calls == [_ffi.E_ARG] * len(calls), calls
        ctx.sync()
        assert m.untouched() and all(r.untouched() for r in rec) and ev.untouched() and evc.untouched() and (host == -7).all()
    finally:
        rs.free()


# ------------------------------------------------------------------------------------------------------------------------ 2. copies, call
def call_matrix(L):
    """rows of the threshold lattice, spread over all coverages: every flag of the call comes up, events among them"""
    la = call_rows.lattice()
    m = np.ascontiguousarray(la[(np.arange(L, dtype=np.int64) * 7919 + 13) % len(la)])
    m[::11, 0] = 0                                                               # coverage 0 (TCMI_F_COVZERO) ...
    m[::11, 6] = 0
    m[5::17, 5] = m[5::17, 0]                                                    # ... and X on top (TCMI_F_PRIMX)
    return m


@pytest.mark.parametrize("L", (1, 255, 256, 257, 1001))
def test_upload_download_and_call_at_a_callers_strides(ctx, L):
    lib = _ffi.lib()
    counts = call_matrix(L)
    odd = L + 2 - L % 2
    nblk = (L + 255) // 256
    n_events = 0
    for ld, off in ((odd, 0), (odd, 1), (L, 0), (L, 1)):
        m = Matrix(L, ld, off)
        _ffi.check(lib.tcmi_counts_upload(ctx.handle, _ffi.ptr(counts), L, ld, C.c_void_p(m.ptr)), ctx.handle)
        m.check(counts, True, ("upload",))                                       # the padding is written as zero
        back = np.full((L, 7), -1, np.int32)
        _ffi.check(lib.tcmi_counts_download(ctx.handle, C.c_void_p(m.ptr), L, ld, _ffi.ptr(back)), ctx.handle)
        assert np.array_equal(back, counts), (ld, off)
        for mincov in (0, 30):
            for amb in (True, False):
                wp, wa, wf = c_oracle.call(counts, mincov, amb)
                want_ev = np.nonzero(wf & 14)[0]
                for with_events in (False, True):
                    rec = [Guarded(L + 19, np.uint8, 1, salt=k) for k in range(3)]      # each output starts at an odd byte address
                    ev, evc = Guarded(nblk * 256, salt=3), Guarded(nblk, salt=4)
                    _ffi.check(lib.tcmi_call_dev(ctx.handle, C.c_void_p(m.ptr), L, ld, mincov, int(amb), *[C.c_void_p(r.ptr) for r in rec],
                                                 C.c_void_p(ev.ptr) if with_events else None, C.c_void_p(evc.ptr) if with_events else None), ctx.handle)
                    ctx.sync()
                    what = (L, ld, off, mincov, amb, with_events)
                    for r, w in zip(rec, (wp, wa, wf)):
                        got = r.read()
                        assert np.array_equal(got[:L], w), (what, np.nonzero(got[:L] != w)[0][:6].tolist())
                        assert np.array_equal(got[L:], r.init[r.lo + L:r.lo + r.n]), what      # bytes [L, ...) as they were
                    if with_events:
                        e, n = ev.read(), evc.read()
                        assert (n >= 0).all() and (n <= 256).all(), what
                        got_ev = np.concatenate([e[b * 256:b * 256 + n[b]] for b in range(nblk)])
                        assert np.array_equal(got_ev, want_ev) and int(n.sum()) == len(want_ev), what
                        n_events += len(want_ev)
                    else:
                        assert ev.untouched() and evc.untouched()
                    m.check(counts, True, what)                                  # clean = 0: the call leaves the counts alone
    assert n_events > 0


@pytest.mark.parametrize("L,ld,off", ((1001, 1001, 0), (1001, 1003, 1), (257, 259, 0)))
def test_tally_then_call_on_one_odd_matrix(ctx, L, ld, off):
    """the route of an outside caller: tcmi_tally_dev, then tcmi_call_dev on the same planes; no wait of the host in between"""
    rd, want, _ = flat(L)
    rs = ctx.upload(rd)
    try:
        for mincov, amb in ((30, True), (0, False)):
            m = Matrix(L, ld, off)
            rec = [Guarded(L, np.uint8, 1, salt=k) for k in range(3)]
            ctx.tally_dev(rs, L, ld, m.ptr, zero=True)
            ctx.call_dev(m.ptr, L, ld, mincov, amb, *[r.ptr for r in rec])
            ctx.sync()
            m.check(want, True, ("chained",))
            for r, w in zip(rec, c_oracle.call(want, mincov, amb)):
                assert np.array_equal(r.read(), w), (mincov, amb)
    finally:
        rs.free()
