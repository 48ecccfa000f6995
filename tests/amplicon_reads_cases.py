"""What the tests of the reads-per-amplicon counts share (tests/test_amplicon_reads.py, and the record-stream tests that repeat its cases
at other sizes): tiled and padded schemes, the yardstick's kept records of a BAM parsed on the host, the device call between guards,
and the scheme rows and the text of the command line's file.  No tests in here."""
import ctypes as C

import numpy as np

from tests import amplicon_reads_yardstick as ry
from tests import device_file as dvf
from trueconsense_amd import _ffi, engine

LDS = engine.AMPLICON_READS_LDS
FAR = 1 << 20                           # where the padding amplicons lie: beyond every read of these tests


def tiled(n, first=30, step=300, length=400, primer=24):
    """n amplicons of `length` columns every `step`: neighbours overlap by length - step"""
    return [(first + step * k, first + step * k + primer, first + step * k + length - primer, first + step * k + length) for k in range(n)]


def padded(amps4, n):
    """amps4 and far-away amplicons behind them, n in all: the counts of the first ones must not change"""
    return list(amps4) + [(FAR + 10 * k, FAR + 10 * k + 3, FAR + 10 * k + 5, FAR + 10 * k + 8) for k in range(n - len(amps4))]


def host_columns(path, shift=None, read_filter=None):
    """the yardstick's kept records of the BAM at `path`, parsed on the host"""
    bam = engine.BamFile(path)
    try:
        rd = bam.arrays()
        return ry.kept_columns(rd, shift, read_filter, rd["mapq"])
    finally:
        bam.close()


def device_counts(ctx, rs, amps4, slack):
    """tcmi_readset_amplicon_reads into a host buffer between guards -> int64 [n + 2, 2]"""
    n = len(amps4)
    fs, le, rs_, fe = engine._amps4(amps4)
    G = 64
    buf = dvf.sentinel(2 * G + 4 * (n + 2), np.int32, salt=5).copy()           # (int32 sentinel words: two per int64)
    before = buf.copy()
    rc = _ffi.lib().tcmi_readset_amplicon_reads(ctx.handle, rs.handle, n, _ffi.ptr(fs), _ffi.ptr(le), _ffi.ptr(rs_), _ffi.ptr(fe), int(slack),
                                                C.c_void_p(buf.ctypes.data + 4 * G))
    _ffi.check(rc, ctx.handle)
    assert np.array_equal(buf[:G], before[:G]) and np.array_equal(buf[-G:], before[-G:]), "a guard around the records was written"
    got = buf[G:-G].view(np.int64).reshape(n + 2, 2).copy()
    again = np.stack([ctx.amplicon_reads(rs, amps4, slack)[k] for k in ("reads", "full")], axis=1)
    assert np.array_equal(got, again), (got[got != again][:8].tolist(), again[got != again][:8].tolist())     # the same numbers run after run
    return got


def scheme_rows_for(chrom, amps4, pools=("1", "2")):
    rows = []
    for k, (fs, le, rs_, fe) in enumerate(amps4):
        rows += [(chrom, fs, le, "%s_amp_%d_LEFT" % (chrom, k + 1), pools[k % 2], "+"), (chrom, rs_, fe, "%s_amp_%d_RIGHT" % (chrom, k + 1), pools[k % 2], "-")]
    return rows


def want_text(sample, columns, chrom_amps, slack):
    """the file's text from the yardstick: chrom_amps = [(chrom, [(fs, le, rs, fe)] on the axis)] in the scheme's order"""
    amps4 = [a for _, amps in chrom_amps for a in amps]
    chroms = [c for c, amps in chrom_amps for _ in amps]
    names = ["%s_amp_%d" % (c, k + 1) for c, amps in chrom_amps for k in range(len(amps))]
    pools = [("1", "2")[k % 2] for _, amps in chrom_amps for k in range(len(amps))]
    return ry.text(sample, ry.counts(columns, amps4, slack), chroms, names, pools)
