"""One process per GPU (torch.distributed; backend "nccl" is RCCL over xGMI on ROCm).

Two shard shapes (BASELINE.json configs[3] and [4]):

* many BAMs  — independent objects: rank r takes BAMs r, r+world, ...; NO data-path collective.
* one BAM    — the tally is a commutative integer sum: every rank takes a contiguous range of the FILE's
               BGZF blocks (tally_split_bamfile: it maps the same file, sends only its range's compressed
               bytes to its GPU, decodes and packs the records that start in those blocks there) — or, for
               reads already decoded, a contiguous range of the read arrays (tally_split_bam) —, tallies
               it into a full-length int32 [7][ld] matrix in HBM, and ONE exchange of that matrix
               (837 284 B at L = 29 903) follows: a reduce to the rank that calls and walks
               (reduce_counts), or an all-reduce when every rank wants the whole matrix (allreduce_counts).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._ffi import E_ARG as _ffi_E_ARG
from ._ffi import E_UNSUPPORTED as _ffi_E_UNSUPPORTED
from ._ffi import TcmiError, check, lib
from .engine import (DEFAULT_FLAG_FILTER, DEFAULT_MAX_DEPTH, DEFAULT_MIN_BASE_QUALITY, BamFile, Context, DeviceBam, ReadSet, _grab,
                     _token_buffer, modal_tokens)


def shard_items(n_items, rank, world):
    """Indices of the independent BAMs rank `rank` processes (round-robin)."""
    return list(range(rank, n_items, world))


def read_range(n_reads, rank, world):
    """Contiguous read range [a, b) of rank `rank`; ranges partition [0, n_reads)."""
    base, rem = divmod(int(n_reads), int(world))
    a = rank * base + min(rank, rem)
    return a, a + base + (1 if rank < rem else 0)


def block_range(n_blocks, rank, world):
    """BGZF blocks [first, first + count) of rank `rank`: contiguous, the ranges partition the file.  (Header and end-of-file
    blocks are simply part of some range: they hold no records.)"""
    a, b = read_range(n_blocks, rank, world)
    return a, b - a


def shard_reads(reads, rank, world):
    """The rank's contiguous slice of a dict of flat read arrays (tcmi_reads layout); a read that
    straddles a boundary simply belongs to one range."""
    n = int(reads["n_reads"])
    a, b = read_range(n, rank, world)
    co, so = np.asarray(reads["cigar_off"]), np.asarray(reads["seq_off"])
    out = {"n_reads": b - a, "pos": reads["pos"][a:b], "flag": reads["flag"][a:b], "l_qseq": reads["l_qseq"][a:b],
           "cigar_off": (co[a:b + 1] - co[a]).astype(np.uint64), "cigar": reads["cigar"][int(co[a]):int(co[b])],
           "seq_off": (so[a:b + 1] - so[a]).astype(np.uint64), "seq": reads["seq"][int(so[a]):int(so[b])]}
    if reads.get("tid") is not None:
        out["tid"] = reads["tid"][a:b]
    if reads.get("qual") is not None:
        lq = np.asarray(reads["l_qseq"], np.int64)
        q0 = int(lq[:a].sum())
        out["qual"] = reads["qual"][q0:q0 + int(lq[a:b].sum())]
    return out


def allreduce_counts(t, group=None):
    """In-place sum of the [7][ld] int32 matrix over the ranks.  A CUDA tensor goes through the
    process group's own backend (RCCL when it is "nccl"); under gloo it is staged through the host."""
    import torch
    import torch.distributed as dist
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return t
    if t.is_cuda and dist.get_backend(group) != "nccl":
        h = t.cpu()
        dist.all_reduce(h, op=dist.ReduceOp.SUM, group=group)
        t.copy_(h)
    else:
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return t


def reduce_counts(t, dst=0, group=None):
    """Sum of the [7][ld] int32 matrix over the ranks, delivered to rank `dst` only (the call kernel and the walk
    run on one GPU, so nobody else needs the whole matrix: SURVEY §8-e).  RCCL reduce under "nccl"; staged
    through the host under gloo.  The other ranks' tensors are left as they were."""
    import torch.distributed as dist
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return t
    if t.is_cuda and dist.get_backend(group) != "nccl":
        h = t.cpu()
        dist.reduce(h, dst=dst, op=dist.ReduceOp.SUM, group=group)
        if dist.get_rank(group) == dst:
            t.copy_(h)
    else:
        dist.reduce(t, dst=dst, op=dist.ReduceOp.SUM, group=group)
    return t


def tally_split_bam(reads, L, rank, world, device=0, group=None, tally_fn=None):
    """BASELINE configs[4]: one BAM over `world` ranks -> the whole int32 [L,7] matrix on every rank.

    tally_fn(shard, L) -> int [L,7] replaces the GPU tally (tests on CPU-only boxes pass the
    oracle's; the product path leaves it None and needs an MI355X)."""
    import torch
    shard = shard_reads(reads, rank, world)
    L = int(L)
    if tally_fn is not None:
        part = torch.from_numpy(np.ascontiguousarray(np.asarray(tally_fn(shard, L)).T.astype(np.int32)))   # [7][L]
        allreduce_counts(part, group)
        return np.ascontiguousarray(part.numpy().T)
    ld = (L + 255) // 256 * 256
    torch.cuda.set_device(device)
    t = torch.zeros((7, ld), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream                 # tally and collective on torch's stream
    ctx = Context(device, stream=stream)
    rs = ctx.upload(shard)
    check(lib().tcmi_tally_dev(ctx.handle, rs.handle, L, ld, C.c_void_p(t.data_ptr()), 0), ctx.handle)
    allreduce_counts(t, group)
    counts = np.ascontiguousarray(t[:, :L].T.cpu().numpy())
    rs.free()
    ctx.close()
    return counts


def check_range_anchors(ranges, inflated_bytes):
    """ranges: per rank, in rank order, (first_block, n_blocks, first, next) — engine.ReadSet.range_anchors of its block range
    (tcmi_readset_range_anchors).  A range in the middle of the file starts at the first offset its first block finds PLAUSIBLE for an
    alignment record; that offset is a record start for sure only if the range in front ends there (by induction from the header,
    whose end the first range starts at).  -> None, or what does not join (a message): then no rank's result is to be trusted and
    the file takes the host reader."""
    expect = None                                                   # where the next record must start, once a range has fixed it
    for r, (first_block, n_blocks, first, nxt) in enumerate(ranges):
        if n_blocks <= 0:
            continue
        if first_block != 0 and first >= 0:
            if expect is not None and first != expect:
                return "rank %d's block range starts a record at stream offset %d, the range in front ends its last record at %d" % (r, first, expect)
            if expect is None and r > 0 and any(n > 0 for _, n, _, _ in ranges[:r]):
                return "rank %d's block range starts a record at stream offset %d, but no range in front says where its last record ends" % (r, first)
        if nxt >= 0:
            expect = nxt
    if expect is not None and expect != inflated_bytes:
        return "the last alignment record ends at stream offset %d, the file's stream at %d" % (expect, inflated_bytes)
    return None


def tally_split_bamfile(path, L, rank, world, device=0, group=None, ctx=None, to_root=False, rules=None):
    """BASELINE configs[4] from ONE FILE: every rank opens the same BAM, decodes on its GPU only the alignment records that start
    in its contiguous range of BGZF blocks (engine.Context.upload_bamfile(blocks=...): inflate, record index, pack), tallies
    them into a full-length int32 [7][ld] matrix and the matrices are summed — to every rank, or (to_root) to rank 0 only.
    -> int [L,7] (None on the other ranks with to_root).  No rank ever holds the file's reads, decoded or not.
    rules: the ReadRules set on the rank's context (Context.set_rules), every rank the same ones; None leaves what the context has."""
    import torch
    L = int(L)
    ld = (L + 255) // 256 * 256
    torch.cuda.set_device(device)
    own = ctx is None
    if own:
        ctx = Context(device, stream=torch.cuda.current_stream().cuda_stream)         # tally and collective on torch's stream
    ctx.set_rules(rules)
    d = DeviceBam(path)
    try:
        import torch.distributed as dist
        first, count = block_range(d.n_blocks, rank, world)
        # A range can be refused on ONE rank only (a record chain that does not close from a false start, a record longer than a block
        # at the range's end, a read the packer does not take): the ranks agree BEFORE anybody enters the collective — else the others
        # wait in it forever — and then all raise.
        rs, err = None, None
        try:
            rs = ctx.upload_bamfile(d, blocks=(first, count))
            if rs.max_end > L:
                err = (_ffi_E_ARG, "L=%d is smaller than the reads' extent %d" % (L, rs.max_end))
        except TcmiError as e:
            err = (e.code, str(e))
        if dist.is_initialized() and dist.get_world_size(group) > 1:
            allv = [None] * dist.get_world_size(group)
            dist.all_gather_object(allv, (err, (first, count) + (rs.range_anchors if rs is not None else (-1, -1))), group=group)
            err = next((v[0] for v in allv if v[0]), None)
            if not err:                                             # ... and the ranges must join into ONE chain of records
                why = check_range_anchors([v[1] for v in allv], d.inflated_bytes)
                if why:
                    err = (_ffi_E_UNSUPPORTED, "%s: %s: host reader" % (path, why))
        if err:
            if rs is not None:
                rs.free()
            raise TcmiError(err[0], "tally_split_bamfile: a rank could not decode its block range: %s" % err[1])
        t = torch.zeros((7, ld), dtype=torch.int32, device="cuda")
        if rs.n_piled:
            check(lib().tcmi_tally_dev(ctx.handle, rs.handle, L, ld, C.c_void_p(t.data_ptr()), 0), ctx.handle)
        if to_root:
            reduce_counts(t, 0, group)
        else:
            allreduce_counts(t, group)
        mine = not to_root or not dist.is_initialized() or dist.get_rank(group) == 0
        counts = np.ascontiguousarray(t[:, :L].T.cpu().numpy()) if mine else None
        rs.free()
    finally:
        d.close()
        if own:
            ctx.close()
    return counts


# --------------------------------------------------------------------------------------------- configs[4], all the way to the consensus
def _entries_of_readset(ctx, rs, positions):
    """This rank's entries of the candidate columns (tcmi_readset_ins_entries) -> (bytes, ent_off list, long-insertion text bytes)."""
    pos = np.ascontiguousarray(positions, np.int64)
    n = len(pos)
    off = np.zeros(n + 1, np.int64)
    cap, lcap = 1 << 14, 1 << 16
    while True:
        ents = np.zeros(cap * 48, np.uint8)
        text = np.zeros(lcap, np.uint8)
        used = C.c_int64(0)
        rc = lib().tcmi_readset_ins_entries(ctx.handle, rs.handle, n, pos.ctypes.data_as(C.c_void_p), DEFAULT_FLAG_FILTER, 1, ents.ctypes.data_as(C.c_void_p),
                                            cap, off.ctypes.data_as(C.c_void_p), text.ctypes.data_as(C.c_void_p), lcap, C.byref(used))
        if rc != 0 and (off[n] > cap or used.value > lcap):        # (the buffers were too small: the call says what is needed)
            cap, lcap = max(cap, int(off[n]) + 16), max(lcap, used.value + 16)
            continue
        check(rc, ctx.handle)
        return ents[:int(off[n]) * 48].tobytes(), off.tolist(), text[:used.value].tobytes()


def _vote(positions, pieces):
    """Rank 0: per column the ranks' pieces concatenated in rank order (= file order), voted on as tcmi_readset_modal_tokens votes
    (tcmi_modal_from_entries: pysam's default filters, Events.py:66).  -> ({pos: token or None}, status flags)."""
    n = len(positions)
    text = b"".join(p[2] for p in pieces)
    base = np.cumsum([0] + [len(p[2]) for p in pieces])
    cols, off = [], [0]
    arrays = []
    for r, (ents, eoff, _) in enumerate(pieces):
        a = np.frombuffer(ents, np.uint8).copy()
        if len(a) and base[r]:
            check(lib().tcmi_ins_entries_rebase(a.ctypes.data_as(C.c_void_p), len(a) // 48, int(base[r])))
        arrays.append(a)
    for k in range(n):
        for r, (_, eoff, _) in enumerate(pieces):
            cols.append(arrays[r][eoff[k] * 48:eoff[k + 1] * 48])
        off.append(off[-1] + sum(p[1][k + 1] - p[1][k] for p in pieces))
    allents = np.ascontiguousarray(np.concatenate(cols)) if cols and sum(len(c) for c in cols) else np.zeros(48, np.uint8)
    off = np.ascontiguousarray(off, np.int64)
    toff, cnt, st = np.zeros(n + 1, np.int64), np.zeros(n, np.int64), C.c_int32(0)
    tb = np.frombuffer(text, np.uint8) if text else np.zeros(1, np.uint8)
    buf = _token_buffer(lambda buf, cap: lib().tcmi_modal_from_entries(
        n, allents.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), DEFAULT_MIN_BASE_QUALITY, DEFAULT_MAX_DEPTH, 1, tb.ctypes.data_as(C.c_void_p),
        len(text), C.cast(buf, C.c_void_p), cap, toff.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), C.byref(st)))
    return {int(positions[k]): (buf.raw[toff[k]:toff[k + 1]].decode("ascii") if cnt[k] else None) for k in range(n)}, st.value


class _Tokens:
    """What Events.inserts_from_flags asks a `bam` for (a token per candidate column)."""
    def __init__(self, toks):
        self.toks = toks

    def modal_token(self, pos):
        return self.toks.get(pos)


def rccl_communicator(rank, world, group=None):
    """An RCCL communicator of this process's own (include/tcmi_rccl.h) for tcmi_split_step's C hook: rank 0 draws the id, the bytes
    travel through the process group that is already up (any backend) — or nowhere at world 1.  -> (comm handle, _ffi.RcclUser);
    destroy with _ffi.rccl_lib().tcmi_rccl_comm_destroy(comm).  The current HIP device must be the rank's."""
    from . import _ffi
    # The ranks move in step: every rank enters the broadcast of the id and the gather of the verdicts whatever happened to it before
    # (a hook library that does not load, an id that cannot be drawn, a communicator that cannot be made) — and then all raise, or none.
    r, err = None, None
    try:
        r = _ffi.rccl_lib()
    except (ImportError, OSError) as e:
        err = str(e)
    ident = C.create_string_buffer(_ffi.RCCL_ID_BYTES)
    if rank == 0 and err is None and r.tcmi_rccl_unique_id(ident):
        err = (r.tcmi_rccl_last_error() or b"").decode()
    multi = world > 1
    if multi:
        import torch.distributed as dist
        box = [(err, ident.raw) if rank == 0 else None]
        dist.broadcast_object_list(box, src=0, group=group)
        root_err, raw = box[0]
        if root_err is not None:
            raise RuntimeError("rccl_communicator: rank 0 could not draw the id: %s" % root_err)
        ident = C.create_string_buffer(raw, _ffi.RCCL_ID_BYTES)
    elif err is not None:
        raise RuntimeError("rccl_communicator: %s" % err)
    comm = C.c_void_p()
    if err is None and r.tcmi_rccl_comm_init(int(world), int(rank), ident, C.byref(comm)):
        err = (r.tcmi_rccl_last_error() or b"").decode()
        comm = C.c_void_p()
    if multi:
        allv = [None] * world
        dist.all_gather_object(allv, err, group=group)
        bad = [(k, v) for k, v in enumerate(allv) if v is not None]
        if bad:
            if comm:
                r.tcmi_rccl_comm_destroy(comm)
            raise RuntimeError("rccl_communicator: rank %d: %s" % bad[0])
    elif err is not None:
        raise RuntimeError("rccl_communicator: %s" % err)
    return comm, _ffi.RcclUser(comm, 0)


def split_reduce_hook(rank, world, group=None, rccl=True):
    """The exchange tcmi_split_step's hook runs on for this job -> (comm or None, rccl_user or None, what it is, in words).
    rccl: the C hook tcmi_rccl_reduce (libtcmi_rccl.so: ncclReduce queued on the context's stream) on a communicator of this job's own —
    at ONE rank too, so that the collective itself runs wherever the step runs.  All ranks get the same answer (rccl_communicator's
    ranks raise together): where the communicator cannot be made — no libtcmi_rccl.so, several ranks on one GPU — every rank falls
    back to torch.distributed's reduce on the process group that is already up.  Destroy `comm` with split_reduce_hook_close."""
    if rccl and os.environ.get("TCMI_SPLIT_HOOK", "rccl") == "rccl":
        try:
            comm, user = rccl_communicator(rank, world, group)
            return comm, user, "tcmi_rccl_reduce: ncclReduce on the context's stream, %d-rank communicator" % world
        except RuntimeError as e:
            return None, None, "torch.distributed reduce (an RCCL communicator of its own could not be made: %s)" % e
    return None, None, "torch.distributed reduce"


def split_reduce_hook_close(comm):
    if comm:
        from . import _ffi
        _ffi.rccl_lib().tcmi_rccl_comm_destroy(comm)


def split_words(L, world):
    """-> (ld, n_words): the leading dimension of the [7][ld] count planes and the int32 words of tcmi_split_step's buffer — the planes
    and, behind them, the range table and the failure word (TCMI_SPLIT_TAIL_WORDS(world))."""
    ld = (int(L) + 255) // 256 * 256
    return ld, 7 * ld + 6 * int(world) + 1


def _split_step(ctx, d, rank, world, L, ld, t, mincov, include_ambig, fn, user):
    """Rank `rank`'s tcmi_split_step over its block range of DeviceBam d, into the int32 tensor t (split_words), the exchange through
    fn(user, ...).  -> (rc, the rank's ReadSet, the root's (plain, alt, flags)): (rc, None, None) when the step failed — the caller
    words the failure (tcmi_last_error) —, no record planes on a rank other than 0 (the call kernel runs on the root)."""
    first, count = block_range(d.n_blocks, rank, world)
    h, p_, a_, f_ = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    rc = lib().tcmi_split_step(ctx.handle, d.handle, first, count, L, ld, C.c_void_p(t.data_ptr()), int(mincov), int(bool(include_ambig)), fn, user,
                               int(rank), int(world), C.byref(h), C.byref(p_), C.byref(a_), C.byref(f_))
    if rc:
        return rc, None, None
    return rc, ReadSet(ctx, h, None), tuple(_grab(vp, np.uint8, L) for vp in (p_, a_, f_)) if rank == 0 else None


def _tokens_for(path, cand, pieces, host_sweep, rules):
    """The candidate columns' modal tokens -> {pos: token or None}: the vote on the ranks' pieces; a sweep of the whole file on the
    host (tcmi_bam_load + tcmi_modal_tokens) when the caller says so (a rank could not collect its entries) or the vote meets a pair
    of mates that only such a sweep resolves (status bit 2); the sweep under the read filter of `rules` (the caller's ReadRules or None)."""
    toks, st = ({}, 2) if host_sweep else _vote(cand, pieces)
    if st & 2:
        bam = BamFile(path, read_filter=rules.read_filter if rules is not None else None)
        try:
            toks = {p: tk for p, (tk, _) in modal_tokens(bam, cand).items()}
        finally:
            bam.close()
    return toks


def _fasta_from_records(name, mincov, gff_rows, plain, alt, flags, toks):
    """The root's walk (Sequences.py:168-322) over the call records, inserts from the voted tokens -> FASTA text."""
    from .Events import inserts_from_flags
    from .Sequences import consensus_from_records
    _, inserts = inserts_from_flags(flags, _Tokens(toks))
    cons, _ = consensus_from_records(plain, alt, flags, {i: dict(r) for i, r in enumerate(gff_rows)}, inserts, True)
    return ">%s mincov=%d\n%s\n" % (name, int(mincov), cons)


def _agree(err, group, multi):
    """Every rank's err = (code, text) or None -> the first rank's that has one, or None: the same answer on every rank, so that all
    raise or all go on into the next collective together.  Not multi: err itself."""
    if not multi:
        return err
    import torch.distributed as dist
    allv = [None] * dist.get_world_size(group)
    dist.all_gather_object(allv, err, group=group)
    return next((v for v in allv if v), None)


def _sum_to_root(what, count, group, multi):
    """A count behind the step: count() -> this rank's contiguous 2-D integer array (or TcmiError); nobody enters the reduce unless
    everybody has counts — else every rank raises TcmiError "consensus_split_bamfile: <what>: ..." with the first failing rank's code
    and words —; then one sum to rank 0 over the group (on the device under "nccl", on the host otherwise; nothing to sum for an empty
    array).  -> the array: on rank 0 the sum."""
    mine, err = None, None
    try:
        mine = count()
    except TcmiError as e:
        err = (e.code, str(e))
    err = _agree(err, group, multi)
    if err is not None:
        raise TcmiError(err[0], "consensus_split_bamfile: %s: %s" % (what, err[1]))
    if multi and mine.size:
        import torch
        import torch.distributed as dist
        tr = torch.from_numpy(mine).cuda() if dist.get_backend(group) == "nccl" else torch.from_numpy(mine)
        dist.reduce(tr, dst=0, op=dist.ReduceOp.SUM, group=group)
        mine = tr.cpu().numpy()
    return mine


def _root_columns(ctx, counts_root, variants, root, group, multi):
    """Rank 0 lists the variant table's records from the reduced matrix (variants: the keyword arguments of Context.variants) and
    everybody gets their distinct columns -> (records, None on the other ranks; int64 columns, ascending)."""
    import torch.distributed as dist
    recs = ctx.variants(counts_root, **variants) if root else None
    cols = [np.unique(recs["pos"].astype(np.int64)).tolist() if root else None]
    if multi:
        dist.broadcast_object_list(cols, src=0, group=group)
    return recs, np.asarray(cols[0], np.int64)


def consensus_split_bamfile(path, ref_len, gff_rows, mincov, include_ambig=True, name="S", rank=0, world=1, device=0, group=None,
                            step_fn=None, entries_fn=None, return_parts=False, rccl_user=None, ctx=None, dbam=None, timings=None, rules=None,
                            amplicon_reads=None, variant_strand=None, variant_links=None):
    """BASELINE configs[4] all the way: ONE BAM file over `world` ranks -> its consensus FASTA text on rank 0 (None on the others).
    What the ranks jointly replace is the reference's single pile-up pass (indexing.py:96-100), its insert candidates' region
    pile-ups (Events.py:47-82) and the walk (Sequences.py:168-322):

      1. every rank decodes, packs and tallies the records that start in ITS contiguous range of the file's BGZF blocks and the count
         matrices are summed to rank 0 (tcmi_split_step: the step in C, the reduce a hook — with `rccl_user` (rccl_communicator) the C
         hook tcmi_rccl_reduce: ncclReduce queued on the context's stream; else torch.distributed's reduce, RCCL under "nccl"); a rank
         that cannot decode its range still takes part (zeros + a failure word): nobody waits for it forever, and every rank learns
         the verdict;
      2. rank 0 calls (HIP call kernel) and broadcasts the insert-candidate columns;
      3. every rank collects the 48-byte entries of those columns from its resident stream (ins_entries_kernel); the ranks agree that
         all of them could (a rank whose range holds reads the entry kernel does not take — longer than 512 positions — says so
         instead of leaving the others in the gather), then send them to rank 0;
      4. rank 0 concatenates the pieces per column in rank order — file order: pysam's max_depth admission and first-seen tie-break
         depend on it —, votes (tcmi_modal_from_entries), and walks.  Overlapping mates whose other mate would have to be looked at on
         another rank, or a rank that could not collect its entries: rank 0 decodes the file on the host for the tokens
         (tcmi_bam_load + tcmi_modal_tokens).

    step_fn(first, count) -> (counts int [L,7] of the rank's range) and entries_fn(positions) -> (entry bytes, ent_off, long text)
    replace the GPU on boxes without one (tests: the oracle's tally and entries; the call then comes from the oracle too).
    return_parts: rank 0 gets (FASTA text, counts int32 [L,7], {candidate column: modal token}) — what the command line's other
    writers need (Outputs.WriteOutputs, Coverage.BuildCoverage).  ctx / dbam: the caller's (kept open: a bench loop); timings: a dict
    that receives the seconds of "step" (tcmi_split_step, reduce included) and "entries" (steps 2-4 up to the vote).
    rules: the ReadRules every rank sets on its context (Context.set_rules; None leaves what the context has).  Its read_filter: the
    rank's read set keeps it for step 3, and rank 0's host sweep of step 4 removes the failing records too.  Its min_baseq and
    primers: the base-quality floor and the primer table of the count matrix; the insert tokens keep their own quality rule.  Its
    mate_overlap: refused by tcmi_split_step (a record's mate may lie in another rank's range).  Three counts behind the step, each taken by
    every rank in its own read set and summed to rank 0 over the same group (_sum_to_root), each one more item of rank 0's return_parts
    tuple, in this order: amplicon_reads = ([(fs, le, rs, fe)], slack): the records per amplicon (Context.amplicon_reads) -> the
    [n + 2, 2] int64 counts; variant_strand = the keyword arguments of Context.variants (ref, min_af, min_alt_depth, min_depth): rank 0
    lists the variant table's records from the reduced matrix and broadcasts their distinct columns (_root_columns), the planes at those
    columns per strand (Context.strand_counts) -> (records, strand counts); variant_links = (the same keyword arguments, K): the joint
    token classes at the root's columns and their next K (Context.link_counts) -> (records, link counts)."""
    import time
    import torch
    import torch.distributed as dist
    multi = dist.is_initialized() and dist.get_world_size(group) > 1
    L = int(ref_len)
    ld, n_words = split_words(L, world)
    root = rank == 0
    plain = alt = flags = counts_root = reads_root = strand_root = links_root = None
    if variant_strand is not None and step_fn is not None:
        raise ValueError("consensus_split_bamfile: variant_strand counts in the stream the device decoded: it does not go with step_fn")
    if variant_links is not None and step_fn is not None:
        raise ValueError("consensus_split_bamfile: variant_links counts in the stream the device decoded: it does not go with step_fn")
    own_ctx, own_d = ctx is None, dbam is None
    d, rs = dbam, None
    err = None
    t0 = time.perf_counter()
    try:
        if step_fn is None:
            torch.cuda.set_device(device)
            try:
                if ctx is None:
                    ctx = Context(device, stream=torch.cuda.current_stream().cuda_stream)
                if d is None:
                    d = DeviceBam(path)
                ctx.set_rules(rules)
            except (TcmiError, OSError) as e:                        # this rank cannot even start: it must still meet the others in the reduce
                err = (getattr(e, "code", _ffi_E_ARG), str(e))
            t = torch.zeros(n_words, dtype=torch.int32, device="cuda")
            if err is not None:
                t[-1] = 1
                if rccl_user is not None:                            # (the others are in ncclReduce on that communicator)
                    from . import _ffi
                    rrc = _ffi.rccl_lib().tcmi_rccl_reduce(C.cast(C.pointer(rccl_user), C.c_void_p), C.c_void_p(t.data_ptr()), t.numel(),
                                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
                    torch.cuda.synchronize()
                    if rrc:                                          # (the failure this rank reports gains the reduce's own)
                        err = (err[0], "%s; and its share of the reduce failed too: %s" % (err[1], (_ffi.rccl_lib().tcmi_rccl_last_error() or b"").decode()))
                else:
                    reduce_counts(t, 0, group)
            else:
                @C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
                def hook(user, ptr, n, stream):                      # (the tensor IS the buffer at `ptr`; torch's collective runs on the context's stream)
                    try:
                        reduce_counts(t, 0, group)
                        return 0
                    except Exception:                                # noqa: BLE001 — a C caller gets a code, not an exception
                        return 1
                if rccl_user is not None:
                    from . import _ffi
                    fn, user = C.cast(_ffi.rccl_lib().tcmi_rccl_reduce, C.c_void_p), C.cast(C.pointer(rccl_user), C.c_void_p)
                else:
                    fn, user = hook, None
                rc, rs, planes = _split_step(ctx, d, rank, world, L, ld, t, mincov, include_ambig, fn, user)
                if rc:
                    err = (rc, (lib().tcmi_last_error(ctx.handle) or b"").decode("utf-8", "replace"))
                elif root:
                    plain, alt, flags = planes
                    if return_parts or variant_strand is not None or variant_links is not None:
                        counts_root = np.ascontiguousarray(t[:7 * ld].view(7, ld)[:, :L].T.cpu().numpy())
        else:
            d_blocks = step_fn("n_blocks")
            first, count = block_range(d_blocks, rank, world)
            part = torch.from_numpy(np.ascontiguousarray(np.asarray(step_fn((first, count))).T.astype(np.int32)))
            if multi:
                dist.reduce(part, dst=0, op=dist.ReduceOp.SUM, group=group)
            if root:
                counts_root = np.ascontiguousarray(part.numpy().T)
                plain, alt, flags = step_fn(("call", counts_root, int(mincov), bool(include_ambig)))
        if timings is not None:
            timings["step"] = time.perf_counter() - t0
        t1 = time.perf_counter()
        # every rank learns whether the step held everywhere (a failed rank took part in the reduce: no deadlock, but no consensus either)
        err = _agree(err, group, multi)
        if err:
            raise TcmiError(err[0], "consensus_split_bamfile: %s" % err[1])
        # behind the step: every rank counts in its own records, one sum to rank 0 (a record starts in one rank's blocks: the sum is the file's)
        if amplicon_reads is not None:
            def count():
                got = ctx.amplicon_reads(rs, *amplicon_reads)
                return np.ascontiguousarray(np.stack([got["reads"], got["full"]], axis=1))
            mine = _sum_to_root("amplicon reads", count, group, multi)
            reads_root = mine if root else None
        if variant_strand is not None:
            from .engine import STRAND_DTYPE
            vrecs, vcols = _root_columns(ctx, counts_root, variant_strand, root, group, multi)

            def count():
                got = ctx.strand_counts_of(rs, cols=vcols)
                return np.ascontiguousarray(np.concatenate([got["fwd"], got["rev"]], axis=1).reshape(len(vcols), 14))
            mine = _sum_to_root("strand counts", count, group, multi)
            if root:
                strand = np.zeros(len(vcols), STRAND_DTYPE)
                strand["fwd"], strand["rev"], strand["pos"] = mine[:, :7], mine[:, 7:], vcols
                strand_root = (vrecs, strand)
        if variant_links is not None:
            from .engine import LINK_DTYPE
            vrecs, vcols = _root_columns(ctx, counts_root, variant_links[0], root, group, multi)
            got = []                                                 # (a and b are the same on every rank: the columns are the root's)

            def count():
                got.append(ctx.link_counts(rs, vcols, variant_links[1]) if len(vcols) else np.zeros(0, LINK_DTYPE))
                return np.ascontiguousarray(got[0]["j"].reshape(len(got[0]), 49))
            mine = _sum_to_root("link counts", count, group, multi)
            if root:
                links = got[0].copy()
                links["j"] = mine.reshape(len(links), 7, 7)
                links_root = (vrecs, links)
        # the insert-candidate columns, from rank 0 to everybody
        cand = [(np.nonzero(flags & 8)[0] + 1).tolist()] if root else [None]
        if multi:
            dist.broadcast_object_list(cand, src=0, group=group)
        cand = cand[0]
        text = None
        host_sweep = False
        if cand:
            piece, perr = None, None
            try:
                piece = entries_fn(cand) if entries_fn is not None else _entries_of_readset(ctx, rs, cand)
            except TcmiError as e:                                   # e.g. TCMI_E_UNSUPPORTED: a read of more than 512 positions in this rank's range
                perr = (e.code, str(e))
            pieces = [piece]
            perr = _agree(perr, group, multi)                        # nobody enters the gather unless everybody has a piece
            if perr is not None:
                if perr[0] != _ffi_E_UNSUPPORTED:
                    raise TcmiError(perr[0], "consensus_split_bamfile: insert entries: %s" % perr[1])
                host_sweep = True                                    # rank 0 sweeps the file on the host, as it does for the vote's status bit 2
            elif multi:
                pieces = [None] * dist.get_world_size(group) if root else None
                dist.gather_object(piece, pieces, dst=0, group=group)
        toks = {}
        if root:
            if cand:
                toks = _tokens_for(path, cand, pieces, host_sweep, rules)
            if timings is not None:
                timings["entries"] = time.perf_counter() - t1
            text = _fasta_from_records(name, mincov, gff_rows, plain, alt, flags, toks)
    finally:
        t2 = time.perf_counter()
        if rs is not None:
            rs.free()
        if d is not None and own_d:
            d.close()
        if ctx is not None and own_ctx and step_fn is None:
            ctx.close()
        if timings is not None:
            timings["release"] = time.perf_counter() - t2
            timings["total"] = time.perf_counter() - t0
    if return_parts:
        parts = (text, counts_root, toks) + ((reads_root,) if amplicon_reads is not None else ()) + ((strand_root,) if variant_strand is not None else ()) + \
            ((links_root,) if variant_links is not None else ())
        return parts if root else None
    return text


def split_ranks_in_turn(path, ref_len, gff_rows, mincov, world, include_ambig=True, name="S", device=0, return_parts=False, timings=None,
                        split_sub=None, rules=None):
    """BASELINE configs[4] at ANY world size on the ONE GPU there is: the ranks' steps of a `world`-GPU job played one after the other
    on one context — rank world-1 first, rank 0 (the root) last — each through tcmi_split_step exactly as a rank of the real job runs
    it (its own contiguous range of the file's BGZF blocks + the block behind it, the range table and the failure word behind the
    matrix, the root's pairwise check of the joins, the call kernel on the root).  The hook stands in for the collective: a non-root
    rank's buffer is added to an accumulator on the device, the root's hook adds the accumulator to its own — the integer sum RCCL's
    reduce delivers (indexing.py:96-100 is the pass the ranks share).  What it cannot show is the collective's time: `timings`
    receives per rank the seconds of its step ("rank_seconds"), so that a node's step can be projected as max(rank) + reduce.
    Insert candidates are voted on from every rank's entries, gathered in rank order as consensus_split_bamfile's step 4 does
    (Events.py:47-82).  -> FASTA text (return_parts: + counts int32 [L,7] + {column: token})."""
    import time
    import torch
    L = int(ref_len)
    world = int(world)
    ld, n_words = split_words(L, world)
    torch.cuda.set_device(device)
    ctx = Context(device, stream=torch.cuda.current_stream().cuda_stream)
    if split_sub is not None:                                        # (tcmi_split_step's sub-ranges per rank: 0 = auto, 1 = never)
        ctx.set_option("split_sub", int(split_sub))
    ctx.set_rules(rules)                                             # (every rank the same rules)
    d = DeviceBam(path)
    acc = torch.zeros(n_words, dtype=torch.int32, device="cuda")
    t = torch.zeros(n_words, dtype=torch.int32, device="cuda")
    state = {"root": False}

    @C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
    def hook(user, ptr_, n, stream):                                 # (ptr_ IS t's buffer; the context runs on torch's current stream)
        if int(n) != n_words or int(ptr_) != t.data_ptr():
            return 1
        if state["root"]:
            t.add_(acc)
        else:
            acc.add_(t)
        return 0

    secs, sets = [0.0] * world, [None] * world
    plain = alt = flags = None
    try:
        for rank in range(world - 1, -1, -1):
            state["root"] = rank == 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc, sets[rank], planes = _split_step(ctx, d, rank, world, L, ld, t, mincov, include_ambig, hook, None)
            torch.cuda.synchronize()
            secs[rank] = time.perf_counter() - t0
            if rc:
                raise TcmiError(rc, "split_ranks_in_turn: rank %d of %d: %s" % (rank, world, (lib().tcmi_last_error(ctx.handle) or b"").decode("utf-8", "replace")))
            if rank == 0:
                plain, alt, flags = planes
            else:                                                    # (a context holds ONE resident stream: this rank's entries are collected below, from a decode of their own)
                sets[rank].free()
                sets[rank] = None
        counts = np.ascontiguousarray(t[:7 * ld].view(7, ld)[:, :L].T.cpu().numpy()) if return_parts else None
        cand = (np.nonzero(flags & 8)[0] + 1).tolist()
        toks = {}
        if cand:
            pieces = []
            for rank in range(world):                                # rank order = file order
                rs = sets[rank]
                if rs is None:
                    rs = ctx.upload_bamfile(d, blocks=block_range(d.n_blocks, rank, world))
                try:
                    pieces.append(_entries_of_readset(ctx, rs, cand))
                finally:
                    rs.free()
                    sets[rank] = None
            toks = _tokens_for(path, cand, pieces, False, rules)
        text = _fasta_from_records(name, mincov, gff_rows, plain, alt, flags, toks)
        if timings is not None:
            timings.update(rank_seconds=secs, blocks_per_rank=[block_range(d.n_blocks, r, world)[1] for r in range(world)],
                           n_blocks=d.n_blocks, file_bytes=d.file_bytes, inflated_bytes=d.inflated_bytes,
                           decode_batched=ctx.stat("decode_batched"), one_sync_taken=ctx.stat("one_sync_taken"), split_sub_taken=ctx.stat("split_sub_taken"))
    finally:
        for rs in sets:
            if rs is not None:
                rs.free()
        d.close()
        ctx.close()
    return (text, counts, toks) if return_parts else text
