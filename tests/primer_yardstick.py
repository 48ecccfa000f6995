"""The yardstick of the primer mask (--primers; tcmi_ctx_set_primers), from committed oracle functions only: for every read that piles
up, (head_end, tail_start) by brute force over the primer list, then the tokens of tc_oracle.read_tokens on columns
head_end <= col < tail_start whose quality is at least Q, tallied per column with tc_oracle.tally_tokens and zero-padded to
c_oracle.extent.  Primers are (start, end, reverse): 0-based, end-exclusive, reverse true for a '-' (right) primer."""
import numpy as np

from oracle import c_oracle
from oracle import tc_oracle as orc


def scheme(first=30, step=300, n=6, amplicon=400, primer=24):
    """'+' [s, s + 24), '-' [s + 376, s + 400) for s = 30, 330, ...: 2 n primers (the ARTIC-like scheme of the issue)"""
    out = []
    for k in range(n):
        s = first + step * k
        out += [(s, s + primer, False), (s + amplicon - primer, s + amplicon, True)]
    return out


def read_mask(p, q, primers, slack=0):
    """first column p, last column q -> (head_end, tail_start)"""
    heads = [e for s, e, rev in primers if not rev and s - slack <= p < e]
    tails = [s for s, e, rev in primers if rev and s <= q < e + slack]
    return (max(heads) if heads else p), (min(tails) if tails else q + 1)


def counts(rd, L, primers=(), q=0, slack=0, shift=0):
    """-> (int32 [extent, 7] (coverage, A, T, C, G, X, I), piled-up reads with a non-empty mask, tokens kept, tokens of the unmasked reads).
    shift: where the reads' reference starts on the axis the primers are given on (the counts stay in the reference's own columns)."""
    n_pos = c_oracle.extent(rd, L)
    cols = {}
    n_masked = kept = total = 0
    for i in range(int(rd["n_reads"])):
        if not orc.read_piles_up(rd, i):
            continue
        toks = list(orc.read_tokens(rd, i, with_qual=True))
        p, last = toks[0][0], toks[-1][0]
        assert p == int(rd["pos"][i])
        head_end, tail_start = read_mask(p + shift, last + shift, primers, slack)
        n_masked += head_end > p + shift or tail_start <= last + shift
        for col, tok, qual in toks:
            total += 1
            if head_end <= col + shift < tail_start and qual >= q:
                kept += 1
                cols.setdefault(col, []).append(tok)
    out = np.zeros((n_pos, 7), np.int32)
    for c, t in cols.items():
        out[c] = orc.tally_tokens(t)
    return out, n_masked, kept, total
