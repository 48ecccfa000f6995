"""The read set of the tests that take one file split over ranks all the way to the consensus, and the oracle chain's FASTA of it.
No tests in here."""
import numpy as np

from oracle import c_oracle
from oracle import tc_oracle as orc
from trueconsense_amd import synthetic as sy


def consensus_case():
    """An indel-carrier read set whose insert-candidate columns lie around the middle of the file (where two ranks' ranges meet):
    accepted insertions of 1, 2 and 14 bases (the last too long for an entry's key: its bases travel as text), a rejected one."""
    ref, orfs = sy.make_reference(L=4000, cds=[(100, 1900), (2100, 3900)])
    sites = [(1900, "I", "A", 0.9), (1990, "I", "GT", 0.7), (2005, "I", "ACGTACGTACGTAC", 0.8), (2010, "D", 3, 0.6), (2100, "I", "C", 0.4), (3000, "I", "TT", 0.95)]
    reads = sy.make_reads(ref, 6000, seed=91, indel_sites=sites)
    return ref, orfs, reads


def oracle_fasta(reads, orfs, L, mincov):
    counts = c_oracle.tally(reads, L)
    has, ins = orc.list_inserts(counts, mincov, lambda pos1: orc.region_tokens(reads, pos1))
    cons, _ = orc.build_consensus(mincov, counts.astype(np.int64), [dict(o) for o in orfs], True, ins if has else None, True)
    return orc.fasta_text("S", mincov, cons), ins if has else {}
