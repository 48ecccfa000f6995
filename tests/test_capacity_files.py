"""CPU: the files of tests/capacity_files.py are (still) beyond the capacities they are written for — the inequalities of the one-sync
path's sizing rules, re-derived from every file as written, so that a change to bamwriter or synth_small cannot quietly turn them
into ordinary files that tests/test_pack_capacities.py would then pass for the wrong reason."""
import numpy as np
import pytest

from oracle import c_oracle
from tests import capacity_files as cf


@pytest.fixture(scope="module")
def facts(tmp_path_factory):
    d = tmp_path_factory.mktemp("capacity_files")
    out = {}
    for case in cf.CASES + ("long_only",):
        p = cf.write(d / (case + ".bam"), case)
        out[case] = cf.facts(p)
        rd = c_oracle.read_bam(p)                                   # (the C oracle's reader agrees on what the walk above counted)
        assert rd["n_reads"] == out[case]["n_rec"] and rd["inflated_bytes"] == out[case]["inflated"], case
        assert np.all(np.diff(rd["pos"]) >= 0), case                # sorted
    return out


def test_the_files_reach_the_cases_they_are_for(facts):
    for case, f in facts.items():
        assert f["ref_len"] == cf.REF_LEN and f["inflated"] <= 2_200_000, (case, f["inflated"])
        assert f["max_end"] < 1 << 29, case
    # a: the header's block shows 38 long records; sized from them the records do not fit, sized for the worst case they do
    f = facts["hint_too_large"]
    assert f["hint"] == 1703 and f["n_rec"] == 20040
    assert f["caps"](f["hint"])["rec_cap"] == 9804 < f["n_rec"] <= f["safe_rec_cap"] == 35353
    safe = f["caps"](0)
    assert f["words"] + 18 <= safe["word_cap"] and f["events"] <= safe["event_cap"] and f["max_end"] <= cf.REF_LEN
    # b: more records than either attempt allows for, whatever the hint; the several-kernel path counts them first
    f = facts["tiny_records"]
    assert f["hint"] == 44 and f["inflated"] == 880068
    for h in (f["hint"], 0, 1703):
        assert f["caps"](h)["rec_cap"] <= 14775 < f["n_rec"] == 20000
    assert f["n_rec"] <= f["inflated"] // 36 + 16
    # c: the records fit, the plane words do not
    f = facts["wide_skips"]
    caps = f["caps"](f["hint"])
    assert f["hint"] == 71 and f["inflated"] == 1420068
    assert f["n_rec"] == 20000 <= caps["rec_cap"] == 23212 and caps["word_cap"] == 244929
    assert f["words"] >= 640000 > caps["word_cap"] and f["max_end"] <= cf.REF_LEN
    # d: records, words and events fit; every read opens a chunk, and they are more than 4 * n_wg + 615 for any grid up to SPARSE_MAX_SLOTS
    f = facts["sparse_beyond_ref_len"]
    caps = f["caps"](f["hint"])
    assert f["hint"] >= 36 and f["n_rec"] == cf.N_SPARSE <= caps["rec_cap"] and f["words"] + 18 <= caps["word_cap"] and f["events"] == 0
    assert f["chunks"] == cf.N_SPARSE > 4 * cf.SPARSE_MAX_SLOTS + (cf.REF_LEN + 65536) // 128 + 64
    assert cf.SPARSE_MAX_SLOTS >= 512 and cf.N_SPARSE <= caps["rec_cap"]       # (chunk_cap is the formula, not rec_cap; an MI355X has 256 CUs)
    assert f["max_end"] > 3_000_000
    # e: everything fits but the events
    f = facts["all_n"]
    caps = f["caps"](f["hint"])
    assert f["hint"] >= 36 and f["n_rec"] == 7500 <= caps["rec_cap"] and f["words"] + 18 <= caps["word_cap"]
    assert f["events"] == 1_125_000 > caps["event_cap"] == 1 << 20
    assert f["events"] > max(1 << 20, f["n_rec"] // 2)              # ... and beyond the several-kernel packer's first capacity too: its re-pack
    assert f["max_end"] <= cf.REF_LEN
    # f: no hint of its own; under the hint the helper file leaves behind the records do not fit, sized for the worst case they do
    f, helper = facts["stale_hint"], facts["long_only"]
    assert f["hint"] == 0 and f["n_ref"] == 300 and f["n_rec"] == 20000
    assert helper["n_rec"] == 80 > 64 and helper["hint"] == 1703
    seen = helper["inflated"] // helper["n_rec"]                    # what the context remembers of the helper file
    assert seen >= 1703 and f["caps"](seen)["rec_cap"] < f["n_rec"] <= f["safe_rec_cap"]
    safe = f["caps"](0)
    assert f["words"] + 18 <= safe["word_cap"] and f["events"] <= safe["event_cap"]
