"""bench.py on one GPU as the driver runs it: a plain run (the headline only) and --dump-outputs, checked against the oracle chain."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_run_times_exactly_k_steps_and_dumps_the_last_fasta(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: one JSON line with the headline keys and exactly K timed steps, none
    of the --full legs, and DIR/fasta_last_step.npy = the FASTA text of the last timed BAM, equal to the oracle chain's on that file."""
    sys.path.insert(0, ROOT)
    import bench
    from trueconsense_amd import synthetic as sy
    steps, files, reads = 3, 2, 40000
    dump = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--reads", str(reads),
           "--files", str(files), "--tmp", str(tmp_path), "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.split("\n") if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["repeats"] == 1 and d["unit"] == "positions/s" and d["higher_is_better"] is True
    assert d["dtype"] == "int32" and d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - 29903 * 1e3 / d["ms_per_step"]) <= 1e-6 * d["value"]
    assert not any(k in d for k in ("cpu_baseline", "fasta_all_timed", "cold_kernels", "roofline", "file_to_fasta", "resident"))
    got = np.load(dump / "fasta_last_step.npy")
    assert got.dtype == np.float32
    text = got.astype(np.uint8).tobytes().decode("ascii")
    # the same seeded input file the last timed step read (bench file (K - 1) mod F of rank 0), through the oracle chain
    ref, orfs = sy.make_reference()
    src = tmp_path / "src"
    src.mkdir()
    paths, _ = bench.write_inputs(str(src), ref, orfs, files, reads, 0, False, 6)
    k = (steps - 1) % files
    want = bench.oracle_chain_many([(paths[k], [dict(o) for o in orfs], len(ref), 30, "S%d" % k)], 1)[0][0]
    assert text == want
