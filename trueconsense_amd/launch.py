"""--gpus N: the launcher of the command line's child processes.  The children are started BEFORE this process touches a GPU (a
process that did is never re-executed); run_gpus deals a manifest's shards, or one file's ranks, to them."""
from __future__ import annotations

import os
import sys
import time

from .cli_args import _child_argv, _names_a_table, amplicons_of
from .cli_tables import join_amplicon_parts


def _spawn(cmds, envs):
    """Start the children BEFORE this process touches a GPU (never re-exec a process that did), wait for all, -> worst exit code.
    The children are polled together: once one of them has failed the others get a short grace (they may be waiting for it in a
    collective) and are then terminated, so nobody sits out a collective's time-out."""
    import subprocess
    procs = [subprocess.Popen(c, env=e) for c, e in zip(cmds, envs)]
    rcs = [None] * len(procs)
    failed_at = None
    while any(r is None for r in rcs):
        for i, p in enumerate(procs):
            if rcs[i] is None:
                rcs[i] = p.poll()
                if rcs[i] not in (None, 0) and failed_at is None:
                    failed_at = time.monotonic()
        if failed_at is not None and time.monotonic() - failed_at > float(os.environ.get("TCMI_SPAWN_GRACE", "20")):
            for i, p in enumerate(procs):
                if rcs[i] is None:
                    p.terminate()
            for i, p in enumerate(procs):
                if rcs[i] is None:
                    try:
                        rcs[i] = p.wait(timeout=10)
                    except subprocess.TimeoutExpired:
                        p.kill()
                        rcs[i] = p.wait()
            break
        time.sleep(0.02)
    return max((abs(r) for r in rcs), default=0)


def run_gpus(a):
    """--gpus N: N processes, one per GPU.  --batch: the manifest's samples dealt round-robin (BASELINE configs[3]: independent files,
    no collective); -i: ONE BAM file shared by the GPUs (configs[4]: trueconsense_amd.split_main)."""
    import socket
    import tempfile
    n = int(a.gpus)
    pkg_parent = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base_env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"),
                    PYTHONPATH=os.pathsep.join([pkg_parent] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    one_gpu = os.environ.get("TCMI_SPLIT_ONE_GPU") == "1"              # (rehearsal on a one-GPU box: every child on GPU 0)
    if a.batch:
        rows = [ln for ln in open(a.batch).read().split("\n") if ln.strip() and not ln.startswith("#")]
        # the thresholds without any table: checked once, over the whole manifest, before anything is dealt out (a shard may well name none)
        if a.variant_thresholds_given and not any(_names_a_table(ln) for ln in rows):
            print("--min-af / --min-alt-depth / --variant-min-depth need a variant table: no line of the manifest has a 7th column. Exiting...")
            return 1
        amps = amplicons_of(a)                      # (an unusable scheme ends the run here, before anything is dealt out)
        with tempfile.TemporaryDirectory(prefix="tcmi_gpus_") as tmp:
            cmds, envs, parts = [], [], []
            for k in range(n):
                mine = rows[k::n]
                if not mine:
                    continue
                shard = os.path.join(tmp, "shard%d.tsv" % k)
                with open(shard, "w") as fh:
                    fh.write("\n".join(mine) + "\n")
                cmd = [sys.executable, "-m", "trueconsense_amd.TrueConsense", "--batch", shard, "--device", str(0 if one_gpu else k)] + \
                    _child_argv(a, False, tables=any(_names_a_table(ln) for ln in mine))
                if a.stats:
                    cmd += ["--stats", "%s.gpu%d" % (a.stats, k)]
                if amps:                            # every child a part file of its own beside FILE
                    parts.append("%s.part%d" % (a.amplicon_table, k))
                    cmd += ["--amplicon-table", parts[-1]]
                cmds.append(cmd)
                envs.append(base_env)
            rc = _spawn(cmds, envs)
            if amps and rc == 0:                    # (all children have exited with status 0: the parts are whole)
                join_amplicon_parts(a.amplicon_table, parts, len(rows), len(amps))
            return rc
    if a.index_override:
        print("--index-override goes with one GPU. Exiting...")
        return 1
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmds, envs = [], []
    for k in range(n):
        cmds.append([sys.executable, "-m", "trueconsense_amd.split_main"] + _child_argv(a, True))
        envs.append(dict(base_env, RANK=str(k), LOCAL_RANK=str(k), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port)))
    return _spawn(cmds, envs)
