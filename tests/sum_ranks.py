"""One rank of tests/test_stream_requests.py's two-process gloo group (python -m tests.sum_ranks RANK PORT): distributed._agree and
distributed._sum_to_root, case after case on the one group; what this rank saw goes to stdout as one JSON line.  No GPU."""
import json
import os
import sys

import numpy as np

WHAT = "strand counts"
MSG = "no counts here"


def own_array(rank):
    return (np.arange(6, dtype=np.int64).reshape(3, 2) + 1) * (10 ** rank)


def main(rank, port):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    from trueconsense_amd import _ffi
    from trueconsense_amd import distributed as td
    dist.init_process_group("gloo", rank=rank, world_size=2)
    out = {}
    try:
        # _agree: an error on rank 0 only, on rank 1 only, on both, on none
        for name, who in (("root", (0,)), ("other", (1,)), ("both", (0, 1)), ("none", ())):
            out["agree_" + name] = td._agree((-(rank + 3), "rank %d" % rank) if rank in who else None, None, True)
        # (a) both ranks count
        out["sum"] = td._sum_to_root(WHAT, lambda: own_array(rank), None, True).tolist()

        # (b) rank 1 has no counts: nobody enters the reduce, both raise
        def refused():
            if rank == 1:
                raise _ffi.TcmiError(_ffi.E_NOMEM, MSG)
            return own_array(rank)
        try:
            td._sum_to_root(WHAT, refused, None, True)
            out["refused"] = None
        except _ffi.TcmiError as e:
            out["refused"] = (e.code, str(e))
        # (c) nothing to sum: the array comes back as it is, and a reduce that only one rank had entered would leave this barrier waiting
        empty = np.zeros((0, 14), np.int32)
        out["empty_untouched"] = td._sum_to_root(WHAT, lambda: empty, None, True) is empty
        dist.barrier()
        out["barrier"] = True
    finally:
        dist.destroy_process_group()
    print(json.dumps(out))


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]))
