"""Allreduce / Iallreduce wall time (the reference's test/testreduceall.lua:8-29 and
test/testireduceall.lua:27-36 instruments): MEGS x 2^20 floats (default 10 -> 40 MiB),
SUM, checked for correctness, timed over --iters calls. HBM tensors use RCCL when every
rank owns a distinct GPU, host tensors the shm point-to-point layer (ring all-reduce).
The measurement itself is mpit_amd.instruments.allreduce_time. ``--algo window`` times the
peer-reduce kernel over symmetric memory (comm.py "window all-reduce"), ``--dtype`` the element
type, ``--sweep`` a table of sizes on every path.

    MEGS=10 python -m torch.distributed.run --nproc-per-node 8 benchmarks/allreduce_bench.py
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mpit_amd as mp
from mpit_amd.instruments import allreduce_time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--megs", type=float, default=float(os.environ.get("MEGS", "10")))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--algo", choices=["auto", "window", "p2p"], default=None,
                    help="all-reduce path (default: the MPIT_ALLREDUCE variable, else auto)")
    ap.add_argument("--dtype", choices=["fp32", "bf16", "fp16"], default="fp32")
    ap.add_argument("--sweep", default=None, metavar="KiB,KiB,...",
                    help="message sizes in KiB: p2p, window one-shot and window two-shot at each, one JSON line each")
    a = ap.parse_args()
    import torch

    mp.Init()
    dtype = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[a.dtype]
    rank0 = mp.COMM_WORLD().Get_rank() == 0
    if a.sweep:
        # one process start for the whole table, every arm in place: every size on the point-to-point path and on the
        # window path with one-shot and with two-shot forced (their crossover is the default of
        # MPIT_AR_ONESHOT_BYTES, profiles/win_allreduce.md)
        es = torch.empty(0, dtype=dtype).element_size()
        for kib in [float(x) for x in a.sweep.split(",")]:
            megs = kib * 1024 / es / (1 << 20)
            for label, algo, oneshot in (("p2p", "p2p", None), ("window-oneshot", "window", 1 << 40),
                                         ("window-twoshot", "window", 0)):
                if oneshot is not None:
                    os.environ["MPIT_AR_ONESHOT_BYTES"] = str(oneshot)
                r = allreduce_time(megs, a.iters, a.host, algo=algo, dtype=dtype, inplace=True)
                os.environ.pop("MPIT_AR_ONESHOT_BYTES", None)
                if rank0:
                    print(json.dumps(dict(benchmark="allreduce", KiB=kib, dtype=a.dtype, path=label, **r)), flush=True)
        mp.Finalize()
        return
    r = allreduce_time(a.megs, a.iters, a.host, algo=a.algo, dtype=dtype)
    if rank0:
        print(json.dumps(dict(benchmark="allreduce", **r)), flush=True)
    mp.Finalize()


if __name__ == "__main__":
    main()
