"""Window collectives against today's routing (comm.py "window collectives"), and the three
kernels of csrc/kernels/peer_coll.hip against what they replace.

Multi-rank part (ranks may share one GPU): for every collective and size, blocking calls on
symmetric fp32 buffers alternate between ``algo="auto"`` (today's routing: the code this path
does not touch), ``algo="window"`` and ``auto`` again; every call ends in a device synchronise and
a cell is the median over --iters calls after --warmup. The two ``auto`` medians bracket the
spread every difference is read against. One JSON line per cell on rank 0.

    python -m torch.distributed.run --nproc-per-node 3 benchmarks/win_coll_probe.py

Single-process part (``--kernels``, no communicator): peer_gather of 8 x 8 MiB against one torch
copy_ of 64 MiB and against itself with source and destination 1, 4 and 8 bytes apart;
peer_gather of 8 x 4 KiB in one launch against 8 peer_reduce(ns=1) launches; peer_fold into a
misaligned destination against peer_reduce on the same operands (its scalar path) at 40 MiB.

    python benchmarks/win_coll_probe.py --kernels
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def kernels(iters, warmup):
    from mpit_amd._ext import native

    nat = native()
    dev, stream = torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream

    def timed(fn):
        ts = []
        for k in range(warmup + iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if k >= warmup:
                ts.append(a.elapsed_time(b) * 1e3)
        return statistics.median(ts)

    def line(**kw):
        print(json.dumps(dict(benchmark="win_coll_kernels", **kw)), flush=True)

    seg, ng, pad = 8 << 20, 8, 64
    src = torch.randint(0, 255, (ng * (seg + pad),), dtype=torch.uint8, device="cuda")
    dst = torch.zeros(ng * (seg + pad), dtype=torch.uint8, device="cuda")
    us = timed(lambda: dst[: ng * seg].copy_(src[: ng * seg]))
    line(case="torch copy_ 64 MiB", us=us, GBps=2 * ng * seg / us / 1e3)
    base = None
    for delta in (0, 1, 4, 8):
        sp = [src.data_ptr() + g * (seg + pad) + delta for g in range(ng)]
        dp = [dst.data_ptr() + g * (seg + pad) for g in range(ng)]
        us = timed(lambda: nat.peer_gather(dev, stream, sp, dp, [seg] * ng, 0))
        base = base or us
        line(case=f"peer_gather 8 x 8 MiB, src - dst = {delta} B", us=us, GBps=2 * ng * seg / us / 1e3,
             ratio_to_aligned=us / base)
    small = 4096
    sp = [src.data_ptr() + g * (seg + pad) for g in range(ng)]
    dp = [dst.data_ptr() + g * (seg + pad) for g in range(ng)]
    one = timed(lambda: nat.peer_gather(dev, stream, sp, dp, [small] * ng, 0))
    eight = timed(lambda: [nat.peer_reduce(dev, stream, 0, 6, [sp[g]], [dp[g]], small) for g in range(ng)])
    line(case="8 x 4 KiB: one peer_gather launch", us=one)
    line(case="8 x 4 KiB: 8 peer_reduce(ns=1) launches", us=eight, ratio_to_one_launch=eight / one)
    n, ns = (40 << 20) // 4, 3
    xs = [torch.randn(n + 8, device="cuda") for _ in range(ns)]
    out = torch.zeros(n + 8, device="cuda")
    ptrs = [x.data_ptr() for x in xs]
    res = {}
    for name, off in (("aligned", 0), ("misaligned", 4)):
        res["fold_" + name] = timed(lambda: nat.peer_fold(dev, stream, 0, 0, ptrs, out.data_ptr() + off, n, 0))
        res["reduce_" + name] = timed(lambda: nat.peer_reduce(dev, stream, 0, 0, ptrs, [out.data_ptr() + off], n))
    gb = (ns + 1) * n * 4 / 1e3
    for k, us in res.items():
        line(case=f"40 MiB fp32 SUM of {ns}: peer_{k.replace('_', ', destination ')}", us=us, GBps=gb / us)
    line(case="peer_fold misaligned / aligned", ratio=res["fold_misaligned"] / res["fold_aligned"])
    line(case="peer_reduce (scalar) / peer_fold, misaligned destination",
         ratio=res["reduce_misaligned"] / res["fold_misaligned"])


def collectives(iters, warmup, sizes_kib, only):
    import mpit_amd as mp
    from mpit_amd import comm as C

    mp.Init()
    W = C.COMM_WORLD()
    r, n = W.Get_rank(), W.Get_size()
    on_gpu = mp.runtime.device() is not None
    nmax = max(sizes_kib) * 1024 // 4 // n * n
    A = W.sym_alloc(nmax, torch.float32, device=on_gpu)
    B = W.sym_alloc(nmax, torch.float32, device=on_gpu)
    A.zero_()
    B.zero_()

    def sync():
        if on_gpu:
            torch.cuda.synchronize()

    def calls(N):
        c = N // n
        return {
            "reduce_scatter": lambda algo: W.Reduce_scatter(A[:N], B[:c], None, C.SUM, algo=algo),
            "allgather": lambda algo: W.Allgather(A[r * c:(r + 1) * c], A[:N], algo=algo),  # in place
            "alltoall": lambda algo: W.Alltoall(A[:N], B[:N], algo=algo),
            "bcast": lambda algo: W.Bcast(A[:N], 0, algo=algo),
            "reduce": lambda algo: W.Reduce(A[:N], B[:N] if r == 0 else None, C.SUM, 0, algo=algo),
            "scan": lambda algo: W.Scan(A[:N], A[:N], C.SUM, algo=algo),  # in place
        }

    for kib in sizes_kib:
        N = max(n, kib * 1024 // 4 // n * n)
        for name, call in calls(N).items():
            if only and name not in only:
                continue
            arms = [("auto", "auto"), ("window", "window"), ("auto_again", "auto")]
            ts = {a: [] for a, _ in arms}
            for k in range(warmup + iters):
                for arm, algo in arms:  # alternating, so that drift hits every arm alike
                    W.Barrier()
                    sync()
                    t0 = time.perf_counter()
                    call(algo)
                    sync()
                    if k >= warmup:
                        ts[arm].append((time.perf_counter() - t0) * 1e6)
            med = {a: statistics.median(v) for a, v in ts.items()}
            got = W.allgather_obj(med)
            if r == 0:
                worst = {a: max(g[a] for g in got) for a in med}  # the slowest rank's median
                base = min(worst["auto"], worst["auto_again"])
                spread = abs(worst["auto"] - worst["auto_again"])
                print(json.dumps(dict(benchmark="win_collectives", ranks=n, collective=name, KiB=kib,
                                      auto_us=round(worst["auto"], 1), auto_again_us=round(worst["auto_again"], 1),
                                      window_us=round(worst["window"], 1), spread_us=round(spread, 1),
                                      speedup=round(base / worst["window"], 2),
                                      beyond_spread=bool(abs(base - worst["window"]) > spread))), flush=True)
    st = W.coll_stats()
    assert all(v["fallback"] == 0 and v["window_staged"] == 0 for v in st.values()), st
    W.sym_free()
    mp.Finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true", help="the single-process kernel comparisons")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="4,256,4096,40960", metavar="KiB,KiB,...")
    ap.add_argument("--only", default="", help="comma-separated collectives (default: all)")
    a = ap.parse_args()
    if a.kernels:
        kernels(a.iters, a.warmup)
    else:
        collectives(a.iters, a.warmup, [int(x) for x in a.sizes.split(",")], [x for x in a.only.split(",") if x])


if __name__ == "__main__":
    main()
