"""MAXLOC on FLOAT_INT pairs: the window all-reduce against the point-to-point tree (what
``algo="auto"`` runs for this op: RCCL has none) and against MAX on the same number of bytes, and
the peer_reduce kernel alone on pairs against fp32 MAX, aligned and at 4 mod 8.

Multi-rank part (ranks may share one GPU): in place on symmetric memory, blocking calls
alternate between the tree (``algo="p2p"``), MAXLOC ``algo="window"``, MAX ``algo="window"`` on the
same bytes viewed as fp32, and the tree again; every call ends in a device synchronise and a cell
is the slowest rank's median over --iters calls after --warmup. The two tree medians bracket the
spread every difference is read against. One JSON line per size on rank 0.

    python -m torch.distributed.run --nproc-per-node 2 benchmarks/pair_reduce_probe.py

Single-process part (``--kernels``): peer_reduce of 3 sources into one destination, MAXLOC on
FLOAT_INT pairs against MAX on fp32 over the same bytes; all pointers 16-byte aligned, and all
of them 4 bytes past (4 mod 8 for the pairs: their body is accessed where it falls; the fp32 arm
keeps its aligned body behind a three-element head).

    python benchmarks/pair_reduce_probe.py --kernels
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def fill_pairs(t, seed):
    """FLOAT_INT pairs in a uint8 tensor: values from a few small numbers, indices 0..5."""
    g = torch.Generator().manual_seed(seed)
    n = t.numel() // 8
    v = torch.randint(-2, 4, (n,), generator=g).float()
    i = torch.randint(0, 6, (n,), generator=g, dtype=torch.int32)
    raw = torch.stack([v.view(torch.int32), i], dim=1).reshape(-1).view(torch.uint8)
    t.copy_(raw.to(t.device))


def kernels(iters, warmup, pairs):
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

    ns, nb = 3, pairs * 8
    xs = [torch.zeros(nb + 64, dtype=torch.uint8, device="cuda") for _ in range(ns)]
    out = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
    for k, x in enumerate(xs):
        fill_pairs(x[: nb], k)
        fill_pairs(x[nb:], k)
    gb = (ns + 1) * nb / 1e3
    res = {}
    for rep in range(2):  # both arms twice, back to back: the second pass shows the run-to-run spread
        for name, off in (("aligned", 0), ("4 mod 8", 4)):
            ptrs = [x.data_ptr() + off for x in xs]
            res[f"MAXLOC FLOAT_INT, {name}", rep] = timed(
                lambda: nat.peer_reduce(dev, stream, nat.PR_MAXLOC, nat.PR_FLOAT_INT, ptrs, [out.data_ptr() + off],
                                        pairs))
            res[f"MAX fp32, {name}", rep] = timed(
                lambda: nat.peer_reduce(dev, stream, 2, 0, ptrs, [out.data_ptr() + off], 2 * pairs))
    for (case, rep), us in res.items():
        print(json.dumps(dict(benchmark="pair_reduce_kernels", case=case, run=rep, MiB=nb / (1 << 20), sources=ns,
                              us=round(us, 1), GBps=round(gb / us, 1))), flush=True)
    for name in ("aligned", "4 mod 8"):
        r = [res[f"MAXLOC FLOAT_INT, {name}", rep] / res[f"MAX fp32, {name}", rep] for rep in range(2)]
        print(json.dumps(dict(benchmark="pair_reduce_kernels", case=f"MAXLOC / MAX, {name}",
                              ratio=[round(x, 3) for x in r])), flush=True)
    r = [res["MAXLOC FLOAT_INT, 4 mod 8", rep] / res["MAXLOC FLOAT_INT, aligned", rep] for rep in range(2)]
    print(json.dumps(dict(benchmark="pair_reduce_kernels", case="MAXLOC 4 mod 8 / aligned",
                          ratio=[round(x, 3) for x in r])), flush=True)


def collectives(iters, warmup, sizes):
    import mpit_amd as mp
    from mpit_amd import comm as C
    from mpit_amd import datatypes as dt

    mp.Init()
    W = C.COMM_WORLD()
    r, n = W.Get_rank(), W.Get_size()
    on_gpu = mp.runtime.device() is not None
    A = W.sym_alloc(max(sizes) * 8, torch.uint8, device=on_gpu)

    def sync():
        if on_gpu:
            torch.cuda.synchronize()

    for pairs in sizes:
        buf = A[: pairs * 8]
        fill_pairs(buf, r)
        f32 = buf.view(torch.float32)
        arms = [("tree", lambda: W.Allreduce(buf, None, C.MAXLOC, algo="p2p", pairtype=dt.FLOAT_INT)),
                ("maxloc_window", lambda: W.Allreduce(buf, None, C.MAXLOC, algo="window", pairtype=dt.FLOAT_INT)),
                ("max_window", lambda: W.Allreduce(f32, None, C.MAX, algo="window")),
                ("tree_again", lambda: W.Allreduce(buf, None, C.MAXLOC, algo="p2p", pairtype=dt.FLOAT_INT))]
        ts = {a: [] for a, _ in arms}
        for k in range(warmup + iters):
            for arm, call in arms:  # alternating, so that drift hits every arm alike
                W.Barrier()
                sync()
                t0 = time.perf_counter()
                call()
                sync()
                if k >= warmup:
                    ts[arm].append((time.perf_counter() - t0) * 1e6)
        med = {a: statistics.median(v) for a, v in ts.items()}
        got = W.allgather_obj(med)
        if r == 0:
            worst = {a: max(g[a] for g in got) for a in med}  # the slowest rank's median
            tree = min(worst["tree"], worst["tree_again"])
            print(json.dumps(dict(benchmark="pair_allreduce", ranks=n, pairs=pairs, MiB=pairs * 8 / (1 << 20),
                                  tree_us=round(worst["tree"], 1), tree_again_us=round(worst["tree_again"], 1),
                                  spread_us=round(abs(worst["tree"] - worst["tree_again"]), 1),
                                  maxloc_window_us=round(worst["maxloc_window"], 1),
                                  max_window_us=round(worst["max_window"], 1),
                                  tree_over_window=round(tree / worst["maxloc_window"], 2),
                                  maxloc_over_max=round(worst["maxloc_window"] / worst["max_window"], 3))), flush=True)
    st = W.ar_stats()
    assert st["window_staged"] == 0 and st["window"] == 2 * len(sizes) * (warmup + iters), st
    W.sym_free()
    mp.Finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true", help="the single-process kernel comparison")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", default=f"{1 << 20},{16 << 20}", metavar="N,N,...")
    a = ap.parse_args()
    sizes = [int(x) for x in a.pairs.split(",")]
    if a.kernels:
        for p in sizes:
            kernels(a.iters, a.warmup, p)
    else:
        collectives(a.iters, a.warmup, sizes)


if __name__ == "__main__":
    main()
