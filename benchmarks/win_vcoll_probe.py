"""Irregular window collectives against today's routing (comm.py "irregular window collectives"),
and peer_plan_gather (csrc/kernels/peer_plan.hip) against what it replaces.

Multi-rank part (ranks may share one GPU, and then see no xGMI): for every size, blocking calls on
symmetric fp32 buffers alternate between ``algo="auto"`` (today's routing), ``algo="p2p"``,
``algo="window"`` and ``auto`` again; every call ends in a device synchronise and a cell is the
slowest rank's median over --iters calls after --warmup. The two ``auto`` medians bracket the
spread every difference is read against. ``alltoallv``: uneven counts (rank s sends a share
proportional to q + 1 to rank q). ``alltoallw``: a column-block transpose, every send a strided
column block, every receive a strided transposed block. The size is one rank's whole send
stream. One JSON line per cell on rank 0; --md appends a table.

    python -m torch.distributed.run --nproc-per-node 4 benchmarks/win_vcoll_probe.py --md profiles/win_vcollectives.md

Single-process part (``--kernels``): 8 strided segments (column blocks) moved by one
peer_plan_gather launch against one type_copy pack per segment plus one peer_gather of the packed
streams (and against a single pack plus gather of one segment of the same total size).

    python benchmarks/win_vcoll_probe.py --kernels --md profiles/win_vcollectives.md
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

SIZES_KIB = "4,64,1024,16384,65536"


def write_md(path, title, rows):
    if not path or not rows:
        return
    keys = list(rows[0])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    new = not os.path.exists(path)
    with open(path, "a") as f:
        if new:
            f.write("# Irregular window collectives: measurements\n\nWritten by `benchmarks/win_vcoll_probe.py`; "
                    "times in microseconds (the slowest rank's median).\n")
        f.write(f"\n## {title}\n\n| " + " | ".join(keys) + " |\n|" + "---|" * len(keys) + "\n")
        for row in rows:
            f.write("| " + " | ".join(str(row[k]) for k in keys) + " |\n")


def kernels(iters, warmup, sizes_kib, md):
    from mpit_amd import datatypes as dt
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

    rows, ng = [], 8
    for kib in sizes_kib:
        cb = 64  # fp32 columns per block: runs of 256 bytes
        rows_n = max(1, kib * 1024 // 4 // (ng * cb))
        A = torch.randn(rows_n, ng * cb, device="cuda")
        B = torch.zeros(ng, rows_n * cb, device="cuda")
        tmp = torch.zeros(ng, rows_n * cb, device="cuda")
        views = [A[:, g * cb:(g + 1) * cb] for g in range(ng)]
        plans = [dt.layout_of(v) for v in views]
        nb = rows_n * cb * 4
        segs = [(v.data_ptr(), ([list(x) for x in p.loops], 0, 1, p.L, p.L), B[g].data_ptr(), ([], 0, 1, nb, nb), 16)
                for g, (v, p) in enumerate(zip(views, plans))]

        def pack_gather():
            for g, (v, p) in enumerate(zip(views, plans)):
                dt.run_plan(p, 0, dt._bytes_at(v), tmp[g].view(torch.uint8))
            nat.peer_gather(dev, stream, [tmp[g].data_ptr() for g in range(ng)], [B[g].data_ptr() for g in range(ng)],
                            [nb] * ng, 0)

        plan_us = timed(lambda: nat.peer_plan_gather(dev, stream, segs, 0, False))
        assert torch.equal(B.view(ng, rows_n, cb), torch.stack([v.contiguous() for v in views]))
        two_us = timed(pack_gather)
        whole = dt.layout_of(A[:, : ng * cb // 2])  # one strided segment of half the matrix
        wv, wt = A[:, : ng * cb // 2], tmp.view(-1)[: A.numel() // 2]

        def one_pack_gather():
            dt.run_plan(whole, 0, dt._bytes_at(wv), wt.view(torch.uint8))
            nat.peer_gather(dev, stream, [wt.data_ptr()], [B.data_ptr()], [wt.numel() * 4], 0)

        one_us = timed(one_pack_gather)
        row = dict(KiB=kib, segments=ng, peer_plan_gather_us=round(plan_us, 1), packs_plus_peer_gather_us=round(two_us, 1),
                   ratio=round(two_us / plan_us, 2), GBps_plan=round(2 * ng * nb / plan_us / 1e3, 1),
                   one_pack_plus_gather_half_size_us=round(one_us, 1))
        rows.append(row)
        print(json.dumps(dict(benchmark="win_vcoll_kernels", **row)), flush=True)
    write_md(md, "peer_plan_gather (8 column blocks, one launch) against 8 type_copy packs + one peer_gather", rows)


def collectives(iters, warmup, sizes_kib, only, md):
    import mpit_amd as mp
    from mpit_amd import comm as C

    mp.Init()
    W = C.COMM_WORLD()
    r, n = W.Get_rank(), W.Get_size()
    on_gpu = mp.runtime.device() is not None
    nmax = 2 * max(sizes_kib) * 1024 // 4 + 64 * n  # (a rank receives up to 2n / (n + 1) of what it sends)
    A = W.sym_alloc(nmax, torch.float32, device=on_gpu)
    B = W.sym_alloc(nmax, torch.float32, device=on_gpu)
    A.zero_()
    B.zero_()

    def sync():
        if on_gpu:
            torch.cuda.synchronize()

    def calls(N):
        unit = max(1, N // (n * (n + 1) // 2))  # rank q receives (q + 1) units from everyone
        sc = [unit * (q + 1) for q in range(n)]
        sd = [sum(sc[:q]) for q in range(n)]
        rc = [unit * (r + 1)] * n
        rd = [unit * (r + 1) * s for s in range(n)]
        cb = 32
        rows = max(1, N // (n * cb))
        Am, Bm = A[: rows * n * cb].view(rows, n * cb), B[: rows * n * cb].view(cb, n * rows)
        sends = [Am[:, q * cb:(q + 1) * cb] for q in range(n)]
        recvs = [Bm[:, s * rows:(s + 1) * rows].t() for s in range(n)]
        return {
            "alltoallv": lambda algo: W.Alltoallv(A[: sum(sc)], sc, sd, B[: sum(rc)], rc, rd, algo=algo),
            "alltoallw": lambda algo: W.Alltoallw(sends, recvs, algo=algo),
        }

    out = []
    for kib in sizes_kib:
        N = kib * 1024 // 4
        for name, call in calls(N).items():
            if only and name not in only:
                continue
            arms = [("auto", "auto"), ("p2p", "p2p"), ("window", "window"), ("auto_again", "auto")]
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
                worst = {a: max(g[a] for g in got) for a in med}
                base = min(worst["auto"], worst["auto_again"])
                spread = abs(worst["auto"] - worst["auto_again"])
                row = dict(ranks=n, collective=name, KiB=kib, auto_us=round(worst["auto"], 1),
                           auto_again_us=round(worst["auto_again"], 1), p2p_us=round(worst["p2p"], 1),
                           window_us=round(worst["window"], 1), spread_us=round(spread, 1),
                           speedup=round(base / worst["window"], 2),
                           beyond_spread=bool(abs(base - worst["window"]) > spread))
                out.append(row)
                print(json.dumps(dict(benchmark="win_vcollectives", **row)), flush=True)
    st = W.vcoll_stats()
    assert all(v["fallback"] == 0 and v["window_staged"] == 0 for v in st.values()), st
    if r == 0:
        where = "one GPU shared by the ranks (no xGMI)" if on_gpu else "host shm windows"
        write_md(md, f"{n} ranks, {where}: window against today's routing (auto), symmetric fp32 buffers", out)
    W.sym_free()
    mp.Finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true", help="the single-process kernel comparison")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default=SIZES_KIB, metavar="KiB,KiB,...")
    ap.add_argument("--only", default="", help="alltoallv, alltoallw (default: both)")
    ap.add_argument("--md", default="", help="append the table to this markdown file")
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]
    if a.kernels:
        kernels(a.iters, a.warmup, sizes, a.md)
    else:
        collectives(a.iters, a.warmup, sizes, [x for x in a.only.split(",") if x], a.md)


if __name__ == "__main__":
    main()
