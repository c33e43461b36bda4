"""Irregular window collectives (csrc/kernels/peer_plan.hip, csrc/core/window.cpp
Window::pull_plan, comm.py "irregular window collectives") on n ranks under torch.distributed.run;
T_DEVICE=cuda: the ranks share the box's GPU and the buffers are HBM, otherwise host shm windows
and the host twins.

Every rank builds every rank's input from a seed (checked against what the ranks hold through
allgather_obj), so the expected value of every call is computed on the CPU from all inputs; every
comparison is bitwise and over the whole receive buffer, whose untouched parts hold a sentinel.
vcoll_stats() is read around every call: a silent fallback, or a staged call where an in-place one
is due, fails. Each case prints ``OK <case>`` on rank 0. Cases (T_CASES, comma separated): rooted,
a2av, a2aw, mixed, big, errors, fifo, subcomm, p2p."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

import mpit_amd as mp
from mpit_amd import comm as C
from mpit_amd.comm import COMM_WORLD

mp.Init()
W = COMM_WORLD()
r, n = W.Get_rank(), W.Get_size()
on_gpu = os.environ.get("T_DEVICE", "cpu") == "cuda"
dev = mp.runtime.device() if on_gpu else torch.device("cpu")
cases = os.environ.get("T_CASES", "rooted,a2av,a2aw,mixed,big,errors,fifo,subcomm,p2p").split(",")
assert float(os.environ["MPIT_AR_STAGE_MB"]) * (1 << 20) == 64 << 10

L = 17000  # elements of every rank's input
BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
DTYPES = [torch.float32, torch.bfloat16, torch.uint8]
SENT = 77


def ok(name):
    W.Barrier()
    if r == 0:
        print("OK", name, flush=True)


def bits(t):
    return t.contiguous().view(BITS[t.element_size()])


def same(a, b):
    return a.shape == b.shape and bool(torch.equal(bits(a.cpu()), bits(b.cpu())))


def gen(dt, rank, length=L):
    g = torch.Generator().manual_seed(100 * rank + 3 + DTYPES.index(dt))
    if dt == torch.uint8:
        return torch.randint(0, 256, (length,), generator=g, dtype=torch.int64).to(dt)
    return (torch.randn(length, generator=g, dtype=torch.float64) * 1000).to(dt)


INPUTS, SYM = {}, {}


def inputs(dt):
    if dt not in INPUTS:
        INPUTS[dt] = [gen(dt, q) for q in range(n)]
        got = W.allgather_obj(INPUTS[dt][r][:512])
        assert all(same(a, b[:512]) for a, b in zip(got, INPUTS[dt]))
    return INPUTS[dt]


def sym(dt, which="in"):
    """Registered buffers shared by the cases: "in" holds my input, "out" is a destination."""
    if (dt, which) not in SYM:
        SYM[(dt, which)] = W.sym_alloc(L, dt, device=on_gpu)
    return SYM[(dt, which)]


def load(dt):
    buf = sym(dt)
    buf.copy_(inputs(dt)[r].to(dev))
    return buf


def sentinel(numel, dt):
    return torch.full((numel,), SENT, dtype=dt).to(dev)


class Stats:
    """vcoll_stats() of one collective around ONE call: path is window, staged or fallback."""

    def __init__(self, comm, name, path):
        self.comm, self.name, self.path = comm, name, path

    def __enter__(self):
        self.before = self.comm.vcoll_stats()[self.name]

    def __exit__(self, *exc):
        if exc[0] is None:
            a, b = self.comm.vcoll_stats()[self.name], self.before
            d = {k: a[k] - b[k] for k in a}
            want = {"window": {"window": 1, "window_staged": 0, "fallback": 0},
                    "staged": {"window": 1, "window_staged": 1, "fallback": 0},
                    "fallback": {"window": 0, "window_staged": 0, "fallback": 1},
                    "none": {"window": 0, "window_staged": 0, "fallback": 0}}[self.path]
            assert d == want, (self.name, self.path, d)


def rooted_layout():
    """counts with a zero (rank 1) and one of several tiles; displacements in reverse rank order
    with gaps of 3 elements. (counts, displs, extent)"""
    counts = [0 if q == 1 else (3001 if q == 0 else 37 * q + 3) for q in range(n)]
    displs, pos = [0] * n, 2
    for q in reversed(range(n)):
        displs[q] = pos
        pos += counts[q] + 3
    return counts, displs, pos


# ---- 1 Gatherv / Gather / Scatterv / Scatter on a non-zero root
if "rooted" in cases:
    root = n - 1
    for dt in DTYPES:
        xs = inputs(dt)
        buf = load(dt)
        counts, displs, extent = rooted_layout()
        for staged in (False, True):
            path = "staged" if staged else "window"
            for off in (0, 1):
                send = xs[r][off: off + counts[r]].clone().to(dev) if staged else buf[off: off + counts[r]]
                recv = sentinel(extent, dt) if r == root else None
                with Stats(W, "gatherv", path):
                    W.Gatherv(send, recv, counts if r == root else None, displs if r == root else None, root, algo="window")
                if r == root:
                    exp = torch.full((extent,), SENT, dtype=dt)
                    for q in range(n):
                        exp[displs[q]: displs[q] + counts[q]] = xs[q][off: off + counts[q]]
                    assert same(recv, exp), ("gatherv", dt, staged, off)
                assert same(send, xs[r][off: off + counts[r]]), "sendbuf modified"
                # Scatterv: the root's send stream has the gaps; every rank's piece lands between guards
                src = (xs[root][:extent].clone().to(dev) if staged else buf[:extent]) if r == root else None
                o = sentinel(counts[r] + 4, dt)
                with Stats(W, "scatterv", path):
                    W.Scatterv(src, o[2 + off: 2 + off + counts[r]] if counts[r] else o[:0],
                               counts if r == root else None, displs if r == root else None, root, algo="window")
                exp = torch.full((counts[r] + 4,), SENT, dtype=dt)
                exp[2 + off: 2 + off + counts[r]] = xs[root][displs[r]: displs[r] + counts[r]]
                assert same(o, exp), ("scatterv", dt, staged, off)
            c = 129
            send = xs[r][5: 5 + c].clone().to(dev) if staged else buf[5: 5 + c]
            recv = sentinel(n * c, dt) if r == root else None
            with Stats(W, "gatherv", path):
                W.Gather(send, recv, root, algo="window")
            if r == root:
                assert same(recv, torch.cat([x[5: 5 + c] for x in xs])), ("gather", dt, staged)
            src = (xs[root][: n * c].clone().to(dev) if staged else buf[: n * c]) if r == root else None
            o = sentinel(c, dt)
            with Stats(W, "scatterv", path):
                W.Scatter(src, o, root, algo="window")
            assert same(o, xs[root][r * c: (r + 1) * c]), ("scatter", dt, staged)
        assert same(buf, xs[r]), "registered buffer modified"
    ok("rooted")


def a2av_layout(c0=7):
    """cnt[s][q] elements from s to q (zero from every even s to s + 1, the diagonal several tiles);
    send displacements with gaps of 2, receive displacements in reverse order with gaps of 3."""
    cnt = [[0 if (s % 2 == 0 and q == (s + 1) % n) else c0 + 13 * s + 101 * q + (1100 if s == q else 0) for q in range(n)] for s in range(n)]
    sd = [[2 + sum(cnt[s][:q]) + 2 * q for q in range(n)] for s in range(n)]
    rd = [[0] * n for _ in range(n)]
    ext = [0] * n
    for q in range(n):
        pos = 1
        for s in reversed(range(n)):
            rd[q][s] = pos
            pos += cnt[s][q] + 3
        ext[q] = pos
    return cnt, sd, rd, ext


def a2av_expected(xs, dt, cnt, sd, rd, ext, me):
    exp = torch.full((ext[me],), SENT, dtype=dt)
    for s in range(n):
        exp[rd[me][s]: rd[me][s] + cnt[s][me]] = xs[s][sd[s][me]: sd[s][me] + cnt[s][me]]
    return exp


def a2av_call(comm, xs, dt, staged, algo, buf=None, lay=None, me=None):
    me = r if me is None else me
    cnt, sd, rd, ext = lay or a2av_layout()
    need = sd[me][-1] + cnt[me][-1]
    send = xs[me][:need].clone().to(dev) if staged else buf[:need]
    recv = sentinel(ext[me], dt)
    comm.Alltoallv(send, cnt[me], sd[me], recv, [cnt[s][me] for s in range(len(cnt))], rd[me], algo=algo)
    assert same(send, xs[me][:need]), "sendbuf modified"
    return recv


# ---- 2 Alltoallv: a zero count, uneven counts, gaps untouched
if "a2av" in cases:
    lay = a2av_layout()
    for dt in DTYPES:
        xs = inputs(dt)
        buf = load(dt)
        for staged in (False, True):
            with Stats(W, "alltoallv", "staged" if staged else "window"):
                recv = a2av_call(W, xs, dt, staged, "window", buf, lay)
            assert same(recv, a2av_expected(xs, dt, *lay, r)), ("alltoallv", dt, staged)
        assert same(buf, xs[r]), "registered buffer modified"
    ok("a2av")


def transpose_case(dt, rows, cb, t_recv):
    """Rank s holds A_s (rows x n*cb) and sends its column block q to rank q; rank q stores it
    transposed into B_q (cb x n*rows) (t_recv) or as row block s of B_q (n*rows x cb)."""
    xs = inputs(dt)
    a_all = [x[3: 3 + rows * n * cb].view(rows, n * cb) for x in xs]
    A = load(dt)[3: 3 + rows * n * cb].view(rows, n * cb)
    out = sym(dt, "out")
    out.fill_(SENT)
    B = out[5: 5 + rows * n * cb].view(cb, n * rows) if t_recv else out[5: 5 + rows * n * cb].view(n * rows, cb)
    sends = [A[:, q * cb: (q + 1) * cb] for q in range(n)]
    if t_recv:
        recvs = [B[:, s * rows: (s + 1) * rows].t() for s in range(n)]
    else:
        recvs = [B[s * rows: (s + 1) * rows, :] for s in range(n)]
    with Stats(W, "alltoallw", "window"):
        W.Alltoallw(sends, recvs, algo="window")
    exp = torch.full((L,), SENT, dtype=dt)
    blocks = [a[:, r * cb: (r + 1) * cb] for a in a_all]
    eb = torch.cat([b.t() for b in blocks], dim=1) if t_recv else torch.cat(blocks, dim=0)
    exp[5: 5 + rows * n * cb] = eb.reshape(-1)
    assert same(out, exp), ("alltoallw transpose", dt, rows, cb, t_recv)
    assert same(sym(dt), xs[r]), "registered buffer modified"


# ---- 3 Alltoallw as a column-block transpose, in place on symmetric memory
if "a2aw" in cases:
    for dt in (torch.float32, torch.bfloat16):
        for rows, cb in ((33, 17), (64, 40)):
            for t_recv in (True, False):
                transpose_case(dt, rows, cb, t_recv)
    ok("a2aw")


def mixed_views(base, me, sending):
    """Per-peer views of a 1-D buffer: contiguous to / from even ranks, strided to / from odd ones."""
    out = []
    for q in range(n):
        s, d = (me, q) if sending else (q, me)
        c = 5 + 40 * s + 2 * d
        at = 16 + q * 700
        if sending:
            out.append(base[at: at + c] if q % 2 == 0 else base[at: at + 2 * c: 2])
        else:
            out.append(base[at: at + c] if q % 2 == 0 else base[at: at + 3 * c: 3])
    return out


# ---- 4 Alltoallw with mixed contiguous and strided peers, in place and staged from plain tensors
if "mixed" in cases:
    for dt in DTYPES:
        xs = inputs(dt)
        buf = load(dt)
        for staged in (False, True):
            src = xs[r].clone().to(dev) if staged else buf
            o = sentinel(L, dt)
            with Stats(W, "alltoallw", "staged" if staged else "window"):
                W.Alltoallw(mixed_views(src, r, True), mixed_views(o, r, False), algo="window")
            exp = torch.full((L,), SENT, dtype=dt)
            for s, v in enumerate(mixed_views(exp, r, False)):
                v.copy_(mixed_views(xs[s], s, True)[r])
            assert same(o, exp), ("alltoallw mixed", dt, staged)
            assert same(src, xs[r]), "sendbuf modified"
    ok("mixed")


# ---- 5 a send stream larger than the staging window: the fallback, on every rank alike
if "big" in cases:
    dt = torch.float32
    xs = inputs(dt)
    c = (64 << 10) // 4 // n + 16  # n * c fp32 > 64 KiB
    d = [q * c for q in range(n)]
    send = xs[r][: n * c].clone().to(dev)
    recv = sentinel(n * c, dt)
    with Stats(W, "alltoallv", "fallback"):
        W.Alltoallv(send, [c] * n, d, recv, [c] * n, d, algo="window")
    assert same(recv, torch.cat([x[r * c: (r + 1) * c] for x in xs]))
    buf = load(dt)
    with Stats(W, "alltoallv", "window"):  # the same call from symmetric memory needs no staging
        W.Alltoallv(buf[: n * c], [c] * n, d, recv.fill_(SENT), [c] * n, d, algo="window")
    assert same(recv, torch.cat([x[r * c: (r + 1) * c] for x in xs]))
    ok("big")


def raises_everywhere(what, call):
    before = W.vcoll_stats()
    try:
        call()
        hit = False
    except ValueError:
        hit = True
    assert all(W.allgather_obj(hit)), (what, "did not raise on every rank")
    assert W.vcoll_stats() == before, (what, "took a ticket or a fallback")


# ---- 6 refusals: every rank raises, before any ticket, and the next collective completes
if "errors" in cases:
    dt = torch.float32
    xs = inputs(dt)
    buf = load(dt)
    c, d = [4] * n, [4 * q for q in range(n)]
    recv = sentinel(4 * n, dt)
    # rank 0 sends one element more to rank 1 than rank 1 expects
    sc = [5 if (r == 0 and q == 1) else 4 for q in range(n)]
    sdd = [5 * q for q in range(n)]
    raises_everywhere("count mismatch", lambda: W.Alltoallv(buf[:64], sc, sdd, recv, c, d, algo="window"))
    # rank n-1's last receive segment ends past its buffer
    rc = [4] * (n - 1) + [5 if r == n - 1 else 4]
    raises_everywhere("span outside", lambda: W.Alltoallv(buf[:64], c, d, recv, rc, d, algo="window"))
    # rank 1 receives into its own send range (not its in-place part)
    bad_recv = buf[2: 2 + 4 * n] if r == 1 else recv
    raises_everywhere("overlap", lambda: W.Alltoallv(buf[:64], c, d, bad_recv, c, d, algo="window"))
    # rank 0 passes a view that needs four loops
    four = buf[: 2 ** 8].view(2, 2, 2, 2, 2, 2, 2, 2)[:, 0, :, 0, :, 0, :, 0]
    flat16 = [buf[100 + 16 * q: 116 + 16 * q] for q in range(n)]
    sends = [four if r == 0 else flat16[q] for q in range(n)]
    recvs = [sentinel(16, dt) for _ in range(n)]
    raises_everywhere("four loops", lambda: W.Alltoallw(sends, recvs, algo="window"))
    raises_everywhere("gatherv mismatch", lambda: W.Gatherv(buf[: 3 + (r == 0)], sentinel(3 * n, dt) if r == n - 1 else None,
                                                            None, None, n - 1, algo="window"))
    with Stats(W, "alltoallv", "window"):
        W.Alltoallv(buf[:64], c, d, recv, c, d, algo="window")
    assert same(recv, torch.cat([x[4 * r: 4 * r + 4] for x in xs]))
    assert same(buf, xs[r])
    ok("errors")


# ---- 7 call order with the all-reduce and the regular window collectives (one FIFO, one staging window)
if "fifo" in cases:
    dt = torch.float32
    xs = inputs(dt)
    lay = a2av_layout()
    for k in range(2):
        a = xs[r][k: k + 9001].clone().to(dev)
        r1 = W.Iallreduce(a, None, C.SUM, algo="window")
        g_out = torch.zeros(n * 515, dtype=dt, device=dev)
        r2 = W.Iallgather(xs[r][k: k + 515].clone().to(dev), g_out, algo="window")
        with Stats(W, "alltoallv", "staged"):
            recv = a2av_call(W, xs, dt, True, "window", lay=lay)  # blocking: ordered behind the two before it
        assert r1.Test() and r2.Test(), "a blocking call returned before an earlier ticket"
        o = sentinel(L, dt)
        r3 = W.Iallreduce(a, None, C.MAX, algo="window")
        with Stats(W, "alltoallw", "staged"):
            W.Alltoallw(mixed_views(xs[r].clone().to(dev), r, True), mixed_views(o, r, False), algo="window")
        assert r3.Test()
        acc = xs[0][k: k + 9001].clone()
        for x in xs[1:]:
            acc = acc + x[k: k + 9001]
        assert same(a, acc) and same(g_out, torch.cat([x[k: k + 515] for x in xs]))
        assert same(recv, a2av_expected(xs, dt, *lay, r))
        exp = torch.full((L,), SENT, dtype=dt)
        for s, v in enumerate(mixed_views(exp, r, False)):
            v.copy_(mixed_views(xs[s], s, True)[r])
        assert same(o, exp)
    ok("fifo")


# ---- 8 sub-communicators: {0,1} and {2,3} at the same time
if "subcomm" in cases and n == 4:
    S = W.Split(r // 2, r)
    sr, base = S.Get_rank(), 2 * (r // 2)
    dt = torch.float32
    parts = [gen(dt, base + q) for q in range(2)]
    sb = S.sym_alloc(L, dt, device=on_gpu)
    sb.copy_(parts[sr].to(dev))
    cnt = [[300 + 7 * s + 3 * q for q in range(2)] for s in range(2)]
    sd = [[1 + sum(cnt[s][:q]) + q for q in range(2)] for s in range(2)]
    rd = [[2 + sum(cnt[p][q] for p in range(s)) + s for s in range(2)] for q in range(2)]
    recv = sentinel(700, dt)
    S.Alltoallv(sb, cnt[sr], sd[sr], recv, [cnt[s][sr] for s in range(2)], rd[sr], algo="window")
    exp = torch.full((700,), SENT, dtype=dt)
    for s in range(2):
        exp[rd[sr][s]: rd[sr][s] + cnt[s][sr]] = parts[s][sd[s][sr]: sd[s][sr] + cnt[s][sr]]
    assert same(recv, exp)
    A = sb[: 20 * 14].view(20, 14)
    o = sentinel(2 * 20 * 7, dt)
    S.Alltoallw([A[:, 7 * q: 7 * q + 7] for q in range(2)], [o.view(7, 40)[:, 20 * s: 20 * s + 20].t() for s in range(2)],
                algo="window")
    eb = torch.cat([p[: 280].view(20, 14)[:, 7 * sr: 7 * sr + 7].t() for p in parts], dim=1)
    assert same(o, eb.reshape(-1))
    root_out = sentinel(2 * 50, dt) if sr == 1 else None
    S.Gather(sb[:50], root_out, 1, algo="window")
    if sr == 1:
        assert same(root_out, torch.cat([p[:50] for p in parts]))
    z = {"window": 1, "window_staged": 0, "fallback": 0}
    assert S.vcoll_stats() == {"gatherv": z, "scatterv": {**z, "window": 0}, "alltoallv": z, "alltoallw": z}, S.vcoll_stats()
    assert set(S.coll_stats()) == {"reduce_scatter", "allgather", "alltoall", "bcast", "reduce", "scan", "exscan"}
    S.sym_free(sb)
    ok("subcomm")


# ---- 9 the same calls by point-to-point messages give the same bits
if "p2p" in cases:
    lay = a2av_layout()
    for dt in (torch.float32, torch.bfloat16):
        xs = inputs(dt)
        a = a2av_call(W, xs, dt, True, "window", lay=lay)
        before = W.vcoll_stats()
        b = a2av_call(W, xs, dt, True, "p2p", lay=lay)
        assert same(a, b), ("alltoallv window != p2p", dt)
        src = xs[r].clone().to(dev)
        o1, o2 = sentinel(L, dt), sentinel(L, dt)
        W.Alltoallw(mixed_views(src, r, True), mixed_views(o1, r, False), algo="p2p")
        assert W.vcoll_stats() == before, "algo='p2p' was counted"
        W.Alltoallw(mixed_views(src, r, True), mixed_views(o2, r, False), algo="window")
        assert same(o1, o2), ("alltoallw window != p2p", dt)
    ok("p2p")

for t in list(SYM.values()):
    W.sym_free(t)
W.sym_free()  # the staging buffers
assert W._sym == []
W.Barrier()
if r == 0:
    print("ALL_DONE", flush=True)
mp.Finalize()
