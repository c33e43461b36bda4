"""Window collectives (csrc/kernels/peer_coll.hip, csrc/core/window.cpp Window::pull_gather /
pull_fold / scan, comm.py "window collectives") on n ranks under torch.distributed.run;
T_DEVICE=cuda: the ranks share the box's GPU and the buffers are HBM, otherwise host shm windows
and the host twins.

Every comparison is bitwise against the CPU computation from the inputs gathered with
allgather_obj (folds: left to right in rank order; 16-bit floats folded in fp32, cast once). Every
collective runs on symmetric buffers (direct: coll_stats shows window, no staging) and on plain
tensors (staged through the 64 KiB staging window in several pieces); a fallback fails the test.
Each case prints ``OK <case>`` on rank 0. Cases (T_CASES, comma separated; default all that fit
the rank count): rs_ag, scan, a2a, rooted, fifo, subcomm, p2p, sharded."""
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
cases = os.environ.get("T_CASES", "rs_ag,scan,a2a,rooted,fifo,subcomm,p2p,sharded").split(",")
assert float(os.environ["MPIT_AR_STAGE_MB"]) * (1 << 20) == 64 << 10

G = 4  # guard elements on both sides of the largest range
COUNTS = [1, 3, n * 4 - 1, 1031, 65541]  # per rank
OFFS = [0, 1, 3]
L = G + max(OFFS) + n * max(COUNTS) + G
FLOATS = [torch.float32, torch.bfloat16, torch.float16, torch.float64]
INTS = [torch.int32, torch.int64, torch.uint8]
BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
FOLDS = [(C.SUM, torch.float32), (C.SUM, torch.bfloat16), (C.MAX, torch.int64)]


def ok(name):
    W.Barrier()
    if r == 0:
        print("OK", name, flush=True)


def bits(t):
    return t.contiguous().view(BITS[t.element_size()])


def same(a, b):
    return a.shape == b.shape and bool(torch.equal(bits(a.cpu()), bits(b.cpu())))


def gen(dtype, rank, length=L):
    """Rank `rank`'s input: floats span about 2^+-20 in magnitude (2^+-4 for fp16) so the order of
    addition shows in the bits; a quarter of the elements are +0 (the logical ops need both)."""
    g = torch.Generator().manual_seed((1000 * rank + 7 + FLOATS.index(dtype)) if dtype in FLOATS else 500 + rank)
    if dtype in FLOATS:
        e = 4 if dtype == torch.float16 else 20
        x = torch.randn(length, generator=g, dtype=torch.float64) * \
            torch.pow(2.0, torch.randint(-e, e + 1, (length,), generator=g).double())
        x[torch.rand(length, generator=g) < 0.25] = 0.0
        return x.to(dtype)
    if dtype == torch.uint8:
        return torch.randint(0, 256, (length,), generator=g, dtype=torch.int64).to(torch.uint8)
    return torch.randint(-50, 51, (length,), generator=g, dtype=torch.int64).to(dtype)


def fold(parts, op, dtype):
    """((p0 op p1) op p2) ... on the CPU; 16-bit floats in fp32, one cast at the end."""
    wide = torch.float32 if dtype in (torch.bfloat16, torch.float16) else dtype
    acc = parts[0].to(wide)
    for p in parts[1:]:
        acc = op(acc, p.to(wide))
    return acc.to(dtype)


INPUTS, SYM = {}, {}


def inputs(dt):
    if dt not in INPUTS:
        INPUTS[dt] = [gen(dt, q) for q in range(n)]  # (deterministic: every rank builds all of them ...)
        got = W.allgather_obj(INPUTS[dt][r][:4096])  # ... and checks them against what the ranks hold
        assert all(same(a, b[:4096]) for a, b in zip(got, INPUTS[dt]))
    return INPUTS[dt]


def sym(dt):
    """One registered buffer per dtype, shared by the cases."""
    if dt not in SYM:
        SYM[dt] = W.sym_alloc(L, dt, device=on_gpu)
    return SYM[dt]


def load(dt):
    """(the registered buffer holding my input, my input on the host)"""
    buf, mine = sym(dt), inputs(dt)[r]
    buf.copy_(mine.to(dev))
    return buf, mine


class Stats:
    """coll_stats() of one collective around a block of calls: all of them by window, staged or
    not as stated, none fell back."""

    def __init__(self, comm, name, staged):
        self.comm, self.name, self.staged, self.calls = comm, name, staged, 0

    def __enter__(self):
        self.before = self.comm.coll_stats()[self.name]
        return self

    def __exit__(self, *exc):
        if exc[0] is None:
            a, b = self.comm.coll_stats()[self.name], self.before
            assert a["window"] - b["window"] == self.calls and a["fallback"] == 0, (self.name, b, a, self.calls)
            assert a["window_staged"] - b["window_staged"] == (self.calls if self.staged else 0), (self.name, b, a)


def out_buf(dt, cnt, pad=2):
    """A plain destination of cnt elements with `pad` zero guard elements on both sides."""
    o = torch.zeros(cnt + 2 * pad, dtype=dt, device=dev)
    return o, o[pad: pad + cnt]


def guards_zero(o, cnt, pad=2):
    return not bool(o[:pad].any()) and not bool(o[pad + cnt:].any())


def uneven(c):
    """Per-rank counts, all different, rank 1's zero; their sum is at most n * c."""
    return [0 if q == 1 else c // (q + 1) + q for q in range(n)] if c > 2 * n else [0 if q == 1 else c for q in range(n)]


MISALIGNED = [False]  # a pair (source, destination) whose distance is no multiple of 16 bytes was seen


def note_mis(src_addr, dst_addr):
    if (src_addr - dst_addr) % 16:
        MISALIGNED[0] = True


# ---- 1 reduce-scatter and all-gather(v)
def run_reduce_scatter(staged):
    for op, dt in FOLDS:
        xs = inputs(dt)
        buf, mine = load(dt)
        with Stats(W, "reduce_scatter", staged) as st:
            for off in (OFFS if not staged else [1]):
                for c in COUNTS:
                    for counts in ([c] * n, uneven(c)):
                        lo, total, d0 = G + off, sum(counts), sum(counts[:r])
                        send = xs[r][lo: lo + total].clone().to(dev) if staged else buf[lo: lo + total]
                        o, recv = out_buf(dt, counts[r])
                        if counts == [c] * n and off == 1:
                            W.Reduce_scatter_block(send, recv, op, algo="window")
                        else:
                            W.Reduce_scatter(send, recv, counts, op, algo="window")
                        st.calls += 1
                        exp = fold([x[lo + d0: lo + d0 + counts[r]] for x in xs], op, dt)
                        tag = ("reduce_scatter", staged, op.name, dt, off, counts)
                        assert same(recv, exp) and guards_zero(o, counts[r]), tag
                        assert same(send, xs[r][lo: lo + total]), (tag, "sendbuf modified")
                        if counts[r]:
                            note_mis(C.Comm._addr(send) + d0 * send.element_size(), recv.data_ptr())
        assert same(buf, mine), "registered buffer modified"
        try:
            W.Reduce_scatter(buf[G: G + 4 * n], buf[G + 1: G + 5], None, op, algo="window")
            raise AssertionError("overlapping recvbuf accepted")
        except ValueError:
            pass


def run_allgather(staged):
    for dt in (torch.float32, torch.bfloat16, torch.uint8):
        xs = inputs(dt)
        buf, mine = load(dt)
        with Stats(W, "allgather", staged) as st:
            for off in (OFFS if not staged else [3]):
                for c in COUNTS:
                    for counts in ([c] * n, uneven(c)):
                        lo, total = G + off, sum(counts)
                        displs = [sum(counts[:q]) for q in range(n)]
                        send = xs[r][lo: lo + counts[r]].clone().to(dev) if staged else buf[lo: lo + counts[r]]
                        o, recv = out_buf(dt, total, pad=3)
                        if counts == [c] * n:
                            W.Allgather(send, recv, algo="window")
                        else:
                            W.Allgatherv(send, recv, counts, None, algo="window")
                        st.calls += 1
                        exp = torch.cat([xs[q][lo: lo + counts[q]] for q in range(n)])
                        tag = ("allgather", staged, dt, off, counts)
                        assert same(recv, exp) and guards_zero(o, total, 3), tag
                        assert same(send, xs[r][lo: lo + counts[r]]), (tag, "sendbuf modified")
                        for q in range(n):
                            if counts[q]:
                                note_mis(C.Comm._addr(send), recv.data_ptr() + displs[q] * recv.element_size())
            if not staged:  # in place: my segment of the symmetric recvbuf is my contribution
                for off in OFFS:
                    for c in COUNTS:
                        lo = G + off
                        buf.copy_(mine.to(dev))
                        W.Allgather(buf[lo + r * c: lo + (r + 1) * c], buf[lo: lo + n * c], algo="window")
                        st.calls += 1
                        exp = mine.clone()
                        for q in range(n):
                            exp[lo + q * c: lo + (q + 1) * c] = xs[q][lo + q * c: lo + (q + 1) * c]
                        assert same(buf, exp), ("allgather in place", dt, off, c)
                buf.copy_(mine.to(dev))
        assert same(buf, mine), "registered buffer modified"


if "rs_ag" in cases:
    for staged in (False, True):
        run_reduce_scatter(staged)
        run_allgather(staged)
    assert MISALIGNED[0], "no pair with (src - dst) * element size mod 16 != 0 was exercised"
    ok("rs_ag")


# ---- 2 scan and exscan: in place on the registered buffer, out of place through the staging window
if "scan" in cases:
    for op, dt in FOLDS + [(C.PROD, torch.float64)]:
        xs = inputs(dt)
        buf, mine = load(dt)
        for excl in (False, True):
            call = W.Exscan if excl else W.Scan
            name = "exscan" if excl else "scan"
            with Stats(W, name, False) as st:
                for off in OFFS:
                    for c in COUNTS:
                        lo = G + off
                        buf.copy_(mine.to(dev))
                        call(buf[lo: lo + c], buf[lo: lo + c], op, algo="window")
                        st.calls += 1
                        exp = mine.clone()
                        if not (excl and r == 0):
                            exp[lo: lo + c] = fold([x[lo: lo + c] for x in xs[: (r if excl else r + 1)]], op, dt)
                        assert same(buf, exp), (name, "in place", op.name, dt, off, c)
            with Stats(W, name, True) as st:
                for c in COUNTS:
                    lo = G + 1
                    send = xs[r][lo: lo + c].clone().to(dev)
                    o = torch.full((c + 4,), 7, dtype=dt, device=dev)
                    call(send, o[2: 2 + c], op, algo="window")
                    st.calls += 1
                    exp = torch.full((c + 4,), 7, dtype=dt)  # rank 0 of Exscan keeps the sentinel
                    if not (excl and r == 0):
                        exp[2: 2 + c] = fold([x[lo: lo + c] for x in xs[: (r if excl else r + 1)]], op, dt)
                    assert same(o, exp), (name, "out of place", op.name, dt, c)
                    assert same(send, xs[r][lo: lo + c]), (name, "sendbuf modified")
    ok("scan")


# ---- 3 all-to-all for element sizes 1, 2, 4 and 8
if "a2a" in cases:
    for dt in (torch.uint8, torch.bfloat16, torch.float32, torch.int64):
        xs = inputs(dt)
        buf, mine = load(dt)
        for staged in (False, True):
            with Stats(W, "alltoall", staged) as st:
                for off in (OFFS if not staged else [1]):
                    for c in COUNTS:
                        lo = G + off
                        send = xs[r][lo: lo + n * c].clone().to(dev) if staged else buf[lo: lo + n * c]
                        o, recv = out_buf(dt, n * c, pad=3)
                        W.Alltoall(send, recv, algo="window")
                        st.calls += 1
                        exp = torch.cat([xs[q][lo + r * c: lo + (r + 1) * c] for q in range(n)])
                        assert same(recv, exp) and guards_zero(o, n * c, 3), ("alltoall", staged, dt, off, c)
                        assert same(send, xs[r][lo: lo + n * c]), ("alltoall", "sendbuf modified")
        assert same(buf, mine), "registered buffer modified"
    ok("a2a")


# ---- 4 broadcast and reduce from a non-zero root
if "rooted" in cases:
    root = n - 1
    for dt in (torch.float32, torch.uint8):
        xs = inputs(dt)
        for staged in (False, True):
            buf, mine = load(dt)
            with Stats(W, "bcast", staged) as st:
                for off in (OFFS if not staged else [3]):
                    for c in COUNTS:
                        lo = G + off
                        if staged:
                            o = torch.zeros(c + 6, dtype=dt, device=dev)
                            o[3: 3 + c].copy_(xs[r][lo: lo + c])
                            W.Bcast(o[3: 3 + c], root, algo="window")
                            assert same(o[3: 3 + c], xs[root][lo: lo + c]) and guards_zero(o, c, 3), ("bcast", dt, c)
                        else:
                            buf.copy_(mine.to(dev))
                            W.Bcast(buf[lo: lo + c], root, algo="window")
                            exp = mine.clone()
                            exp[lo: lo + c] = xs[root][lo: lo + c]
                            assert same(buf, exp), ("bcast", dt, off, c)
                        st.calls += 1
    root = 1
    for op, dt in FOLDS:
        xs = inputs(dt)
        buf, mine = load(dt)
        for staged in (False, True):
            with Stats(W, "reduce", staged) as st:
                for off in (OFFS if not staged else [1]):
                    for c in COUNTS:
                        lo = G + off
                        send = xs[r][lo: lo + c].clone().to(dev) if staged else buf[lo: lo + c]
                        o, recv = out_buf(dt, c)
                        W.Reduce(send, recv if r == root else None, op, root, algo="window")
                        st.calls += 1
                        if r == root:
                            assert same(recv, fold([x[lo: lo + c] for x in xs], op, dt)), ("reduce", op.name, dt, off, c)
                        assert not bool(o.any()) or r == root, "a non-root recvbuf was written"
                        assert guards_zero(o, c) and same(send, xs[r][lo: lo + c]), ("reduce", "guards / sendbuf")
        assert same(buf, mine), "registered buffer modified"
    ok("rooted")


# ---- 5 FIFO: a mixed sequence of non-blocking calls on the staging path, waited in reverse order
if "fifo" in cases:
    dt, c = torch.float32, 30011  # (n * c fp32: several pieces of the 64 KiB staging window)
    xs = inputs(dt)
    reqs, checks = [], []
    s_ar, s_co = W.ar_stats(), W.coll_stats()
    for k in range(2):
        lo = G + k
        a = xs[r][lo: lo + c].clone().to(dev)
        reqs.append(W.Iallreduce(a, None, C.SUM, algo="window"))
        checks.append((a, fold([x[lo: lo + c] for x in xs], C.SUM, dt)))
        send = xs[r][lo: lo + n * c].clone().to(dev)
        recv = torch.zeros(c, dtype=dt, device=dev)
        reqs.append(W.Ireduce_scatter(send, recv, None, C.SUM, algo="window"))
        checks.append((recv, fold([x[lo + r * c: lo + (r + 1) * c] for x in xs], C.SUM, dt)))
        g_out = torch.zeros(n * 1031, dtype=dt, device=dev)
        reqs.append(W.Iallgather(xs[r][lo: lo + 1031].clone().to(dev), g_out, algo="window"))
        checks.append((g_out, torch.cat([x[lo: lo + 1031] for x in xs])))
        t_out = torch.zeros(n * c, dtype=dt, device=dev)
        reqs.append(W.Ialltoall(send, t_out, algo="window"))
        checks.append((t_out, torch.cat([x[lo + r * c: lo + (r + 1) * c] for x in xs])))
        if k == 0:
            b = xs[r][:777].clone().to(dev)
            W.Bcast(b, n - 1, algo="window")  # blocking: ordered behind the four before it
            assert same(b, xs[n - 1][:777])
            assert all(q.Test() for q in reqs), "a blocking call returned before an earlier ticket"
        W.Barrier()
        assert W.allgather_obj(("fifo", k, r)) == [("fifo", k, q) for q in range(n)]
    rb = xs[r][:99].clone().to(dev)
    reqs.append(W.Ibcast(rb, 1, algo="window"))
    checks.append((rb, xs[1][:99]))
    ro = torch.zeros(99, dtype=dt, device=dev)
    reqs.append(W.Ireduce(xs[r][:99].clone().to(dev), ro if r == 0 else None, C.MAX, 0, algo="window"))
    if r == 0:
        checks.append((ro, fold([x[:99] for x in xs], C.MAX, dt)))
    for q in reversed(reqs):
        q.Wait()
        assert q.Test()
    for got, exp in checks:
        assert same(got, exp)
    e_ar, e_co = W.ar_stats(), W.coll_stats()
    assert e_ar["window"] - s_ar["window"] == 2 and e_ar["window_staged"] - s_ar["window_staged"] == 2
    for name, k in (("reduce_scatter", 2), ("allgather", 2), ("alltoall", 2), ("bcast", 2), ("reduce", 1)):
        assert e_co[name]["window"] - s_co[name]["window"] == k and e_co[name]["fallback"] == 0, (name, s_co, e_co)
        assert e_co[name]["window_staged"] - s_co[name]["window_staged"] == k, (name, s_co, e_co)
    ok("fifo")


# ---- 6 sub-communicators: {0,1} and {2,3} run reduce-scatter and all-gather at the same time
if "subcomm" in cases and n == 4:
    S = W.Split(r // 2, r)
    sr, base = S.Get_rank(), 2 * (r // 2)
    LS = G + 2 * max(COUNTS) + G
    sb = S.sym_alloc(LS, torch.float32, device=on_gpu)
    for k, c in enumerate(COUNTS * 2):
        parts = [gen(torch.float32, base + q)[:LS] for q in range(2)]
        sb.copy_(parts[sr].to(dev))
        op = (C.SUM, C.MAX, C.PROD)[k % 3]
        shard = torch.zeros(c, device=dev)
        S.Reduce_scatter(sb[G: G + 2 * c], shard, None, op, algo="window")
        assert same(shard, fold([p[G + sr * c: G + (sr + 1) * c] for p in parts], op, torch.float32)), (k, c)
        S.Allgather(sb[G + sr * c: G + (sr + 1) * c], sb[G: G + 2 * c], algo="window")
        exp = parts[sr].clone()
        exp[G + (1 - sr) * c: G + (2 - sr) * c] = parts[1 - sr][G + (1 - sr) * c: G + (2 - sr) * c]
        assert same(sb, exp), (k, c)
    cs = S.coll_stats()
    for name in ("reduce_scatter", "allgather"):
        assert cs[name] == {"window": 2 * len(COUNTS), "window_staged": 0, "fallback": 0}, cs
    S.sym_free(sb)
    assert S._sym == []
    ok("subcomm")


# ---- 7 two ranks: a fold of two is order-free, so Scan by window equals Scan by p2p bit for bit
if "p2p" in cases and n == 2:
    for dt in (torch.float32, torch.bfloat16):
        xs = inputs(dt)
        for c in COUNTS:
            x = xs[r][G: G + c].clone().to(dev)
            a, b = torch.zeros(c, dtype=dt, device=dev), torch.zeros(c, dtype=dt, device=dev)
            W.Scan(x, a, C.SUM, algo="window")
            W.Scan(x, b, C.SUM, algo="p2p")
            assert same(a, b), ("scan window != p2p", dt, c)
    assert W.coll_stats()["scan"]["fallback"] == 0
    ok("p2p")


# ---- 8 the sharded step's identity: Reduce_scatter, then Allgather in place on one symmetric
# buffer == Allreduce(algo="window") on a copy, bit for bit
if "sharded" in cases:
    for op, dt in FOLDS:
        buf, mine = load(dt)
        for off in OFFS:
            for c in COUNTS:
                lo = G + off
                buf.copy_(mine.to(dev))
                ref = buf[lo: lo + n * c].clone()
                W.Allreduce(ref, None, op, algo="window")
                shard = torch.zeros(c, dtype=dt, device=dev)
                W.Reduce_scatter(buf[lo: lo + n * c], shard, None, op, algo="window")
                buf[lo + r * c: lo + (r + 1) * c].copy_(shard)  # (the sharded optimizer step goes here)
                W.Allgather(buf[lo + r * c: lo + (r + 1) * c], buf[lo: lo + n * c], algo="window")
                assert same(buf[lo: lo + n * c], ref), ("sharded", op.name, dt, off, c)
                assert same(buf[:lo], mine[:lo]) and same(buf[lo + n * c:], mine[lo + n * c:]), "guards"
    cs = W.coll_stats()
    assert cs["reduce_scatter"]["fallback"] == 0 and cs["allgather"]["fallback"] == 0, cs
    ok("sharded")

for t in list(SYM.values()):
    W.sym_free(t)
W.sym_free()  # the staging buffers
assert W._sym == []
W.Barrier()
if r == 0:
    print("ALL_DONE", flush=True)
mp.Finalize()
