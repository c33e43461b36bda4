"""Window all-reduce (csrc/kernels/allreduce.hip, csrc/core/window.cpp Window::allreduce,
comm.py "window all-reduce") on n ranks under torch.distributed.run; T_DEVICE=cuda: the ranks
share the box's GPU and the buffers are HBM, otherwise host shm windows and the host twin.

Every comparison is bitwise against the left fold in rank order, computed on the CPU from the
inputs gathered with allgather_obj (16-bit floats: folded in fp32, cast once). Each case prints
``OK <case>`` on rank 0. Cases (T_CASES, comma separated; default all that fit the rank count):
grid, modes, staged, fifo, subcomm, routing."""
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
cases = os.environ.get("T_CASES", "grid,modes,staged,fifo,subcomm,routing").split(",")

G = 4  # guard elements on both sides of the largest range
COUNTS = [1, 3, n * 4 - 1, 1031, 65541]
OFFS = [0, 1, 3]
L = G + max(OFFS) + max(COUNTS) + G
FLOATS = [torch.float32, torch.bfloat16, torch.float16, torch.float64]
INTS = [torch.int32, torch.int64, torch.uint8]
OPS_ALL = [C.SUM, C.PROD, C.MAX, C.MIN, C.LAND, C.LOR, C.LXOR]
OPS_INT = [C.BAND, C.BOR, C.BXOR]
BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


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


def pairs():
    for dt in FLOATS + INTS:
        for op in OPS_ALL + (OPS_INT if dt in INTS else []):
            yield op, dt


INPUTS, EXPECT = {}, {}


def inputs(dt):
    if dt not in INPUTS:
        INPUTS[dt] = [gen(dt, q) for q in range(n)]  # (deterministic: every rank builds all of them ...)
        got = W.allgather_obj(INPUTS[dt][r])  # ... and checks them against what the ranks hold
        assert all(same(a, b) for a, b in zip(got, INPUTS[dt]))
    return INPUTS[dt]


def expect(op, dt):
    if (op.name, dt) not in EXPECT:
        EXPECT[(op.name, dt)] = fold(inputs(dt), op, dt)
    return EXPECT[(op.name, dt)]


SYM = {}


def sym(dt):
    """One registered buffer per dtype, shared by the cases."""
    if dt not in SYM:
        SYM[dt] = W.sym_alloc(L, dt, device=on_gpu)
        assert SYM[dt].numel() == L and SYM[dt].dtype == dt and SYM[dt].device.type == dev.type
    return SYM[dt]


def run_grid(tag, pair_list, dest=False):
    """Every (op, dtype) of pair_list x COUNTS x OFFS in place on the registered buffer (dest: out
    of place into an unregistered tensor): result == fold, everything else unchanged."""
    for op, dt in pair_list:  # (collective set-up first: creating a window is itself an all-reduce)
        sym(dt), expect(op, dt)
    before = W.ar_stats()
    calls = 0
    for op, dt in pair_list:
        buf, mine, exp = sym(dt), inputs(dt)[r].to(dev), expect(op, dt)
        for off in OFFS:
            for cnt in COUNTS:
                lo = G + off
                buf.copy_(mine)
                if dest:
                    out = torch.zeros(cnt + 2, dtype=dt, device=dev)
                    W.Allreduce(buf[lo:lo + cnt], out[1:1 + cnt], op, algo="window")
                    assert same(buf, mine), (tag, op.name, dt, off, cnt, "source modified")
                    assert same(out[1:1 + cnt], exp[lo:lo + cnt]), (tag, op.name, dt, off, cnt)
                    assert float(out[0]) == 0 and float(out[-1]) == 0, (tag, op.name, dt, off, cnt, "guards")
                else:
                    W.Allreduce(buf[lo:lo + cnt], None, op, algo="window")
                    got = buf.cpu()
                    assert same(got[lo:lo + cnt], exp[lo:lo + cnt]), (tag, op.name, dt, off, cnt)
                    assert same(got[:lo], mine[:lo]) and same(got[lo + cnt:], mine[lo + cnt:]), \
                        (tag, op.name, dt, off, cnt, "guards")
                calls += 1
    after = W.ar_stats()
    assert after["window"] - before["window"] == calls and after["p2p"] == before["p2p"], (before, after)
    assert after["window_staged"] == before["window_staged"], (before, after)


def forced(nbytes):
    W._ar_drain()
    if nbytes is None:
        os.environ.pop("MPIT_AR_ONESHOT_BYTES", None)
    else:
        os.environ["MPIT_AR_ONESHOT_BYTES"] = str(nbytes)


nat = mp._ext.native()
assert nat.peer_reduce_supported(0, 0) and not nat.peer_reduce_supported(7, 0) and nat.peer_reduce_supported(7, 4)
assert not nat.peer_reduce_supported(10, 0) and not nat.peer_reduce_supported(0, 7)

# ---- 1 kernel grid: every supported (op, dtype), two-shot (slices, empty ones when count < n)
if "grid" in cases:
    forced(0)
    run_grid("two-shot", list(pairs()))
    forced(None)
    # NaN propagates through MAX / MIN like torch.maximum / torch.minimum
    for dt in (torch.float32, torch.bfloat16):
        buf = sym(dt)
        buf.copy_(inputs(dt)[r].to(dev))
        if r == n - 1:
            buf[G + 5] = float("nan")
        for op in (C.MAX, C.MIN):
            W.Allreduce(buf[G:G + 64], None, op, algo="window")
            assert bool(torch.isnan(buf[G + 5])) and int(torch.isnan(buf[G:G + 64]).sum()) == 1, (op.name, dt)
    ok("grid")

# ---- 2 one-shot == two-shot, in place and into a different destination
if "modes" in cases:
    forced(1 << 40)
    run_grid("one-shot", list(pairs()))
    run_grid("one-shot-dest", [(C.SUM, dt) for dt in FLOATS + INTS] + [(C.MAX, torch.float32)], dest=True)
    forced(None)
    ok("modes")

# ---- 3 staged: unregistered tensors, sendbuf != recvbuf, several chunks of the staging buffer
if "staged" in cases:
    assert float(os.environ["MPIT_AR_STAGE_MB"]) * (1 << 20) == 64 << 10
    m = 76801  # ~300 KiB of fp32: five chunks of 64 KiB
    xs = [gen(torch.float32, q, m) for q in range(n)]
    x, y = xs[r].to(dev), torch.zeros(m, device=dev)
    s0 = W.ar_stats()
    W.Allreduce(x, y, C.SUM, algo="window")
    s1 = W.ar_stats()
    assert same(y, fold(xs, C.SUM, torch.float32)) and same(x, xs[r]), "staged"
    assert s1["window_staged"] == s0["window_staged"] + 1 and s1["window"] == s0["window"] + 1, (s0, s1)
    x16 = [gen(torch.bfloat16, q, m) for q in range(n)]
    z = x16[r].clone().to(dev)
    W.Allreduce(z, None, C.SUM, algo="window")  # unregistered, in place
    assert same(z, fold(x16, C.SUM, torch.bfloat16))
    ok("staged")

# ---- 4 FIFO: six non-blocking calls of different sizes and dtypes, a blocking one in between,
# waited in reverse order, while the main thread runs Barrier and allgather_obj
if "fifo" in cases:
    specs = [(torch.float32, 65541, True), (torch.bfloat16, 1031, True), (torch.int32, 3, False),
             (torch.float64, 4099, False), (torch.uint8, 11, True), (torch.float16, 30011, False)]
    reqs, checks = [], []
    for k, (dt, cnt, registered) in enumerate(specs):
        src = [gen(dt, q, cnt) if not registered else inputs(dt)[q][G:G + cnt] for q in range(n)]
        if registered:
            sym(dt).copy_(inputs(dt)[r].to(dev))
            t = sym(dt)[G:G + cnt]
        else:
            t = src[r].clone().to(dev)
        reqs.append(W.Iallreduce(t, None, C.SUM, algo="window"))
        checks.append((t, fold(src, C.SUM, dt)))
        if k == 2:
            mid = [gen(torch.int64, q, 777) for q in range(n)]
            b = mid[r].clone().to(dev)
            W.Allreduce(b, None, C.MAX, algo="window")  # blocking: ordered behind the three before it
            assert same(b, fold(mid, C.MAX, torch.int64))
            assert all(q.Test() for q in reqs), "a blocking call returned before an earlier ticket"
        W.Barrier()
        assert W.allgather_obj(("fifo", k, r)) == [("fifo", k, q) for q in range(n)]
    for q in reversed(reqs):
        q.Wait()
        assert q.Test()
    for t, exp in checks:
        assert same(t, exp)
    ok("fifo")

# ---- 5 sub-communicators: {0,1} and {2,3} run window all-reduces at the same time
if "subcomm" in cases and n == 4:
    S = W.Split(r // 2, r)
    sr, base = S.Get_rank(), 2 * (r // 2)
    sb = S.sym_alloc(L, torch.float32, device=on_gpu)
    for k, cnt in enumerate(COUNTS * 3):
        parts = [gen(torch.float32, base + q)[:G + cnt] for q in range(2)]
        sb[:G + cnt].copy_(parts[sr].to(dev))
        op = (C.SUM, C.MAX, C.PROD)[k % 3]
        S.Allreduce(sb[G:G + cnt], None, op, algo="window")
        assert same(sb[G:G + cnt], fold(parts, op, torch.float32)[G:]) and same(sb[:G], parts[sr][:G]), (k, cnt)
    assert S.ar_stats()["window"] == 3 * len(COUNTS) and S.ar_stats()["window_staged"] == 0
    S.sym_free(sb)
    assert S._sym == []
    ok("subcomm")

# ---- 6 routing: MPIT_ALLREDUCE=window takes the window path (rank-order fold, bit for bit);
# with the variable unset nothing goes there
if "routing" in cases:
    assert os.environ.get("MPIT_ALLREDUCE") == "window"
    xs = inputs(torch.float32)
    x, y = xs[r].to(dev), torch.zeros(L, device=dev)
    s0 = W.ar_stats()
    W.Allreduce(x, y, C.SUM)
    s1 = W.ar_stats()
    assert s1["window"] == s0["window"] + 1 and s1["p2p"] == s0["p2p"], (s0, s1)
    assert same(y, fold(xs, C.SUM, torch.float32)), "MPIT_ALLREDUCE=window: not the rank-order fold"
    q = W.Iallreduce(x, y, C.MAX)
    q.Wait()
    assert W.ar_stats()["window"] == s1["window"] + 1 and same(y, fold(xs, C.MAX, torch.float32))
    del os.environ["MPIT_ALLREDUCE"]
    s2 = W.ar_stats()
    W.Allreduce(x, y, C.SUM)
    W.Iallreduce(x, y, C.SUM).Wait()
    s3 = W.ar_stats()
    assert s3["window"] == s2["window"] and s3["p2p"] + s3["rccl"] == s2["p2p"] + s2["rccl"] + 2, (s2, s3)
    # (any summation order: within n roundings of the sum of magnitudes)
    ref, mag = sum(t.double() for t in xs), sum(t.double().abs() for t in xs)
    assert bool(((y.cpu().double() - ref).abs() <= n * 2.0 ** -23 * mag).all())
    os.environ["MPIT_ALLREDUCE"] = "window"
    ok("routing")

for t in list(SYM.values()):
    W.sym_free(t)
W.sym_free()  # the staging buffers
assert W._sym == []
W.Barrier()
if r == 0:
    print("ALL_DONE", flush=True)
mp.Finalize()
