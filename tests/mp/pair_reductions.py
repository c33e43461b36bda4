"""MAXLOC / MINLOC between ranks, on n ranks under torch.distributed.run; T_DEVICE=cuda: the ranks
share the box's GPU and the buffers are HBM, otherwise host shm windows and the host twins.

Every rank gathers all inputs with allgather_obj and folds them on the CPU with the oracle of
tests/test_pair_kernels.py (the rule in its three steps, left fold in rank order); every
comparison is bitwise on whole pairs. The collectives run with algo="window" on registered
symmetric memory, in place and out of place, and on plain tensors (staged through the 64 KiB
staging window in pieces); ar_stats / coll_stats must show them there, and the same calls with
algo="p2p" must give the same bytes. Each case prints ``OK <case>`` on rank 0. Cases (T_CASES):
allreduce, rooted, rs, scan, facade, onesided, errors, k1."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np
import torch

import mpit_amd as mp
from mpit_amd import comm as C
from mpit_amd import datatypes as dt
from mpit_amd import mpiT
from mpit_amd.comm import COMM_WORLD
from test_pair_kernels import KIND, LAYOUTS, enc, gen, takes_b

mp.Init()
W = COMM_WORLD()
r, n = W.Get_rank(), W.Get_size()
on_gpu = os.environ.get("T_DEVICE", "cpu") == "cuda"
dev = mp.runtime.device() if on_gpu else torch.device("cpu")
cases = os.environ.get("T_CASES", "allreduce,rooted,rs,scan,facade,onesided,errors,k1").split(",")
assert float(os.environ["MPIT_AR_STAGE_MB"]) * (1 << 20) == 64 << 10

# 16384 pairs: a third of them is no whole number; 5003: nor is any even cut. At three ranks an
# element-wise cut of a slice, and a 64 KiB staging piece of the 16-byte pairs, would split a pair
PAIRS = [16384, 5003]
PMAX = max(PAIRS)
PAIRTYPE = {"float_int": dt.FLOAT_INT, "double_int": dt.DOUBLE_INT, "long_int": dt.LONG_INT}
OPS = {"MAXLOC": C.MAXLOC, "MINLOC": C.MINLOC}


def ok(name):
    W.Barrier()
    if r == 0:
        print("OK", name, flush=True)


def tdtype(lname):
    """Interleaved pairs live in a tensor of their dtype, struct pairs in their bytes."""
    return torch.uint8 if lname in PAIRTYPE else KIND[LAYOUTS[lname][1]]


def to_tensor(lname, raw):
    return torch.from_numpy(np.ascontiguousarray(raw).reshape(-1)).view(tdtype(lname))


def raw_of(lname, t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().reshape(-1, LAYOUTS[lname][4])


def per_pair(lname):
    return LAYOUTS[lname][4] // to_tensor(lname, np.zeros((1, LAYOUTS[lname][4]), np.uint8)).element_size()


INPUTS, PREFIX, SYM = {}, {}, {}
# (the staging window comes into being with the first staged call, which agrees on it with an
# all-reduce of its own: have that behind us before any case counts calls)
W.Allreduce(torch.zeros(2, device=dev), None, C.MAXLOC, algo="window")


def inputs(lname):
    if lname not in INPUTS:
        mine = gen(lname, r, PMAX)
        INPUTS[lname] = W.allgather_obj(mine)  # every rank folds what the ranks really hold
        assert np.array_equal(INPUTS[lname][r], mine)
    return INPUTS[lname]


def prefix(lname, oname):
    """prefix[j] = the left fold of ranks 0..j over PMAX pairs, [PMAX, extent] bytes."""
    if (lname, oname) not in PREFIX:
        out, acc = [], None
        for s in inputs(lname):
            acc = s if acc is None else np.where(takes_b(lname, acc, s, oname == "MAXLOC")[:, None], s, acc)
            out.append(acc)
        PREFIX[lname, oname] = out
    return PREFIX[lname, oname]


def sym(lname):
    """(registered input buffer, registered output buffer), PMAX pairs each"""
    if lname not in SYM:
        k = PMAX * per_pair(lname)
        SYM[lname] = (W.sym_alloc(k, tdtype(lname), device=on_gpu), W.sym_alloc(k, tdtype(lname), device=on_gpu))
    return SYM[lname]


def mine(lname, p):
    return to_tensor(lname, inputs(lname)[r][:p]).clone().to(dev)  # (a copy: the inputs stay as gathered)


def eq(lname, t, rows, tag):
    got = raw_of(lname, t)
    assert got.shape == rows.shape and np.array_equal(got, rows), (tag, np.flatnonzero((got != rows).any(1))[:6])


def ar_delta(before, calls, staged):
    a = W.ar_stats()
    assert a["window"] - before["window"] == calls and a["window_staged"] - before["window_staged"] == staged and \
        a["p2p"] == before["p2p"], (before, a, calls, staged)


class Stats:
    """coll_stats() of one collective around a block of calls: all by window, none fell back."""

    def __init__(self, name, calls, staged):
        self.name, self.calls, self.staged = name, calls, staged

    def __enter__(self):
        self.before = W.coll_stats()[self.name]

    def __exit__(self, *exc):
        if exc[0] is None:
            a, b = W.coll_stats()[self.name], self.before
            assert a["window"] - b["window"] == self.calls and a["fallback"] == b["fallback"], (self.name, b, a)
            assert a["window_staged"] - b["window_staged"] == self.staged, (self.name, b, a)


def each():
    for i, lname in enumerate(LAYOUTS):
        yield lname, ("MAXLOC", "MINLOC")[i % 2], PAIRTYPE.get(lname)


# ------------------------------------------------------------------ Allreduce, Iallreduce
if "allreduce" in cases:
    for lname, oname, pt in each():
        op, pp = OPS[oname], per_pair(lname)
        sin, sout = sym(lname)
        for p in PAIRS:
            want = prefix(lname, oname)[n - 1][:p]
            tag = ("allreduce", lname, oname, p)
            b = W.ar_stats()
            v = sin[: p * pp]
            v.copy_(mine(lname, p))
            assert W.Allreduce(v, None, op, algo="window", pairtype=pt) is v  # symmetric, in place: direct
            eq(lname, v, want, (tag, "in place"))
            ar_delta(b, 1, 0)
            v.copy_(mine(lname, p))
            o = sout[: p * pp]
            o.zero_()
            W.Allreduce(v, o, op, algo="window", pairtype=pt)  # symmetric, out of place
            eq(lname, o, want, (tag, "out of place"))
            eq(lname, v, inputs(lname)[r][:p], (tag, "sendbuf kept"))
            x, y = mine(lname, p), torch.zeros_like(mine(lname, p))
            b = W.ar_stats()
            W.Allreduce(x, y, op, algo="window", pairtype=pt)  # plain tensors: staged in pieces
            eq(lname, y, want, (tag, "staged"))
            req = W.Iallreduce(x, x, op, algo="window", pairtype=pt)
            req.Wait()
            eq(lname, x, want, (tag, "Iallreduce staged in place"))
            ar_delta(b, 2, 2)
            x, y = mine(lname, p), torch.zeros_like(mine(lname, p))
            W.Allreduce(x, y, op, algo="p2p", pairtype=pt)  # the tree gives the same bytes, for any k
            eq(lname, y, want, (tag, "p2p"))
            assert W.ar_stats()["p2p"] == b["p2p"] + 1
    # buffers aligned to the pair's largest member only (4 mod 8, 8 mod 16): any such tensor will do
    for lname, off in (("f32x2", 4), ("float_int", 4), ("double_int", 8), ("i64x2", 8)):
        pt, p, ext = PAIRTYPE.get(lname), 1031, LAYOUTS[lname][4]
        want = prefix(lname, "MAXLOC")[n - 1][:p]

        def odd():
            raw = torch.zeros(16 + off + p * ext, dtype=torch.uint8, device=dev)
            v = raw[16 + off: 16 + off + p * ext]
            v.copy_(mine(lname, p).view(torch.uint8))
            assert v.data_ptr() % ext == off
            return v.view(tdtype(lname))
        x, y = odd(), odd()
        y.zero_()
        b = W.ar_stats()
        assert W.Allreduce(x, y, C.MAXLOC, algo="window", pairtype=pt) is y
        eq(lname, y, want, ("allreduce", lname, off, "member-aligned"))
        eq(lname, x, inputs(lname)[r][:p], ("allreduce", lname, off, "sendbuf kept"))
        W.Iallreduce(x, None, C.MAXLOC, algo="window", pairtype=pt).Wait()
        eq(lname, x, want, ("Iallreduce", lname, off, "member-aligned, in place"))
        ar_delta(b, 2, 2)
        x = odd()
        W.Allreduce(x, x, C.MAXLOC, algo="p2p", pairtype=pt)
        eq(lname, x, want, ("allreduce p2p", lname, off, "member-aligned"))
    ok("allreduce")

# ------------------------------------------------------------------ Reduce to every root
if "rooted" in cases:
    for lname, oname, pt in each():
        op, pp, p = OPS[oname], per_pair(lname), 5003
        want = prefix(lname, oname)[n - 1][:p]
        sin, _ = sym(lname)
        for root in range(n):
            tag = ("reduce", lname, oname, root)
            v = sin[: p * pp]
            v.copy_(mine(lname, p))
            out = torch.zeros_like(mine(lname, p)) if r == root else None
            with Stats("reduce", 1, 0):
                W.Reduce(v, out, op, root, algo="window", pairtype=pt)
            x = mine(lname, p)
            out2 = torch.zeros_like(x) if r == root else None
            with Stats("reduce", 1, 1):
                W.Reduce(x, out2, op, root, algo="window", pairtype=pt)
            out3 = torch.zeros_like(x) if r == root else None
            W.Reduce(x, out3, op, root, algo="p2p", pairtype=pt)
            if r == root:
                for o, how in ((out, "symmetric"), (out2, "staged"), (out3, "p2p")):
                    eq(lname, o, want, (tag, how))
    ok("rooted")

# ------------------------------------------------------------------ Reduce_scatter, uneven counts
if "rs" in cases:
    for lname, oname, pt in each():
        op, pp = OPS[oname], per_pair(lname)
        sin, _ = sym(lname)
        for p in PAIRS:
            cnt = [p // n + (7 if q == 0 else 0) for q in range(n)]
            cnt[-1] = p - sum(cnt[:-1])  # uneven, in pairs
            d0 = sum(cnt[:r])
            want = prefix(lname, oname)[n - 1][d0: d0 + cnt[r]]
            given = cnt if pt is not None else [2 * c for c in cnt]  # interleaved: counts of elements
            tag = ("reduce_scatter", lname, oname, p)
            v = sin[: p * pp]
            v.copy_(mine(lname, p))
            o = torch.zeros(cnt[r] * pp, dtype=tdtype(lname), device=dev)
            with Stats("reduce_scatter", 1, 0):
                W.Reduce_scatter(v, o, given, op, algo="window", pairtype=pt)
            eq(lname, o, want, (tag, "symmetric"))
            x, o2 = mine(lname, p), torch.zeros_like(o)
            with Stats("reduce_scatter", 1, 1):
                W.Ireduce_scatter(x, o2, given, op, algo="window", pairtype=pt).Wait()
            eq(lname, o2, want, (tag, "staged"))
            o3 = torch.zeros_like(o)
            W.Reduce_scatter(x, o3, given, op, algo="p2p", pairtype=pt)
            eq(lname, o3, want, (tag, "p2p"))
    ok("rs")

# ------------------------------------------------------------------ Scan, Exscan
if "scan" in cases:
    for lname, oname, pt in each():
        op, pp, p = OPS[oname], per_pair(lname), 5003
        sin, _ = sym(lname)
        pre = prefix(lname, oname)
        for excl in (False, True):
            name = "exscan" if excl else "scan"
            call = W.Exscan if excl else W.Scan
            keep = inputs(lname)[r][:p]
            want = keep if excl and r == 0 else pre[r - 1 if excl else r][:p]  # rank 0 of Exscan: untouched
            tag = (name, lname, oname)
            v = sin[: p * pp]
            v.copy_(mine(lname, p))
            with Stats(name, 1, 0):
                call(v, v, op, algo="window", pairtype=pt)  # symmetric, in place
            eq(lname, v, want, (tag, "in place"))
            x, y = mine(lname, p), mine(lname, p)
            with Stats(name, 1, 1):
                call(x, y, op, algo="window", pairtype=pt)  # staged, out of place
            eq(lname, y, want, (tag, "staged"))
            y2 = mine(lname, p)
            call(x, y2, op, algo="p2p", pairtype=pt)
            eq(lname, y2, want, (tag, "p2p"))
    ok("scan")

# ------------------------------------------------------------------ the mpiT facade: count counts pairs
if "facade" in cases:
    os.environ["MPIT_ALLREDUCE"] = os.environ["MPIT_COLLECTIVES"] = "window"
    for lname, mtype in (("float_int", mpiT.FLOAT_INT), ("double_int", mpiT.DOUBLE_INT), ("long_int", mpiT.LONG_INT),
                         ("i32x2", mpiT.TWOINT)):
        p, pp = 1031, per_pair(lname)
        x = mine(lname, p + 5)  # five pairs more than count: they stay out of it
        y = torch.zeros_like(x)
        b = W.ar_stats()
        assert mpiT.Allreduce(x, y, p, mtype, mpiT.MAXLOC, W) == mpiT.SUCCESS
        ar_delta(b, 1, 1)
        eq(lname, y[: p * pp], prefix(lname, "MAXLOC")[n - 1][:p], ("facade Allreduce", lname))
        assert not y[p * pp:].any()
        y.zero_()
        mpiT.Iallreduce(x, y, p, mtype, mpiT.MINLOC, W).Wait()
        eq(lname, y[: p * pp], prefix(lname, "MINLOC")[n - 1][:p], ("facade Iallreduce", lname))
        y.zero_()
        with Stats("scan", 1, 1):
            mpiT.Scan(x, y, p, mtype, mpiT.MINLOC, W)
        eq(lname, y[: p * pp], prefix(lname, "MINLOC")[r][:p], ("facade Scan", lname))
        y.zero_()
        with Stats("reduce", 1, 1):
            mpiT.Reduce(x, y if r == 1 else None, p, mtype, mpiT.MAXLOC, 1, W)
        if r == 1:
            eq(lname, y[: p * pp], prefix(lname, "MAXLOC")[n - 1][:p], ("facade Reduce", lname))
        cnt = [p // n] * n
        cnt[0] += p - sum(cnt)
        o = torch.zeros(cnt[r] * pp, dtype=x.dtype, device=dev)
        with Stats("reduce_scatter", 1, 1):
            mpiT.Reduce_scatter(x[: p * pp], o, cnt, mtype, mpiT.MAXLOC, W)
        d0 = sum(cnt[:r])
        eq(lname, o, prefix(lname, "MAXLOC")[n - 1][d0: d0 + cnt[r]], ("facade Reduce_scatter", lname))
    del os.environ["MPIT_ALLREDUCE"], os.environ["MPIT_COLLECTIVES"]
    for mtype in (mpiT.SHORT_INT, mpiT.LONG_DOUBLE_INT):
        try:
            z = torch.zeros(64, dtype=torch.uint8)
            mpiT.Allreduce(z, z.clone(), 2, mtype, mpiT.MAXLOC, W)
            raise AssertionError("a pair datatype without kernels accepted")
        except TypeError as e:
            assert mtype._name in str(e), e
    ok("facade")

# ------------------------------------------------------------------ one-sided: every rank onto rank 0
if "onesided" in cases:
    P = 257
    for lname, oname, pt in each():
        _, vk, ik, ioff, ext, _ = LAYOUTS[lname]
        op, pp = OPS[oname], per_pair(lname)
        # indices that are different on every rank and in every call: the rule is then a total
        # order, and the final target is the fold of all origins in any order
        def origin(q, call):
            raw = gen(lname, 10 + 3 * q + call, P)
            raw[:, ioff: ioff + KIND[ik].itemsize] = enc(ik, np.full(P, 3 * q + call + 1))
            return raw
        win = mp.Win.Allocate(P * pp, tdtype(lname), W, device=on_gpu)
        start = origin(n, 0)
        win.tensor.copy_(to_tensor(lname, start).to(dev))
        win.Fence()
        fetched = []
        for call in range(3):
            o = to_tensor(lname, origin(r, call)).to(dev)
            res = torch.zeros_like(o)
            if call == 0:  # (each call takes rank 0's exclusive lock itself, as every accumulate here does)
                win.Accumulate(o, 0, 0, op, pairtype=pt)
            elif call == 1:
                win.Get_accumulate(o, res, 0, 0, op, pairtype=pt)
            else:
                win.Fetch_and_op(o[:pp], res[:pp], 0, 0, op, pairtype=pt)
            fetched.append(res)
        win.Fence()
        want = start.copy()
        for q in range(n):
            for call in range(3):
                s = origin(q, call)
                if call == 2:
                    s = np.concatenate([s[:1], want[1:]])  # Fetch_and_op: one pair
                want = np.where(takes_b(lname, want, s, oname == "MAXLOC")[:, None], s, want)
        if r == 0:
            eq(lname, win.tensor, want, ("onesided", lname, oname))
        # what a fetch returned is a pair the target held at some time: the start or an origin
        got = raw_of(lname, fetched[1])
        cand = [start] + [origin(q, c) for q in range(n) for c in range(3)]
        assert all(any(np.array_equal(got[i], c[i]) for c in cand) for i in range(0, P, 16)), lname
        W.Barrier()
        win.Free()
    ok("onesided")

# ------------------------------------------------------------------ refused before any ticket is taken
if "errors" in cases:
    b, cb = W.ar_stats(), W.coll_stats()
    f = torch.zeros(8, device=dev)

    def refused(exc, fn):
        try:
            fn()
        except exc:
            return
        raise AssertionError("accepted")
    refused(ValueError, lambda: W.Allreduce(f[:7], f[:7], C.MAXLOC, algo="window"))  # an odd element count
    refused(ValueError, lambda: W.Reduce_scatter(f, f[:3], [3, 5] + [0] * (n - 2), C.MAXLOC, algo="window"))
    refused(ValueError, lambda: W.Allreduce(f, f, C.SUM, algo="window", pairtype=dt.FLOAT_INT))
    refused(ValueError, lambda: W.Scan(f, f, C.MAX, algo="window", pairtype=dt.TWOINT))
    refused(TypeError, lambda: W.Allreduce(f, f, C.MAXLOC, algo="window", pairtype=dt.SHORT_INT))
    refused(TypeError, lambda: W.Allreduce(f, f, C.MINLOC, algo="p2p", pairtype=dt.LONG_DOUBLE_INT))
    refused(TypeError, lambda: W.Allreduce(f, f, C.MAXLOC, algo="window", pairtype=dt.FLOAT))
    raw = torch.zeros(64, dtype=torch.uint8, device=dev)
    refused(ValueError, lambda: W.Allreduce(raw[2:18], raw[2:18], C.MAXLOC, pairtype=dt.FLOAT_INT))  # 2 mod 4
    refused(ValueError, lambda: W.Allreduce(raw[4:36], raw[4:36], C.MAXLOC, pairtype=dt.DOUBLE_INT))  # 4 mod 8
    refused(ValueError, lambda: W.Allreduce(raw[:12], raw[:12], C.MAXLOC, pairtype=dt.FLOAT_INT))  # one pair and a half
    refused(ValueError, lambda: C.Reduce_local(f, f.clone(), C.SUM, pairtype=dt.FLOAT_INT))
    assert W.ar_stats() == b and W.coll_stats() == cb
    ok("errors")

# ------------------------------------------------------------------ one pair on the p2p tree: as it always was
if "k1" in cases:
    loc = torch.tensor([[float((r * 7) % n), float(r)]], device=dev)
    ol = torch.zeros_like(loc)
    W.Allreduce(loc, ol, mp.MAXLOC, algo="p2p")
    vals = [((q * 7) % n, q) for q in range(n)]
    best = max(vals, key=lambda t: (t[0], -t[1]))
    assert ol.tolist()[0] == [float(best[0]), float(best[1])]
    W.Allreduce(loc, ol, mp.MINLOC)
    assert ol[0, 0].item() == 0.0 and ol.shape == loc.shape
    two = torch.tensor([[1.0, float(r)], [float(r), 5.0]], device=dev)  # k = 2 on the tree
    o2 = torch.zeros_like(two)
    W.Allreduce(two, o2, mp.MAXLOC, algo="p2p")
    assert o2.tolist() == [[1.0, 0.0], [float(n - 1), 5.0]], o2
    a, bb = torch.tensor([1.0, 4.0, 2.0, 0.0]), torch.tensor([1.0, 3.0, 1.0, 9.0])
    assert C.MAXLOC(a, bb).tolist() == [1.0, 3.0, 2.0, 0.0] and C.MINLOC(a, bb).tolist() == [1.0, 3.0, 1.0, 9.0]
    ok("k1")

W.Barrier()
W.sym_free()
mp.Finalize()
if r == 0:
    print("ALL_DONE", flush=True)
