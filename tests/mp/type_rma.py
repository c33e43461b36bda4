"""Derived datatypes between ranks: one-launch Put / Get on a derived target type
(Window::put_plan / get_plan over csrc/kernels/type_copy.hip) and Send / Recv of derived types
and of non-contiguous tensors, on 2 ranks under torch.distributed.run. T_DEVICE=cuda: the ranks
share the box's GPU and windows / buffers are HBM; otherwise host shm windows and the host twin.

Every comparison is bitwise against a per-byte oracle built from the type map's definition
(numpy), over the target's WHOLE window, sentinels included. Each case prints ``OK <case>`` on
rank 0. Cases (T_CASES, comma separated): put, get, sendrecv, views, mismatch."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

import mpit_amd as mp
from mpit_amd import datatypes as dt
from mpit_amd import mpiT
from mpit_amd.comm import COMM_WORLD

mp.Init()
W = COMM_WORLD()
r, n = W.Get_rank(), W.Get_size()
assert n == 2
peer = 1 - r
on_gpu = os.environ.get("T_DEVICE", "cpu") == "cuda"
dev = mp.runtime.device() if on_gpu else torch.device("cpu")
cases = os.environ.get("T_CASES", "put,get,sendrecv,views,mismatch").split(",")
SENT = 0xA5
WIN_BYTES = 4096


def ok(name):
    W.Barrier()
    if r == 0:
        print("OK", name, flush=True)


def type_index(t, count):
    idx = []
    for i in range(count):
        for d, b in t.typemap:
            idx.extend(range(i * t.extent + d, i * t.extent + d + dt._BASIC[b][0]))
    return np.array(idx, dtype=np.int64)


def rand_bytes(nbytes, seed):
    return np.random.default_rng(seed).integers(1, 256, nbytes, dtype=np.uint8)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def sync_dev():
    if on_gpu:
        torch.cuda.synchronize()


VEC = dt.Type_vector(64, 2, 5, dt.INT)  # 64 runs of 8 bytes every 20
IRR = dt.Type_create_hindexed([3, 1, 6, 2, 16], [1, 6, 9, 40, 64], dt.BYTE)  # irregular, extent 79
ORG = dt.Type_vector(4, 1, 3, dt.INT)  # a derived origin: 4 ints, every third
TARGETS = [("vec", VEC, 1, 3), ("irr", IRR, 8, 16)]  # name, type, count, displacement (bytes)


def origin_for(nbytes, derived, seed):
    """(origin tensor, count, datatype, the packed bytes it carries as numpy)."""
    if not derived:
        host = rand_bytes(nbytes, seed)
        return to_dev(host), nbytes, dt.BYTE, host
    assert nbytes % ORG.Get_size() == 0
    cnt = nbytes // ORG.Get_size()
    idx = type_index(ORG, cnt)
    host = rand_bytes(int(idx.max()) + 1, seed)
    return to_dev(host), cnt, ORG, host[idx]


def new_window():
    win = mpiT.Win_create(torch.full((WIN_BYTES,), SENT, dtype=torch.uint8, device=dev), comm=W)
    win.tensor.fill_(SENT)  # a host window is a shm copy: fill the exposed memory itself
    sync_dev()
    mpiT.Win_fence(0, win)
    return win


if "put" in cases:
    for name, typ, cnt, disp in TARGETS:
        for derived in (False, True):
            win = new_window()
            tidx = type_index(typ, cnt) + disp
            org, ocnt, otyp, carried = origin_for(len(tidx), derived, 10 * r + derived)
            before = dict(dt.COUNTERS)
            assert mpiT.Put(org, ocnt, otyp, peer, disp, cnt, typ, win) == mpiT.SUCCESS
            assert dt.COUNTERS["rma_kernel"] == before["rma_kernel"] + 1 and dt.COUNTERS["rma_copies"] == 0
            mpiT.Win_fence(0, win)
            # what the peer put into MY window: its origin stream, regenerated from its seed
            _, _, _, theirs = origin_for(len(tidx), derived, 10 * peer + derived)
            want = np.full(WIN_BYTES, SENT, dtype=np.uint8)
            want[tidx] = theirs
            got = win.tensor.cpu().numpy()
            assert np.array_equal(got, want), (name, derived, np.flatnonzero(got != want)[:8])
            mpiT.Win_fence(0, win)
            mpiT.Win_free(win)
    # a span that leaves the window is refused on the host, nothing launched
    win = new_window()
    try:
        mpiT.Put(to_dev(rand_bytes(VEC.Get_size(), 1)), VEC.Get_size(), dt.BYTE, peer, WIN_BYTES - 100, 1, VEC, win)
        raise AssertionError("Put outside the window accepted")
    except IndexError:
        pass
    mpiT.Win_fence(0, win)
    assert bool((win.tensor == SENT).all())
    mpiT.Win_free(win)
    ok("put")

if "get" in cases:
    for name, typ, cnt, disp in TARGETS:
        for derived in (False, True):
            win = new_window()
            win.tensor.copy_(to_dev(rand_bytes(WIN_BYTES, 50 + r)))
            sync_dev()
            mpiT.Win_fence(0, win)
            tidx = type_index(typ, cnt) + disp
            remote = rand_bytes(WIN_BYTES, 50 + peer)
            if derived:
                ocnt = len(tidx) // ORG.Get_size()
                oidx = type_index(ORG, ocnt)
                dst = torch.full((int(oidx.max()) + 1 + 9,), SENT, dtype=torch.uint8, device=dev)
                otyp = ORG
            else:
                ocnt, otyp, oidx = len(tidx), dt.BYTE, np.arange(len(tidx))
                dst = torch.full((len(tidx) + 9,), SENT, dtype=torch.uint8, device=dev)
            before = dict(dt.COUNTERS)
            assert mpiT.Get(dst, ocnt, otyp, peer, disp, cnt, typ, win) == mpiT.SUCCESS
            assert dt.COUNTERS["rma_kernel"] == before["rma_kernel"] + 1 and dt.COUNTERS["rma_copies"] == 0
            mpiT.Win_fence(0, win)
            want = np.full(dst.numel(), SENT, dtype=np.uint8)
            want[oidx] = remote[tidx]
            assert np.array_equal(dst.cpu().numpy(), want), (name, derived)
            assert np.array_equal(win.tensor.cpu().numpy(), rand_bytes(WIN_BYTES, 50 + r))  # a Get writes no window
            mpiT.Win_fence(0, win)
            mpiT.Win_free(win)
    ok("get")

if "sendrecv" in cases:
    for typ, cnt in ((VEC, 2), (IRR, 3)):
        idx = type_index(typ, cnt)
        nb = int(idx.max()) + 1 + 4
        host = rand_bytes(nb, 70 + r)
        dst = torch.full((nb,), SENT, dtype=torch.uint8, device=dev)
        before = dt.COUNTERS["kernel"]
        rq = W.Irecv(dst, peer, 5, count=cnt, datatype=typ)
        W.Send(to_dev(host), peer, 5, count=cnt, datatype=typ)
        rq.Wait()
        assert dt.COUNTERS["kernel"] == before + 2  # one pack, one unpack
        want = np.full(nb, SENT, dtype=np.uint8)
        want[idx] = rand_bytes(nb, 70 + peer)[idx]
        assert np.array_equal(dst.cpu().numpy(), want)
    ok("sendrecv")

if "views" in cases:
    def views_of(x, y):
        return [x[:, 1:5], x.t(), y.contiguous(memory_format=torch.channels_last), x[::3]]

    def make(rank):
        x = (torch.arange(60, dtype=torch.float32) + 1000 * (rank + 1)).reshape(6, 10)
        y = (torch.arange(120, dtype=torch.int16) + 1000 * (rank + 1)).reshape(2, 3, 4, 5)
        return x.to(dev), y.to(dev)

    mine, theirs = views_of(*make(r)), views_of(*make(peer))
    for k, (v, tv) in enumerate(zip(mine, theirs)):
        assert not v.is_contiguous()
        # strided view -> contiguous buffer
        flat = torch.zeros(v.numel(), dtype=v.dtype, device=dev)
        rq = W.Irecv(flat, peer, 20 + k)
        W.Send(v, peer, 20 + k)
        rq.Wait()
        assert torch.equal(flat.cpu(), tv.cpu().reshape(-1)), k
        # strided view -> strided view of a sentinel-filled storage of the same geometry
        span = max(sum((s - 1) * st for s, st in zip(v.shape, v.stride())) + 1, 1)
        store = torch.full((span + 3,), -7, dtype=v.dtype, device=dev)
        into = torch.as_strided(store, v.shape, v.stride())
        rq = W.Irecv(into, peer, 40 + k)
        W.Send(v, peer, 40 + k)
        st = rq.Wait()
        assert st.Get_count() == v.numel()
        want = torch.full((span + 3,), -7, dtype=v.dtype)
        torch.as_strided(want, v.shape, v.stride()).copy_(tv.cpu())
        assert torch.equal(store.cpu(), want), k
    # receiving into a tensor that aliases itself is refused
    x, _ = make(r)
    for bad in (x[0:1, :].expand(4, 10), torch.as_strided(x, (3, 4), (2, 1))):
        try:
            W.Irecv(bad, peer, 99)
            raise AssertionError("self-overlapping receive buffer accepted")
        except ValueError:
            pass
    # while sending an expanded tensor is fine
    e = x[0:1, :].expand(4, 10)
    flat = torch.zeros(40, device=dev)
    rq = W.Irecv(flat, peer, 60)
    W.Send(e, peer, 60)
    rq.Wait()
    assert torch.equal(flat.cpu(), make(peer)[0][0:1, :].expand(4, 10).cpu().reshape(-1))
    # collectives keep refusing strided buffers
    try:
        W.Bcast(x[:, 1:5], 0)
        raise AssertionError("strided collective buffer accepted")
    except ValueError:
        pass
    ok("views")

if "mismatch" in cases:
    win = new_window()
    src = to_dev(rand_bytes(VEC.Get_size(), 3))
    for cnt in (VEC.Get_size() - 4, 4):
        try:  # signatures that do not carry the same bytes are refused, not silently truncated
            mpiT.Put(src, cnt, dt.BYTE, peer, 0, 1, VEC, win)
            raise AssertionError("mismatched one-sided signature accepted")
        except ValueError:
            pass
    dst = torch.zeros(VEC.Get_size(), dtype=torch.uint8, device=dev)
    try:
        mpiT.Get(dst, 8, dt.BYTE, peer, 0, 1, VEC, win)
        raise AssertionError("mismatched one-sided signature accepted")
    except ValueError:
        pass
    mpiT.Win_fence(0, win)
    assert bool((win.tensor == SENT).all())
    mpiT.Win_free(win)
    ok("mismatch")

W.Barrier()
if r == 0:
    print("ALL_DONE", flush=True)
mp.Finalize()
