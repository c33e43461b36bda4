"""Window all-reduce: the peer-reduce kernel (csrc/kernels/allreduce.hip) and its host twin, the
two-barrier protocol (csrc/core/window.cpp), symmetric memory / routing / the FIFO (comm.py) and
the data-parallel trainer on top of it (parallel/ddp.py). The multi-rank scripts are
tests/mp/win_allreduce.py and tests/mp/ddp_window_equiv.py; every comparison in them is bitwise
against the left fold in rank order."""
import pytest
import torch

from mp_util import run_ranks

ENV = {"MPIT_ALLREDUCE": "window", "MPIT_AR_STAGE_MB": "0.0625"}  # 64 KiB staging buffer


def _cases(out, names):
    for c in names:
        assert f"OK {c}" in out, (c, out[-3000:])
    assert "ALL_DONE" in out


def _result(out):
    return eval([ln for ln in out.splitlines() if ln.startswith("RESULT")][-1][len("RESULT"):])


# ------------------------------------------------------------------ host twin, one process
def test_peer_reduce_host_twin_fold_order_and_single_rounding():
    from mpit_amd._ext import native

    nat = native()
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(1031, generator=g) * torch.pow(2.0, torch.randint(-20, 21, (1031,), generator=g).float())
          for _ in range(5)]
    out = [torch.zeros(1031) for _ in range(2)]
    nat.peer_reduce(-1, 0, 0, 0, [x.data_ptr() for x in xs], [o.data_ptr() for o in out], 1031)
    exp = xs[0]
    for x in xs[1:]:
        exp = exp + x
    assert torch.equal(out[0].view(torch.int32), exp.view(torch.int32)) and torch.equal(out[0], out[1])
    rev = torch.zeros(1031)
    nat.peer_reduce(-1, 0, 0, 0, [x.data_ptr() for x in xs[::-1]], [rev.data_ptr()], 1031)
    assert not torch.equal(rev, out[0])  # the order given is the order folded
    # bf16: fp32 accumulation, one rounding (a chain of bf16 additions rounds after every step)
    bs = [x.bfloat16() for x in xs]
    ob = torch.zeros(1031, dtype=torch.bfloat16)
    nat.peer_reduce(-1, 0, 0, 1, [b.data_ptr() for b in bs], [ob.data_ptr()], 1031)
    acc = bs[0].float()
    for b in bs[1:]:
        acc = acc + b.float()
    assert torch.equal(ob.view(torch.int16), acc.bfloat16().view(torch.int16))
    # in place on source 0, and the bitwise ops are integer only
    a, b = torch.arange(40, dtype=torch.int32), torch.full((40,), 6, dtype=torch.int32)
    nat.peer_reduce(-1, 0, 7, 4, [a.data_ptr(), b.data_ptr()], [a.data_ptr()], 40)
    assert torch.equal(a, torch.arange(40, dtype=torch.int32) & 6)
    assert not nat.peer_reduce_supported(7, 0) and not nat.peer_reduce_supported(9, 3)
    with pytest.raises(Exception):
        nat.peer_reduce(-1, 0, 7, 0, [xs[0].data_ptr()], [out[0].data_ptr()], 4)
    with pytest.raises(Exception):
        nat.peer_reduce(-1, 0, 0, 0, [xs[0].data_ptr()] * 9, [out[0].data_ptr()], 4)


# ------------------------------------------------------------------ CPU tier (host shm windows)
def test_window_allreduce_suite_cpu_three_ranks():
    """Kernel grid (host twin), one-shot == two-shot, staged path, FIFO, routing: 3 ranks."""
    out = run_ranks("win_allreduce.py", 3, {"MPIT_CPU_ONLY": "1", **ENV}, timeout=300)
    _cases(out, ["grid", "modes", "staged", "fifo", "routing"])


def test_window_allreduce_subcommunicators_cpu_four_ranks():
    out = run_ranks("win_allreduce.py", 4, {"MPIT_CPU_ONLY": "1", "T_CASES": "subcomm", **ENV}, timeout=300)
    _cases(out, ["subcomm"])


def test_ddp_window_cpu_three_ranks():
    """Host gradients go through the staging buffer: still the rank-order fold, whatever the
    bucket layout, fp32 and bf16 wire; cnn7 training (one warm-up and four timed steps) ends
    bit-identical with tiny buckets and with one bucket (the ring gives this only at 2 ranks)."""
    res = _result(run_ranks("ddp_window_equiv.py", 3, {"MPIT_CPU_ONLY": "1", "T_PART": "grads,train"}, timeout=300))
    assert len(res) == 3
    for rr in res:
        for wire in ("fp32", "bf16"):
            g = rr["grads_" + wire]
            assert g["same"] and g["fold"] and g["padding"] and g["window"], (wire, rr)
            assert g["buckets"][0] > 3 and g["buckets"][1] == 1 and g["registered"] == 0, (wire, rr)
        t = rr["train"]
        assert t["same"] and t["finite"] and t["buckets"][0] > 3 and t["buckets"][1] == 1, rr
        assert t["calls"]["window"] == 5 * t["buckets"][0], rr
    assert len({rr["train"]["digest"] for rr in res}) == 1, res


def test_ddp_window_equals_p2p_cpu_two_ranks():
    """A sum of two is order-free: the window path and the point-to-point path train to the
    same bits."""
    res = _result(run_ranks("ddp_window_equiv.py", 2, {"MPIT_CPU_ONLY": "1", "T_PART": "p2p"}, timeout=300))
    for rr in res:
        p = rr["p2p"]
        assert p["same"], rr
        assert p["window_calls"]["window"] == 5 * p["buckets"], rr
        assert p["p2p_calls"]["window"] == 0 and p["p2p_calls"]["p2p"] >= 5 * p["buckets"], rr


# ------------------------------------------------------------------ GPU tier (ranks share the device)
@pytest.mark.gpu
def test_window_allreduce_grid_gpu_two_ranks():
    out = run_ranks("win_allreduce.py", 2, {"T_DEVICE": "cuda", "T_CASES": "grid,modes", **ENV}, timeout=300)
    _cases(out, ["grid", "modes"])


@pytest.mark.gpu
def test_window_allreduce_suite_gpu_three_ranks():
    out = run_ranks("win_allreduce.py", 3, {"T_DEVICE": "cuda", **ENV}, timeout=300)
    _cases(out, ["grid", "modes", "staged", "fifo", "routing"])


@pytest.mark.gpu
def test_window_allreduce_subcommunicators_gpu_four_ranks():
    out = run_ranks("win_allreduce.py", 4, {"T_DEVICE": "cuda", "T_CASES": "subcomm", **ENV}, timeout=300)
    _cases(out, ["subcomm"])


@pytest.mark.gpu
def test_ddp_window_gpu_three_ranks():
    """In place on the registered flat gradient (zero-copy, no staging): random gradients with tiny
    buckets == one bucket == rank-order fold, both wires. Then one warm-up and four timed cnn7 steps
    overlapped with the backward: tiny buckets and one bucket end bit-identical, on every rank."""
    res = _result(run_ranks("ddp_window_equiv.py", 3, {"T_PART": "grads,train"}, timeout=400))
    assert len(res) == 3
    for rr in res:
        for wire, nreg in (("fp32", 1), ("bf16", 2)):
            g = rr["grads_" + wire]
            assert g["same"] and g["fold"] and g["padding"] and g["window"], (wire, rr)
            assert g["buckets"][0] > 3 and g["buckets"][1] == 1, (wire, rr)
            assert g["registered"] == nreg and g["staged"] == 0, (wire, rr)
        t = rr["train"]
        assert t["same"] and t["finite"], rr
        assert t["buckets"][0] > 3 and t["buckets"][1] == 1 and t["registered"] == 1, rr
        # (1 + 4 steps of one all-reduce per bucket: every one of them took the window path)
        assert t["calls"]["window"] == 5 * t["buckets"][0], rr
        assert t["calls"]["window_staged"] == 0, rr
    assert len({rr["train"]["digest"] for rr in res}) == 1, res


@pytest.mark.gpu
def test_ddp_window_equals_p2p_gpu_two_ranks():
    """A sum of two is order-free: in place on the registered flat gradient, the window path and
    the point-to-point path train to the same bits."""
    res = _result(run_ranks("ddp_window_equiv.py", 2, {"T_PART": "p2p"}, timeout=400))
    assert len(res) == 2
    for rr in res:
        p = rr["p2p"]
        assert p["same"], rr
        assert p["window_calls"]["window"] == 5 * p["buckets"] and p["window_calls"]["window_staged"] == 0, rr
        assert p["p2p_calls"]["window"] == 0 and p["p2p_calls"]["p2p"] >= 5 * p["buckets"], rr
