"""Irregular window collectives: Gatherv / Gather, Scatterv / Scatter, Alltoallv and the strided
Alltoallw over symmetric memory (csrc/kernels/peer_plan.hip, csrc/core/window.cpp
Window::pull_plan, comm.py "irregular window collectives"). The multi-rank script is
tests/mp/win_vcollectives.py; every comparison in it is bitwise against the CPU computation from
the gathered inputs, and vcoll_stats() is read around every call, so a silent fallback fails it.
The kernel alone is in tests/test_peer_plan_kernels.py."""
import pytest
import torch

from mp_util import run_ranks

ENV = {"MPIT_AR_STAGE_MB": "0.0625"}  # 64 KiB staging window
CPU = {"MPIT_CPU_ONLY": "1", **ENV}
GPU = {"T_DEVICE": "cuda", **ENV}
ALL = ["rooted", "a2av", "a2aw", "mixed", "big", "errors", "fifo", "p2p"]


def _cases(out, names):
    for c in names:
        assert f"OK {c}" in out, (c, out[-3000:])
    assert "ALL_DONE" in out


def _run(n, names, env):
    _cases(run_ranks("win_vcollectives.py", n, {"T_CASES": ",".join(names), **env}, timeout=300), names)


# ------------------------------------------------------------------ the interface, one process
def test_algo_argument_and_vcoll_stats_single_rank():
    """algo= is accepted and validated on all six calls; a communicator of one is not eligible and
    takes today's routing, counted as a fallback; coll_stats keeps its seven keys."""
    from mpit_amd import comm as C

    W = C.Comm([0], 4243)  # (a communicator of this process alone: nothing in here communicates)
    x, y = torch.arange(6, dtype=torch.float32), torch.zeros(6)
    W.Gatherv(x, y, [6], [0], 0, algo="window")
    assert torch.equal(y, x)
    W.Gather(x, y.zero_(), 0, algo="window")
    W.Scatterv(x, y.zero_(), [6], [0], 0, algo="window")
    W.Scatter(x, y.zero_(), 0, algo="p2p")
    W.Alltoallv(x, [6], [0], y.zero_(), [6], [0], algo="window")
    assert torch.equal(y, x)
    m = torch.zeros(2, 3)
    W.Alltoallw([x.view(3, 2).t()], [m], algo="window")
    assert torch.equal(m, x.view(3, 2).t())
    W.Alltoallw([x], [y], algo="auto")
    for call in (lambda: W.Gatherv(x, y, None, None, 0, algo="ring"), lambda: W.Alltoallw([x], [y], algo="ring"),
                 lambda: W.Alltoallv(x, [6], [0], y, [6], [0], algo="ring"), lambda: W.Scatter(x, y, 0, algo="ring")):
        with pytest.raises(ValueError):
            call()
    one = {"window": 0, "window_staged": 0, "fallback": 1}
    assert W.vcoll_stats() == {"gatherv": {**one, "fallback": 2}, "scatterv": one, "alltoallv": one, "alltoallw": one}
    assert set(W.coll_stats()) == {"reduce_scatter", "allgather", "alltoall", "bcast", "reduce", "scan", "exscan"}
    assert all(v == {"window": 0, "window_staged": 0, "fallback": 0} for v in W.coll_stats().values())


def test_environment_does_not_reroute_the_internal_calls(monkeypatch):
    """Allgatherv, Alltoall and Reduce_scatter reach Gatherv / Alltoallv / Scatterv with
    algo="auto": MPIT_COLLECTIVES=window counts the outer call alone."""
    from mpit_amd import comm as C

    monkeypatch.setenv("MPIT_COLLECTIVES", "window")
    W = C.Comm([0], 4244)
    x, y = torch.arange(6, dtype=torch.float32), torch.zeros(6)
    W.Allgatherv(x, y, [6], [0])
    W.Alltoall(x, y.zero_())
    W.Reduce_scatter(x, y.zero_(), [6], C.SUM)
    assert torch.equal(y, x)
    assert all(v["fallback"] == 0 for v in W.vcoll_stats().values()), W.vcoll_stats()
    assert W.coll_stats()["allgather"]["fallback"] == 1 and W.coll_stats()["alltoall"]["fallback"] == 1
    W.Alltoallv(x, [6], [0], y.zero_(), [6], [0])  # called directly, the variable holds
    assert W.vcoll_stats()["alltoallv"]["fallback"] == 1


# ------------------------------------------------------------------ CPU tier (host shm windows)
def test_window_vcollectives_cpu_three_ranks():
    _run(3, ALL, CPU)


def test_window_vcollectives_cpu_four_ranks():
    _run(4, ["rooted", "a2av", "a2aw", "mixed", "subcomm"], CPU)


def test_window_vcollectives_cpu_two_ranks():
    _run(2, ["a2av", "a2aw", "errors", "p2p"], CPU)


# ------------------------------------------------------------------ GPU tier (ranks share the device)
# The comparison with algo="p2p" stays in the CPU tier: it measures the window path against the
# point-to-point messages, and those are host messages there. (Between HBM buffers the
# point-to-point path refuses an empty message, which uneven counts produce.)
@pytest.mark.gpu
def test_window_vcollectives_gpu_two_ranks():
    _run(2, ["rooted", "a2av", "a2aw", "mixed", "fifo"], GPU)


@pytest.mark.gpu
def test_window_vcollectives_gpu_three_ranks():
    _run(3, [c for c in ALL if c != "p2p"], GPU)


@pytest.mark.gpu
def test_window_vcollectives_gpu_four_ranks():
    _run(4, ["rooted", "a2av", "a2aw", "mixed", "big", "errors", "subcomm"], GPU)
