"""Window collectives: reduce-scatter, all-gather(v), all-to-all, broadcast, reduce, scan and
exscan over symmetric memory (csrc/kernels/peer_coll.hip, csrc/core/window.cpp, comm.py "window
collectives"). The multi-rank script is tests/mp/win_collectives.py; every comparison in it is
bitwise against the CPU computation from the gathered inputs, and a silent fallback fails it.
The kernels alone are in tests/test_peer_coll_kernels.py."""
import pytest
import torch

from mp_util import run_ranks

ENV = {"MPIT_AR_STAGE_MB": "0.0625"}  # 64 KiB staging window: the staged paths run in several pieces
CPU = {"MPIT_CPU_ONLY": "1", **ENV}
GPU = {"T_DEVICE": "cuda", **ENV}


def _cases(out, names):
    for c in names:
        assert f"OK {c}" in out, (c, out[-3000:])
    assert "ALL_DONE" in out


# ------------------------------------------------------------------ the interface, one process
def test_algo_argument_and_coll_stats_single_rank():
    """algo= is accepted and validated; a communicator of one is not eligible and takes today's
    routing, counted as a fallback; ar_stats keeps its four keys."""
    from mpit_amd import comm as C

    W = C.Comm([0], 4242)  # (a communicator of this process alone: nothing in here communicates)
    x, y = torch.arange(6, dtype=torch.float32), torch.zeros(6)
    W.Reduce_scatter(x, y, None, C.SUM, algo="window")
    assert torch.equal(y, x)
    W.Scan(x, y, C.SUM, algo="window")
    W.Allgather(x, y, algo="p2p")
    W.Alltoall(x, y, algo="auto")
    with pytest.raises(ValueError):
        W.Allgather(x, y, algo="ring")
    cs = W.coll_stats()
    assert set(cs) == {"reduce_scatter", "allgather", "alltoall", "bcast", "reduce", "scan", "exscan"}
    assert cs["reduce_scatter"] == {"window": 0, "window_staged": 0, "fallback": 1} and cs["scan"]["fallback"] == 1
    assert cs["allgather"] == {"window": 0, "window_staged": 0, "fallback": 0}
    assert set(W.ar_stats()) == {"window", "window_staged", "p2p", "rccl"}


# ------------------------------------------------------------------ CPU tier (host shm windows)
def test_window_collectives_cpu_three_ranks():
    out = run_ranks("win_collectives.py", 3, CPU, timeout=300)
    _cases(out, ["rs_ag", "scan", "a2a", "rooted", "fifo", "sharded"])


def test_window_collectives_cpu_four_ranks():
    out = run_ranks("win_collectives.py", 4, {"T_CASES": "rs_ag,scan,subcomm,sharded", **CPU}, timeout=300)
    _cases(out, ["rs_ag", "scan", "subcomm", "sharded"])


def test_window_scan_equals_p2p_cpu_two_ranks():
    out = run_ranks("win_collectives.py", 2, {"T_CASES": "p2p", **CPU}, timeout=300)
    _cases(out, ["p2p"])


# ------------------------------------------------------------------ GPU tier (ranks share the device)
@pytest.mark.gpu
def test_window_collectives_gpu_two_ranks():
    out = run_ranks("win_collectives.py", 2, {"T_CASES": "rs_ag,scan,p2p,sharded", **GPU}, timeout=300)
    _cases(out, ["rs_ag", "scan", "p2p", "sharded"])


@pytest.mark.gpu
def test_window_collectives_gpu_three_ranks():
    out = run_ranks("win_collectives.py", 3, GPU, timeout=300)
    _cases(out, ["rs_ag", "scan", "a2a", "rooted", "fifo", "sharded"])


@pytest.mark.gpu
def test_window_collectives_gpu_four_ranks():
    out = run_ranks("win_collectives.py", 4, {"T_CASES": "rs_ag,a2a,rooted,subcomm", **GPU}, timeout=300)
    _cases(out, ["rs_ag", "a2a", "rooted", "subcomm"])
