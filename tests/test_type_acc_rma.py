"""One-sided accumulate between ranks (tests/mp/type_acc.py): Accumulate with every new op and
type, Get_accumulate and Fetch_and_op on basic and derived target types in one type_accumulate
launch under one target lock (Window::accumulate_plan), and the per-run axpby path that
MPIT_DTYPE_KERNEL=0 keeps. 2 ranks on host shm windows (the host twin) and, gpu tier, 2 ranks
sharing the device. Every comparison in the script is bitwise against a per-element oracle over
the target's whole window."""
import pytest

from mp_util import run_ranks

CASES = ["ops", "compat", "atomic", "fetch", "bounds"]


def _cases(out, names):
    for c in names:
        assert f"OK {c}" in out, (c, out[-3000:])
    assert "ALL_DONE" in out


def _result(out):
    return [ln for ln in out.splitlines() if ln.startswith("RESULT compat ")][-1]


def _both_paths(env):
    out = run_ranks("type_acc.py", 2, env, timeout=240)
    _cases(out, CASES)
    # the calls both paths serve give the same bytes without the kernel, counted per run
    off = run_ranks("type_acc.py", 2, {**env, "MPIT_DTYPE_KERNEL": "0", "T_CASES": "compat"}, timeout=240)
    _cases(off, ["compat"])
    assert _result(off) == _result(out) and len(_result(out)) > 40


def test_type_acc_cpu_two_ranks():
    _both_paths({"MPIT_CPU_ONLY": "1"})


@pytest.mark.gpu
def test_type_acc_gpu_two_ranks():
    _both_paths({"T_DEVICE": "cuda"})
