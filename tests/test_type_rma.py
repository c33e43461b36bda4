"""Derived datatypes between ranks (tests/mp/type_rma.py): Put / Get on a derived target type in
one type_copy launch on the peer-mapped window (Window::put_plan / get_plan), Send / Recv of
derived types and of non-contiguous tensors. 2 ranks on host shm windows (the host twin) and, gpu
tier, 2 ranks sharing the device. Every comparison in the script is bitwise against a per-byte
oracle over the target's whole window."""
import pytest

from mp_util import run_ranks

CASES = ["put", "get", "sendrecv", "views", "mismatch"]


def _cases(out, names):
    for c in names:
        assert f"OK {c}" in out, (c, out[-3000:])
    assert "ALL_DONE" in out


def test_type_rma_cpu_two_ranks():
    _cases(run_ranks("type_rma.py", 2, {"MPIT_CPU_ONLY": "1"}, timeout=240), CASES)


@pytest.mark.gpu
def test_type_rma_gpu_two_ranks():
    _cases(run_ranks("type_rma.py", 2, {"T_DEVICE": "cuda"}, timeout=240), CASES)
