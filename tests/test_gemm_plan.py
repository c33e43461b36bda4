"""The GEMM launch selection (csrc/kernels/gemm.hip nt_plan / tn_plan) against a recorded table.

Every kernel variant is numerically right, so the exact oracles cannot notice a wrong tile,
ring depth or split plan: it only shows as a slower benchmark. tests/golden/gemm_plan_table.json
holds, for every case of tests/gemm_plan_cases.py under every knob setting, the kernel
instantiation, grid, dynamic LDS and split-reduce grids that the launchers of the commit before
the planners existed issued (recorded there by redefining hipLaunchKernelGGL above the launchers
to print its stringified kernel expression, grid and LDS bytes, with the HIP calls stubbed, and
driving launch_nt / launch_tn over the cases in one process per setting). The planners the
launchers now call must choose the same, and the recorded launches must reach every
instantiation that is built. CPU only: dev = -1 plans for 256 compute units."""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

import gemm_plan_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [G.setting_id(e) for e in G.SETTINGS]
ENVS = dict(zip(IDS, G.SETTINGS))

with open(os.path.join(ROOT, "tests", "golden", "gemm_plan_table.json")) as _f:
    TABLE = json.load(_f)


def _expand(packed, base=None):
    """A table entry 'inst|grid[|reduce grids]' as the row tests/mp/gemm_plan_dump.py prints:
    'instantiation|grid|LDS bytes[|reduce grids]' (TABLE['inst'] holds 'instantiation|LDS', or a
    refusal's whole text). A bare number is an instantiation with the grids of the row `base`."""
    if isinstance(packed, int):
        b = base.split("|")
        packed = "|".join([str(packed), b[1]] + b[3:])
    i, *rest = packed.split("|")
    inst = TABLE["inst"][int(i)]
    if inst.startswith("error:"):
        return inst
    name, lds = inst.split("|")
    return "|".join([name, rest[0], lds] + rest[1:])


def golden(sid):
    """The recorded rows of one setting, by index into cases(): the table stores a setting as its
    differences from the default (a combination of two knobs: from its first knob alone)."""
    if sid == "default":
        return dict(enumerate(_expand(r) for r in TABLE["default"]))
    env = ENVS[sid]
    rows = dict(golden(G.setting_id(G.base_of(env))))
    rows.update((int(i), _expand(r, rows[int(i)])) for i, r in TABLE["settings"][sid].items())
    index = {tuple(sorted(c.items())): i for i, c in enumerate(G.cases())}
    return {i: rows[i] for i in (index[tuple(sorted(c.items()))] for c in G.cases(env))}


def _child(env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mp", "gemm_plan_dump.py")],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout)


@pytest.fixture(scope="module")
def dumps():
    """One child per knob setting (knobs are read once per process), a few at a time."""
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return dict(zip(IDS, ex.map(_child, G.SETTINGS)))


def test_table_matches_the_case_list():
    assert len(TABLE["default"]) == len(G.cases())
    assert set(TABLE["settings"]) == set(IDS) - {"default"}


@pytest.mark.parametrize("sid", IDS)
def test_plans_equal_the_recorded_launches(dumps, sid):
    cases, want = G.cases(ENVS[sid]), golden(sid)
    got = dumps[sid]["rows"]
    assert len(got) == len(want) == len(cases)
    bad = [(c, g, w) for c, g, w in zip(cases, got, want.values()) if g != w]
    assert not bad, f"{len(bad)} of {len(got)} plans differ, e.g.\n" + "\n".join(
        f"{c}\n  planned  {g}\n  recorded {w}" for c, g, w in bad[:8])


# Built but reached by no input: (f32, TBN, TBK, STAGES, CONV, FM, KR) of gemm_tn_kernel.
# fp32 gemm_tn always runs a 2-deep ring (it stages twice the bytes per row), yet the 4-deep
# fp32 instantiations have always been compiled next to the bf16 ones; they stay so the code
# object keeps its kernels.
UNREACHED_TN = {(1, tbn, tbk, 4, conv, fm, 32)
                for tbn in (64, 128) for tbk in (64, 128) for conv in (0, 1) for fm in (0, 1, 11, 12)}
UNREACHED_NT = set()


def _seen(prefix):
    out = set()
    for sid in IDS:
        for r in golden(sid).values():
            if r.startswith(prefix + ":"):
                out.add(tuple(int(v) for v in r.split("|")[0].split(":")[1:]))
    return out


def test_recorded_launches_reach_every_built_instantiation(dumps):
    d = dumps["default"]
    nt_built = {tuple(v) for v in d["nt_built"]}
    tn_built = {tuple(v) for v in d["tn_built"]}
    assert UNREACHED_NT <= nt_built and UNREACHED_TN <= tn_built
    nt_seen, tn_seen = _seen("nt"), _seen("tn")
    assert nt_seen - nt_built == set() and tn_seen - tn_built == set()
    assert sorted(nt_built - UNREACHED_NT - nt_seen) == []
    assert sorted(tn_built - UNREACHED_TN - tn_seen) == []
    # both instantiations of the split-once fp32 kernel
    assert _seen("tnf32s") == {(1, 0), (1, 1)}
