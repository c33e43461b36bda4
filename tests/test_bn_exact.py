"""Exact and fp64 oracles for the fused BatchNorm kernels (csrc/kernels/bn_act.hip) at their edges.

The apply passes are fmaf / add / max with per-channel coefficients and the reductions are sums,
so inputs whose fp32 results are exact in any order pin every element: dyadic coefficients on
small integers or 14-bit values give the fp64 result rounded once (bitwise, bf16 ties included),
integer data with a large common offset gives statistics whose only roundings are the handful
in the finalize (tolerance: that count + 1 ulp of the largest term, tests/bn_exact_util.py).
Every case asserts its exactness bound on the CPU first. Inputs end in NaN rows, outputs, mask
bytes, per-channel vectors and the amax buffer sit between sentinels, the workspace ends in
sentinels; everything outside what a call owns must still hold them afterwards. All calls go
through the raw bindings of mpit_amd._ext.native()."""
import os
import subprocess
import sys
import time

import pytest
import torch
import torch.nn.functional as F

import bn_exact_util as U
from gemm_exact_util import F32, PRE, assert_guards, key, out_buf, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
DTS = ("bf16", "f32")


def _m():
    from mpit_amd._ext import native

    return native()


def _check_all(cases, results):
    bad = []
    for c in cases:
        try:
            U.CHECK[c["op"]](c, results(c))
        except AssertionError as e:
            bad.append(str(e)[:300])
    print(f"{len(cases)} launches compared, {len(bad)} failed")
    assert not bad, f"{len(bad)} of {len(cases)} cases failed:\n" + "\n".join(bad[:12])


def _run(cases):
    """Launch and check every case; mismatches are collected so one run names them all (anything
    but a failed comparison, a HIP error for instance, ends the run at once)."""
    m = _m()
    _check_all(cases, lambda c: U.LAUNCH[c["op"]](m, c))


# ------------------------------------------------------------------ CPU: the net itself
@pytest.mark.parametrize("relu", (True, False))
def test_oracle_matches_fp64_batch_norm_autograd(relu):
    g = torch.Generator().manual_seed(11)
    for (M, C) in ((1, 8), (2, 8), (37, 24)):
        x = torch.randn(M, C, generator=g, dtype=torch.float64) * 3 + 50
        res, dy = torch.randn(M, C, generator=g, dtype=torch.float64), torch.randn(M, C, generator=g, dtype=torch.float64)
        ga, be = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
        rm0, rv0 = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 1
        o = U.bn_forward64(x, ga, be, rm0, rv0, res, relu)
        xa, ra, wa, ba = (t.clone().requires_grad_(True) for t in (x, res, ga, be))
        rm, rv = rm0.clone(), rv0.clone()
        # (an image of M pixels: F.batch_norm wants more than one value per channel only when M > 1)
        y = F.batch_norm(xa.t().reshape(1, C, M), rm, rv, wa, ba, training=True, momentum=U.MOM, eps=U.EPS) if M > 1 \
            else None
        if y is None:  # M = 1: the library refuses; var = 0, y = beta, unbiased factor M / 1
            assert torch.equal(o["var"], torch.zeros(C, dtype=torch.float64))
            torch.testing.assert_close(o["y"], (be + res).clamp(min=0) if relu else be + res, rtol=1e-10, atol=1e-10)
            torch.testing.assert_close(o["rvar"], (1 - U.MOM) * rv0, rtol=1e-14, atol=0)
            torch.testing.assert_close(o["rmean"], (1 - U.MOM) * rm0 + U.MOM * x[0], rtol=1e-14, atol=0)
            continue
        y = y.reshape(C, M).t() + ra
        y = y.clamp(min=0) if relu else y
        y.backward(dy)
        tol = dict(rtol=1e-10, atol=1e-10)
        torch.testing.assert_close(o["y"], y.detach(), **tol)
        torch.testing.assert_close(o["rmean"], rm, **tol)
        torch.testing.assert_close(o["rvar"], rv, **tol)
        b = U.bn_backward64(dy, o["pos"].double() if relu else None, x, ga, o["mean"], o["rstd"])
        torch.testing.assert_close(b["dx"], xa.grad, **tol)
        torch.testing.assert_close(b["dgamma"], wa.grad, **tol)
        torch.testing.assert_close(b["dbeta"], ba.grad, **tol)
        torch.testing.assert_close(b["dres"], ra.grad, **tol)


CPU_PARTS = {"apply-bf16": lambda: U.apply_cases(dts=("bf16",)), "apply-f32": lambda: U.apply_cases(dts=("f32",)),
             "stat-bf16": lambda: U.stat_cases(dts=("bf16",)), "stat-f32": lambda: U.stat_cases(dts=("f32",)),
             "tile": U.tile_cases, "chain": U.chain_cases,
             "u0": lambda: [c for c in U.worker_cases({"MPIT_BN_APPLY_U": "0"}) if c["M"] == U.U0_M]}
GEN = {"apply": U.gen_apply, "fwdc": U.gen_apply, "pair": U.gen_apply, "pairb": U.gen_apply, "bwdc": U.gen_apply,
       "stat": U.gen_stat, "tile": U.gen_tile, "chain": U.gen_chain}


@pytest.mark.parametrize("part", CPU_PARTS)
def test_generators_meet_their_exactness_bounds(part):
    """Every case's generator asserts what the case relies on: each fmaf / add of an apply pass
    exact in fp32 with bf16 ties among the bf16 results, every shifted sum, sum of squares,
    reduced sum and level-1 tile sum below 2^24 units of its granularity."""
    cases = CPU_PARTS[part]()
    for c in cases:
        GEN[c["op"]](c)
    assert len({key(c) for c in cases}) == len(cases)


def test_case_counts_and_coverage():
    ap, st, ti, ch = U.apply_cases(), U.stat_cases(), U.tile_cases(), U.chain_cases()
    assert (len(ap), len(ti), len(ch)) == (12 * 2 * 31, 2 * 2 * 30, 14) and len(st) >= 200
    shapes = {(c["C"], c["M"]) for c in ap}
    assert {(8, M) for M in U.C8_M} <= shapes and {(C, M) for C in (24, 72, 64, 512, 2048, 4096, 8192)
                                                   for M in (1, 3, 129)} <= shapes
    assert {c["apre"] for c in ap} == {0, 1, 2}
    # the pre-filled amax values sit in slots a launch hits: block b raises slot b % 16, so slot 0
    # (block 0) in every launch. Both pre-filled kinds include launches of one block and of several:
    # a block is the largest multiple of G = C / 8 threads within 256 (G itself from 256 on), and a
    # thread takes one 8-element vector (two at most) of the M G there are
    def blocks(c):  # (fewest, most) over the MPIT_BN_APPLY_U settings
        G = c["C"] // 8
        blk = G if G >= 256 else 256 // G * G
        return -(-c["M"] * G // (2 * blk)), -(-c["M"] * G // blk)
    for pre in (1, 2):
        nb = [blocks(c) for c in ap if c["apre"] == pre and c["op"] != "apply"]
        assert any(hi == 1 for (_, hi) in nb) and any(lo >= 2 for (lo, _) in nb)
    ss = {(c["C"], c["M"]) for c in st}
    assert {(2048, 4095), (2048, 4096), (2048, 4097), (2048, 5000), (1024, 8200), (8192, 1), (4096, 129),
            (200, 333), (8, 1), (64, 2), (2048, 7)} <= ss
    assert {c["nt"] for c in ti} == {1, 2, 31, 32, 33, 64, 65, 4096, 4100}
    assert {c["last"] for c in ti if c["dir"] == "fwd"} == {1, 64, 127, 128}
    assert {(2048, 4097), (8, 513)} <= {(c["C"], c["M"]) for c in ch}
    for env in VARIANTS:
        w = U.worker_cases(env)
        assert {c["op"] for c in w} == {"apply", "fwdc", "pair", "pairb", "bwdc", "tile", "chain"}
        assert sum(c["M"] == U.U0_M for c in w) == (2 if env.get("MPIT_BN_APPLY_U") == "0" else 0)


def test_tile_oracle_equals_the_statistics_of_the_rows():
    """the documented combination of the per-tile (mean, M2) is the mean and variance of the data"""
    for c in (dict(op="tile", dir="fwd", dt="f32", C=8, nt=33, last=127, M=128 * 32 + 127),
              dict(op="tile", dir="fwd", dt="bf16", C=72, nt=2, last=1, M=129),
              dict(op="tile", dir="fwd", dt="f32", C=8, nt=1, last=64, M=64)):
        d, o = U.gen_tile(c)
        ref = U.bn_forward64(d["x"], d["gamma"], d["beta"], d["rmean0"], d["rvar0"])
        for k in ("mean", "var", "scale", "shift", "rmean", "rvar"):
            torch.testing.assert_close(o[k], ref[k], rtol=1e-11, atol=1e-11)


def test_helpers_notice_one_bit_one_guard_one_ulp():
    # a flipped mask bit, a touched mask guard byte
    ref = torch.arange(40, dtype=torch.uint8)
    full, _ = U.byte_buf(40, "cpu")
    full[U.BPRE:U.BPRE + 40] = ref
    U.check_bytes(full, ref, "m")
    flip = full.clone()
    flip[U.BPRE + 7] ^= 0x10
    with pytest.raises(AssertionError):
        U.check_bytes(flip, ref, "m")
    for at in (U.BPRE - 1, U.BPRE + 40):
        g = full.clone()
        g[at] = 0
        with pytest.raises(AssertionError):
            U.check_bytes(g, ref, "m")
    pos = torch.rand(5, 24) > 0.5
    assert torch.equal(U.unpack_mask(U.pack_mask(pos), 5, 24) > 0, pos)
    assert int(U.pack_mask(torch.tensor([[0, 1, 0, 0, 0, 0, 0, 1]]) > 0)[0]) == 0x82
    # a touched guard row, a value 1 ulp off
    out, _ = out_buf(3, 8, F32, "cpu")
    assert_guards(out, 3, 8, "g")
    out[PRE - 1, 7] = 0
    with pytest.raises(AssertionError):
        assert_guards(out, 3, 8, "g")
    a = torch.tensor([1.0, 300.0])
    b = a.clone().view(torch.int32)
    b[1] += 1
    with pytest.raises(AssertionError):
        same_bits(a, b.view(F32), "u")
    # the ulp tolerance: n + 1 ulp of the largest term passes, one more fails
    ref = torch.tensor([1.5, -3.0], dtype=torch.float64)
    U.assert_within((ref + 2 * 2.0 ** -23 * torch.tensor([1.0, 2.0])).float(), ref, [ref], 1, "t")
    with pytest.raises(AssertionError):
        U.assert_within((ref + 3 * 2.0 ** -23 * torch.tensor([1.0, 2.0])).float(), ref, [ref], 1, "t")
    with pytest.raises(AssertionError):
        U.assert_within(torch.tensor([float("nan"), -3.0]), ref, [ref], 1, "t")
    assert U.bf16_ties(torch.tensor([257.0, -303.0, 256.0, 301.5, 3.0], dtype=torch.float64)).tolist() == \
        [True, True, False, False, False]
    # amax: a lowered slot, a slot above the maximum, a store outside the slots
    class _B:
        @staticmethod
        def bound_floats():
            return U.NSLOT * U.SSTRIDE
    # 'above0': what a kernel leaves that takes a maximum with the slot's contents (2 blocks)
    am, _ = U.amax_buf(_B, "cpu", "above0")
    am[PRE, U.SSTRIDE] = U._bits(7.0)
    U.check_amax(am, "above0", 7.0, "a")
    # a plain store of block 0's maximum over slot 0, a lowered slot, a slot above the maximum,
    # a store outside the slots
    for (i, v) in ((0, 7.0), (2 * U.SSTRIDE, 0.0), (U.SSTRIDE, 8.0), (1, 0.0)):
        bad = am.clone()
        bad[PRE, i] = U._bits(v)
        with pytest.raises(AssertionError):
            U.check_amax(bad, "above0", 7.0, "a")
    # 'below': slot 0 raised to the maximum passes; left at its earlier value, or the maximum
    # missing from every slot, fails
    am, _ = U.amax_buf(_B, "cpu", "below")
    with pytest.raises(AssertionError):
        U.check_amax(am, "below", 7.0, "a")
    am[PRE, 0] = U._bits(6.0)
    with pytest.raises(AssertionError):
        U.check_amax(am, "below", 7.0, "a")
    am[PRE, U.SSTRIDE] = U._bits(7.0)
    U.check_amax(am, "below", 7.0, "a")
    am, _ = U.amax_buf(_B, "cpu", "raise")
    am[PRE, 2 * U.SSTRIDE] = U._bits(6.0)
    with pytest.raises(AssertionError):  # the maximum itself is missing
        U.check_amax(am, "raise", 7.0, "a")


# ------------------------------------------------------------------ 1. apply passes, given coefficients
@gpu
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("op", tuple(U.APPLY_OPS))
def test_apply_exact(op, dt):
    """bn_act_apply, bn_act_fwd(coef) with mask and amax, bn_pair_apply, bn_pair_bwd_apply and
    bn_act_bwd(coef): every output element bitwise the fp64 value rounded once, the mask bytes
    the packed t > 0 bits, amax raised (never zeroed, never lowered) to exactly max |out|. C = 8
    walks the wave-chunk, block and 2-slot grid tails; 24 / 72 the 255- / 252-thread blocks;
    64 / 512 / 2048 the split fp32 layout; 4096 / 8192 blocks above 256 threads."""
    _run(U.apply_cases(ops=(op,), dts=(dt,)))


# ------------------------------------------------------------------ 2. stand-alone statistics / reduction
@gpu
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("dir", ("fwd", "bwd"))
def test_stats_exact(dir, dt):
    """bn_act_fwd with y = 0 / bn_act_bwd with dx = 0 on integer data with a large common offset:
    a row dropped or counted twice moves an integer sum by a whole unit. Block seams, the
    512-block cap, C % 64 != 0, C = 4096 and 8192 (64 KiB of dynamic LDS), M = 1."""
    _run([c for c in U.stat_cases(dts=(dt,)) if c["dir"] == dir])


# ------------------------------------------------------------------ 3. tile partials as input
@gpu
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("dir", ("fwd", "bwd"))
def test_tile_finalize_exact(dir, dt):
    """bn_act_fwd(stats, nstat) / bn_act_bwd(part, npart) on synthetic partials: one group, two,
    three with a short last one, the 128-group cap; ragged last tiles of 1, 64 and 127 rows."""
    _run([c for c in U.tile_cases(dts=(dt,)) if c["dir"] == dir])


@gpu
def test_tile_finalize_rejects_bad_counts_and_wide_channels():
    m = _m()
    x = torch.zeros(300, 4096, device="cuda")
    v = torch.zeros(8 * 4096, device="cuda")
    ws = torch.zeros(m.bn_workspace_floats(4096), device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def fwd(C, nstat):
        m.bn_act_fwd(0, s, False, x.data_ptr(), 0, 0, 300, C, v.data_ptr(), v.data_ptr(), 0, 0, v.data_ptr(),
                     v.data_ptr(), ws.data_ptr(), 0.1, 1e-5, True, 0, stats=v.data_ptr(), nstat=nstat)

    for nstat in (2, 4):  # ceil(300 / 128) = 3
        with pytest.raises(ValueError, match="stats tiles"):
            fwd(64, nstat)
    with pytest.raises(ValueError, match="too many channels"):
        fwd(4096, 3)
    with pytest.raises(ValueError, match="too many channels"):
        m.bn_act_bwd(0, s, False, x.data_ptr(), 0, x.data_ptr(), 0, 0, 300, 4096, v.data_ptr(), v.data_ptr(),
                     v.data_ptr(), v.data_ptr(), v.data_ptr(), ws.data_ptr(), False, part=v.data_ptr(), npart=3)
    fwd(64, 3)
    torch.cuda.synchronize()


@gpu
def test_tile_finalize_ticket_sets_wrap():
    """136 tile-finalize launches back to back on one stream (the 64 rotating ticket sets wrap
    twice), alternating forward / backward, C = 64 / 2048 and 1 / 3 groups; every launch checked."""
    m = _m()
    cases = []
    for i in range(136):
        C, nt, dr = (64, 2048)[(i // 2) % 2], (20, 65)[(i // 4) % 2], ("fwd", "bwd")[i % 2]
        c = dict(op="tile", dir=dr, dt="bf16" if C == 2048 else "f32", C=C, nt=nt)
        c.update(dict(last=127, M=128 * (nt - 1) + 127) if dr == "fwd" else dict(M=32 * nt + 5))
        cases.append(c)
    gens = {key(c): U.gen_tile(c) for c in cases[:8]}  # the 8 distinct cases, generated once
    assert len(gens) == 8 and all(key(c) in gens for c in cases)
    shared, pending = {}, []
    for c in cases:
        out, sh, keep = U.launch_tile(m, c, sync=False, shared=shared.get(key(c)), gen=gens[key(c)])
        shared[key(c)] = sh
        pending.append((out, keep))
    torch.cuda.synchronize()
    bad = []
    for c, (out, _) in zip(cases, pending):
        try:
            U.check_tile(c, {k: v.cpu() for k, v in out.items()}, gen=gens[key(c)])
        except AssertionError as e:
            bad.append(str(e)[:300])
    print(f"{len(cases)} launches compared, {len(bad)} failed")
    assert not bad, f"{len(bad)} of {len(cases)} launches failed:\n" + "\n".join(bad[:12])


# ------------------------------------------------------------------ 4. the whole chain
@gpu
@pytest.mark.parametrize("dt", DTS)
def test_chain(dt):
    """bn_act_fwd (stats, finalize, apply with residual, mask, amax) then bn_act_bwd with the mask
    it produced, dres and amax."""
    _run(U.chain_cases(dts=(dt,)))


# ------------------------------------------------------------------ 5. environment variants
VARIANTS = ({"MPIT_BN_APPLY_U": "0"}, {"MPIT_BN_APPLY_U": "1"}, {"MPIT_BN_APPLY_U": "2"}, {"MPIT_BN_SPLIT": "0"},
            {"MPIT_BN_FIN_LANES": "16"})
# a child takes 2.7 - 3.7 s on an MI355X machine (import, 248 launches, 250 under MPIT_BN_APPLY_U=0
# with the two 8.4 M-element cases, save; measured per setting); the limit leaves room for a cold
# file cache
CHILD_TIMEOUT = 60


@gpu
@pytest.mark.parametrize("env", VARIANTS, ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_variants_exact(env, tmp_path):
    path = str(tmp_path / "out.pt")
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mp", "bn_exact_check.py"), path],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    print(f"child {env}: {time.time() - t0:.1f}s {r.stdout.strip()[-80:]}")
    assert r.returncode == 0, r.stderr[-3000:]
    saved = torch.load(path, weights_only=True)
    by_case = {}
    for k, v in saved.items():
        ck, name = k.split("|")
        by_case.setdefault(ck, {})[name] = v
    cases = U.worker_cases(env)
    assert len(cases) == len(by_case)
    _check_all(cases, lambda c: by_case[key(c)])
