"""Exact per-element oracles for the MFMA GEMMs (csrc/kernels/gemm.hip) at tile and ring edges.

fp32 accumulation is exact in any order when every partial sum is representable, so inputs
built from small integers (`narrow`) or from 14-bit values against small integers (`wide`)
must give the same bits on every tile shape, ring depth, split plan and bf16x6 / fp16x3 split:
the fp64 product rounded once to the output type. Each case asserts its own exactness bound
on the CPU first (tests/gemm_exact_util.py). Operands live inside larger allocations whose
padding is NaN; outputs and partial buffers are pre-filled with a sentinel bit pattern, and
everything outside the region a call owns must still hold it afterwards."""
import os
import subprocess
import sys
import time

import pytest
import torch

import gemm_exact_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu


def _m():
    from mpit_amd._ext import native

    return native()


def _run(cases):
    """Launch and check every case; mismatches are collected so one run names them all (anything
    but a failed comparison, a HIP error for instance, ends the run at once)."""
    m = _m()
    bad = []
    for c in cases:
        res = U.LAUNCH[c["op"]](m, c)
        try:
            U.CHECK[c["op"]](c, res)
        except AssertionError as e:
            bad.append(str(e)[:300])
    print(f"{len(cases)} launches compared, {len(bad)} failed")
    assert not bad, f"{len(bad)} of {len(cases)} cases failed:\n" + "\n".join(bad[:12])
    return len(cases)


# ------------------------------------------------------------------ CPU: the net itself
def test_generators_meet_their_exactness_bounds():
    """Every case's inputs sit on their granularity with |A||B|^T below 2^24 units (asserted by
    the generators), across all the lists the GPU tests and the worker run."""
    n = 0
    for c in U.nt_cases() + U.nt256_cases():
        U.gen_nt(c)
        n += 1
    for c in U.epi_cases():
        U.epi_oracle(c, U.gen_epi(c))
        n += 1
    for c in U.tn_cases():
        U.gen_tn(c)
        n += 1
    for i in range(len(U.CONV_SHAPES)):
        U.gen_conv(dict(shape=i))
        n += 1
    assert n > 1000
    # an inexact case fails loudly
    big = torch.full((1, 160), 4000.0)
    with pytest.raises(AssertionError):
        U.assert_exact(big, big, (2.0 ** -10, 1.0))
    with pytest.raises(AssertionError):
        U.assert_exact(torch.full((1, 16), 0.3), torch.ones(1, 16), (1.0, 1.0))


def _bf16_planes(x):
    h = x.to(torch.bfloat16).float()
    m = (x - h).to(torch.bfloat16).float()
    lo = ((x - h) - m).to(torch.bfloat16).float()
    return h, m, lo


def test_wide_family_needs_more_than_one_plane_and_drops_nothing():
    from mpit_amd.ops.conv import f16_planes

    g = torch.Generator().manual_seed(3)
    w, n = U.wide((129, 160), g), U.narrow((64, 160), g)
    # bf16x6: wide = h + m exactly with m in use; narrow is a single plane
    h, m, lo = _bf16_planes(w)
    assert (m != 0).any() and not lo.any() and torch.equal(h + m, w)
    nh, nm, nl = _bf16_planes(n)
    assert torch.equal(nh, n) and not nm.any() and not nl.any()
    # the products the bf16x6 kernels drop (ml, lm, ll), either way round
    for (a, b) in (((h, m, lo), (nh, nm, nl)), ((nh, nm, nl), (h, m, lo))):
        for (p, q) in ((1, 2), (2, 1), (2, 2)):
            assert not (a[p].abs() @ b[q].abs().t()).any()
    # fp16x3: the l plane of wide is in use, (h + l / 2^11) / 2^e is wide exactly, narrow has none
    wp = f16_planes(w, w.abs().max().reshape(1))
    np_ = f16_planes(n, n.abs().max().reshape(1))
    assert wp[1].float().abs().max() > 0 and not np_[1].any()
    e = 14 - torch.frexp(w.abs().max())[1].item()
    assert torch.equal((wp[0].double() + wp[1].double() / 2048) / 2.0 ** e, w.double())
    # the dropped fp16 product (ll) is zero either way round
    assert not (wp[1].float().abs() @ np_[1].float().abs().t()).any()


def test_epilogue_oracles_agree_with_independent_formulations():
    import numpy as np

    for c in (dict(op="epi", path="f32", epi="bnred2", M=257, N=64, K=32),
              dict(op="epi", path="bf16", epi="bnred", M=129, N=192, K=96)):
        d = U.gen_epi(c)
        M, N = c["M"], c["N"]
        C, o = U.epi_oracle(c, d)
        # the bit mask through numpy's unpackbits
        bits = torch.from_numpy(np.unpackbits(d["mask"].numpy(), bitorder="little").reshape(M, N).astype(np.float64))
        assert torch.equal(bits, U.unpack_mask(d["mask"], M, N))
        # the BN partials as fp64 autograd of a batch-norm backward: out = (x - mean) w + b with the
        # loss sum(out dz) over a tile has dL/db = sum dz and dL/dw = sum dz (x - mean)
        dz = C.double() * bits
        for name, xk, mk in (("part", "x", "mean"), ("part2", "x2", "mean2")):
            if name not in o:
                continue
            for t in range((M + 127) // 128):
                w = torch.ones(N, dtype=torch.float64, requires_grad=True)
                b = torch.zeros(N, dtype=torch.float64, requires_grad=True)
                rows = slice(128 * t, 128 * t + 128)
                out = (d[xk].double()[rows] - d[mk].double()) * w + b
                (out * dz[rows]).sum().backward()
                assert torch.equal(b.grad.float(), o[name][t, 0]) and torch.equal(w.grad.float(), o[name][t, 1])
    # cin + cmask: the oracle against a per-element Python loop
    c = dict(op="epi", path="bf16", epi="cmask", M=1, N=64, K=32)
    d = U.gen_epi(c)
    C, _ = U.epi_oracle(c, d)
    for n in range(64):
        p = float(sum(float(d["a"][0, k]) * float(d["b"][n, k]) for k in range(32)))
        bit = (int(d["cmask"][n // 8]) >> (n % 8)) & 1
        want = torch.tensor(torch.tensor(p).to(torch.bfloat16).item() + bit * float(d["cin"][0, n])).to(torch.bfloat16)
        assert C[0, n].item() == want.item()
    # the stats check accepts Welford partials of its own data and rejects a shifted mean
    x = torch.randn(130, 64, dtype=torch.float64)
    part = torch.stack([torch.stack([r.mean(0), ((r - r.mean(0)) ** 2).sum(0)]) for r in (x[:128], x[128:])]).float()
    full = torch.full((U.PRE + 2 + U.POST, 128), U.SENT32, dtype=torch.int32)
    full[U.PRE:U.PRE + 2] = part.view(2, 128).view(torch.int32)
    U.check_stats(full, x, 130, 64, "self")
    full[U.PRE, 0] = torch.tensor(float(part[0, 0, 0]) + 1e-3).view(torch.int32)
    with pytest.raises(AssertionError):
        U.check_stats(full, x, 130, 64, "self")


def test_guard_and_bit_checks_notice_one_element():
    full, _ = U.out_buf(5, 16, torch.bfloat16, "cpu")
    U.assert_guards(full, 5, 8, "g")
    full[U.PRE + 5, 0] = 0
    with pytest.raises(AssertionError):
        U.assert_guards(full, 5, 8, "g")
    a = torch.zeros(4, 4)
    b = a.clone()
    b[3, 3] = -0.0
    with pytest.raises(AssertionError):
        U.same_bits(a, b, "z")


# ------------------------------------------------------------------ 1. gemm_nt, plain
@gpu
@pytest.mark.parametrize("path", U.NT_PATHS)
def test_gemm_nt_exact(path):
    """M x N x K cross product of one path (bf16, fp32 bf16x6 FM 3 / FM 1, fp16x3 with B planes
    FM 11, with A and B planes FM 13), padded leading dimensions, NaN padding, guarded C."""
    _run(U.nt_cases((path,)))


@gpu
def test_gemm_nt_exact_256_row_blocks():
    """bf16, K = 2304: 256 x 128 blocks by the deep-K rule, plain and with per-128-row stats."""
    _run(U.nt256_cases())


# ------------------------------------------------------------------ 2. gemm_nt epilogues
@gpu
@pytest.mark.parametrize("path", ("bf16", "f32"))
@pytest.mark.parametrize("epi", U.EPI_KINDS)
def test_gemm_nt_epilogue_exact(path, epi):
    """bf16 with cin: the product is rounded to bf16, then cin is added and the sum rounded
    (csrc/kernels/kernels.h); the cases are chosen so that this differs from one rounding."""
    _run([c for c in U.epi_cases() if c["path"] == path and c["epi"] == epi])


# ------------------------------------------------------------------ 3. gemm_tn
@gpu
@pytest.mark.parametrize("path", U.TN_PATHS)
def test_gemm_tn_exact(path):
    _run([c for c in U.tn_cases() if c["path"] == path])


# ------------------------------------------------------------------ 4. convolutions
@gpu
@pytest.mark.parametrize("path", ("bf16", "f32"))
def test_conv_exact(path):
    """conv_fwd (plain, bias + ReLU, cin, EPI_RELUB), conv_dgrad_strided and conv_wgrad on
    non-square images against fp64 F.conv2d and its autograd."""
    _run([c for c in U.conv_cases() if c["path"] == path])


# ------------------------------------------------------------------ 5. build variants
VARIANTS = ({"MPIT_GEMM_TILE": "256"}, {"MPIT_GEMM_TILE": "256x128"}, {"MPIT_GEMM_STAGES": "4"},
            {"MPIT_F32_MFMA": "native"}, {"MPIT_F32_BK": "16"}, {"MPIT_TN_FUSED": "1"}, {"MPIT_TN_KROWS": "64"},
            # the bf16 4 x 32-row ring (KROWS=64 is the default's 64-row steps), 4 and 2 deep
            {"MPIT_TN_KROWS": "32"}, {"MPIT_TN_KROWS": "32", "MPIT_GEMM_TN_STAGES": "2"},
            {"MPIT_TN_KR_STAGES": "3"}, {"MPIT_TN_F16S": "0"}, {"MPIT_TN_OCC": "1"},
            {"MPIT_F32_BN64": "1"}, {"MPIT_F32_TILE": "256x64"})
# a child takes 3.1 - 3.6 s on an MI355X machine (import, 520 - 700 launches, save; measured per
# setting); the limit leaves room for a cold file cache
CHILD_TIMEOUT = 60


@gpu
@pytest.mark.parametrize("env", VARIANTS, ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_variants_exact(env, tmp_path):
    path = str(tmp_path / "out.pt")
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mp", "gemm_exact_check.py"), path],
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
    bad = []
    for c in cases:
        try:
            U.CHECK[c["op"]](c, by_case[U.key(c)])
        except AssertionError as e:
            bad.append(str(e)[:300])
    print(f"{len(cases)} launches compared, {len(bad)} failed")
    assert not bad, f"{len(bad)} of {len(cases)} cases failed:\n" + "\n".join(bad[:12])
