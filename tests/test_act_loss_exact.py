"""Exact oracles for relu_bias_bwd and col_sums (csrc/kernels/act.hip) and softmax_xent
(csrc/kernels/loss.hip), through the raw bindings of mpit_amd._ext.native().

relu_bias_bwd moves dy where y > 0 and sums integer columns, col_sums sums integer partial rows:
every bit is pinned whatever the order of the sums (|column sum| < 2^24, asserted per case). The
ReLU mask sees -1, -0.0, +0.0, the smallest subnormal, 1 and NaN. softmax_xent is checked bitwise on
structural rows (logits m at j columns, m - 200 elsewhere: exp is exactly 1 or 0) and, on random
logits, per row and per element against fp64: its largest error may be at most twice the largest
error of PyTorch's fp32 log_softmax / nll_loss / softmax gradient on the same logits and device,
plus one fp32 ulp of the largest term (tests/test_fp32_path.py's fp32 class; both errors are
printed). Logits rows end in NaN columns (ldx > C) and NaN rows, outputs and workspaces sit between
sentinels. Helpers in tests/pool_exact_util.py.

Measured on an MI355X machine: the GPU tests of this file take 3.5 s together; test_relu_bias_bwd_exact
takes 1.3 - 1.5 s per type (C = 8192 x M = 5000 and the 4.2 M-row case past the block cap, both checked
on the device), every other test stays below 0.2 s."""
import pytest
import torch
import torch.nn.functional as F

import pool_exact_util as U
from gemm_exact_util import key

gpu = pytest.mark.gpu


def _m():
    from mpit_amd._ext import native

    return native()


def _run(cases, launch=None, check=None):
    U.run_cases(_m(), cases, launch, check)


# ------------------------------------------------------------------ CPU: the net itself
def test_loss_oracle_matches_fp64_cross_entropy():
    g = torch.Generator().manual_seed(5)
    for (rows, C) in ((1, 1), (3, 10), (40, 257)):
        x = torch.randn(rows, C, generator=g, dtype=torch.float64) * 4
        t = torch.randint(0, C, (rows,), generator=g)
        xa = x.clone().requires_grad_(True)
        ref = F.cross_entropy(xa, t, reduction="none")
        ref.sum().backward()
        loss, d = U.xent64(x, t)
        torch.testing.assert_close(loss, ref.detach(), rtol=1e-13, atol=1e-13)
        torch.testing.assert_close(d, xa.grad, rtol=1e-13, atol=1e-13)
    loss, d = U.xent64(x, torch.where(torch.arange(rows) % 2 == 0, -1, C))
    assert loss.isnan().all()
    torch.testing.assert_close(d, torch.softmax(x, 1), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("part", ("rbb", "cs", "xent"))
def test_generators_meet_their_exactness_bounds(part):
    """integer columns below 2^24 in all (the cases past BIG elements are only counted here: their
    bound is the same product), structural logits exact in their type with the maxima where the
    docstring says"""
    if part == "rbb":
        cases = U.rbb_cases()
        for c in cases:
            lim = 100 if c["M"] * 100 < 2 ** 24 else 3
            assert c["M"] * lim < 2 ** 24
            if not U.big(c):
                d = U.gen_rbb(c)
                assert float(d["dy"].double().abs().max()) <= lim
                assert (d["y"].double() > 0).float().mean().item() < 0.6
    elif part == "cs":
        cases = U.cs_cases()
        for c in cases:
            if c["nb"] * c["C"] <= 1 << 18:
                assert U.gen_cs(c).shape == (c["nb"], c["C"])
    else:
        cases = U.xent_cases("struct") + U.xent_cases("num")
        for c in cases:
            if c["rows"] * c["C"] > 1 << 16:
                continue
            d = U.gen_xent(c)
            if c["kind"] == "struct":
                x = d["x"].double()
                assert torch.equal((x == d["m"][:, None]).sum(1), d["j"]) and set(d["j"].tolist()) <= {1, 2, 4, 8}
                assert torch.equal(x.amax(1), d["m"])
    assert len({key(c) for c in cases}) == len(cases)


def test_case_counts_and_coverage():
    rb = U.rbb_cases()
    assert {c["C"] for c in rb} == {8, 24, 64, 1024, 2040, 2400, 8192}
    # blocks of 256 and 255 threads; one row slot with 255, 300 and 1024 threads; 32 KiB of LDS
    assert [U.rbb_rows(C) for C in (8, 24, 64, 1024, 2040, 2400, 8192)] == [256, 85, 32, 2, 1, 1, 1]
    for C in U.RBB_C:
        R = U.rbb_rows(C)
        assert {c["M"] for c in rb if c["C"] == C and c["db"]} >= {1, 15, 16 * R - 1, 16 * R, 16 * R + 1, 5000}
        assert any(c["C"] == C and not c["db"] for c in rb)
    assert any(c["C"] == 8 and c["M"] > 1024 * 16 * 256 for c in rb)
    cs = U.cs_cases()
    assert {(c["nb"], c["C"]) for c in cs} == {(nb, C) for nb in (1, 15, 16, 17, 64, 65, 66, 1000, 1024, 8192)
                                               for C in (8, 64, 72, 1000)}
    assert all({c["ld"] for c in cs if c["C"] == C} == {C, 2 * C, C + 8} for C in (8, 64, 72, 1000))
    assert all(c["mid"] for c in cs if c["nb"] > 64) and {c["mid"] for c in cs if c["nb"] <= 64} == {0, 1}
    for kind in ("struct", "num"):
        xe = U.xent_cases(kind)
        assert {(c["C"], c["rows"], c["dt"]) for c in xe} == {(C, r, dt) for C in (1, 2, 10, 255, 256, 257, 513, 1000, 4097)
                                                              for r in (1, 3, 300) for dt in U.DTS}
        assert all({c["ldx"] for c in xe if c["C"] == C} == {C, (C + 63) // 64 * 64} for C in U.XE_C)
        assert {(c["scale"], c["dt"]) for c in xe} == {(s, dt) for s in (1.0, 2.0 ** -8) for dt in U.DTS}
    # structural rows: maxima in column 0, in the last column, past the first 256-column sweep
    d = U.gen_xent(dict(op="xent", kind="struct", dt="f32", C=513, ldx=576, rows=300, scale=1.0))
    first = (d["x"].double() == d["m"][:, None]).double().argmax(1)
    assert {0, 256, 512} <= set(first.tolist()) and {-1, 513} <= set(d["t"].tolist())


# ------------------------------------------------------------------ GPU
@gpu
@pytest.mark.parametrize("dt", U.DTS)
def test_relu_bias_bwd_exact(dt):
    """dz bitwise dy where y > 0 else +0.0, db the exact column sum; with db == 0 (no workspace) only
    dz is written. M around 16 R (one block / two), 5000, and past the 1024-block cap at C = 8."""
    _run(U.rbb_cases(dts=(dt,)))


@gpu
def test_relu_bias_bwd_rejects_wide_channels_and_missing_workspace():
    m = _m()
    t = torch.zeros(8200 * 4, device="cuda")
    s, p = torch.cuda.current_stream().cuda_stream, t.data_ptr()
    with pytest.raises(ValueError, match="8192"):
        m.relu_bias_bwd(0, s, 1, 8200, p, p, p, 0, 0, f32=True)
    with pytest.raises(ValueError, match="workspace"):
        m.relu_bias_bwd(0, s, 1, 8, p, p, p, p, 0, f32=True)
    with pytest.raises(ValueError, match="aligned"):
        m.relu_bias_bwd(0, s, 1, 8, p + 4, p, p, 0, 0, f32=True)


@gpu
def test_col_sums_exact():
    """one level (nb <= 64) and two (from 65), ld = C, 2 C and C + 8 with NaN between the rows,
    C = 72 and 1000 (the c < C tail of the last 64-channel block)"""
    _run(U.cs_cases())


@gpu
def test_col_sums_needs_its_workspace_past_64_rows():
    m = _m()
    t = torch.zeros(65 * 8 + 8, device="cuda")
    s, p = torch.cuda.current_stream().cuda_stream, t.data_ptr()
    with pytest.raises(ValueError, match="workspace"):
        m.col_sums(0, s, p, 65, 8, 8, p + 65 * 8 * 4, 0)
    m.col_sums(0, s, p, 64, 8, 8, p + 65 * 8 * 4, 0)
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("dt", U.DTS)
def test_softmax_xent_structural(dt):
    """d bitwise (targets outside [0, C) included: NaN loss, no one-hot subtracted), the loss of the
    rows with one maximum bitwise 0 or 200, the loss of the rows with j > 1 maxima (log j) in the fp32
    class"""
    m, bad = _m(), []
    cases = U.xent_cases("struct", dts=(dt,))
    for c in cases:
        res = U.launch_xent(m, c)
        try:
            more = U.check_xent_struct(c, res)
            U.check_xent_lib(c, res, rows_sel=more)
        except AssertionError as e:
            bad.append(str(e)[:300])
    assert not bad, f"{len(bad)} of {len(cases)} cases failed:\n" + "\n".join(bad[:12])


@gpu
@pytest.mark.parametrize("dt", U.DTS)
def test_softmax_xent_numeric(dt):
    """per-row loss and d / scale against fp64 on 4 randn logits and rows spanning +-30"""
    _run(U.xent_cases("num", dts=(dt,)), launch=U.launch_xent, check=U.check_xent_lib)


@gpu
@pytest.mark.parametrize("dt", U.DTS)
def test_softmax_xent_infinite_rows_give_nan(dt):
    """a row of all -inf and a row holding +inf: NaN, like PyTorch's log_softmax"""
    c = dict(op="xent", kind="inf", dt=dt, C=300, ldx=320, rows=3, scale=1.0)
    x = torch.randn(3, 300, generator=torch.Generator().manual_seed(1))
    x[0] = -U.INF
    x[2, 299] = U.INF
    d = dict(x=x.to(U.dt_of(c)), t=torch.tensor([0, 5, 7]))
    loss, dd = U.xent_got(c, U.launch_xent(_m(), c, d=d))
    lib = F.cross_entropy(x.cuda(), d["t"].cuda(), reduction="none").cpu()
    assert lib.isnan().tolist() == [True, False, True]
    assert loss.isnan().tolist() == [True, False, True] and dd.isnan().all(1).tolist() == [True, False, True]
