"""The opt-in fused per-example gradients of the BiCNN parity rule (csrc/kernels/seq_grad.hip,
ops/seq.py ``per_example_grads``, ``BiCNN(fused_grad=True)``, apps/bicnn.py -fusedGrad).

Accuracy rule (the project's, tests/test_fp32_path.py, tests/test_seq_encoder.py): the relative
error ``|got - ref| / |ref|`` against an fp64 autograd reference of the same model on the CPU is
at most ``2 * e_torch + 1e-9``, e_torch being the error of ``models.bicnn.per_example_grads``
(torch.func.vmap on PyTorch's fp32 ops) on the same GPU for the same inputs; for the whole matrix
and for each of the five parameter blocks, no element left out.

Gradients are discontinuous at the kinks (arg-max ties, the ReLU, the hinge), so the cases are
asserted, on the fp64 reference, to stay away from them; the seeds below were picked on the CPU
for that (SEEDS: of the seeds 0..23, none misses the arg-max / ReLU distances at shape A and two do
at shape B; three more at A and eight at B have no hinge-inactive example at this margin. The
chosen ones keep the example with the interior pad and the repeated word hinge-active).

Shapes (V, D, H, F, k): A = (50, 12, 24, 72, 3) with n = 5, T_q = 6, T_a = 9 (Kp = 80: 8 pad
columns, Fp = 128, WpT needs row padding); B = (60, 100, 200, 300, 2) with n = 3, T = 5 / 7 (F spans
two 256-thread blocks, Fp = 320, no pad columns). The tokens hold a sentence shorter than k, an
interior pad token followed by real ones, a word repeated within a sentence and shared between q
and a_pos, and an example whose a_neg is its q token for token (distance 0)."""
import copy

import pytest
import torch
import torch.nn.functional as F

from mpit_amd.apps import bicnn as app
from mpit_amd.models import bicnn as M
from mpit_amd.models.bicnn import BiCNN, gesd, parity_grad_
from mpit_amd.ops import seq
from mpit_amd.utils.flat import FlatParams

gpu = pytest.mark.gpu
SENT = -12345.0
GUARD = 512

DIMS = {"A": (50, 12, 24, 72, 3), "B": (60, 100, 200, 300, 2)}
SEEDS = {"A": 10, "B": 1}  # picked on the CPU: _kinks() holds (see the module docstring)
MARGIN = 0.009  # the application's default


def _rel(a, ref):
    a, ref = a.double().cpu(), ref.double().cpu()
    return ((a - ref).norm() / (ref.norm() + 1e-300)).item()


def _rule(name, got, lib, ref):
    e, el = _rel(got, ref), _rel(lib, ref)
    print(f"{name}: e = {e:.3e}, e_torch = {el:.3e}")
    assert e <= 2.0 * el + 1e-9, (name, e, el)


def _guarded(shape, device="cuda"):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.float32, device=device)
    return buf, buf[GUARD: GUARD + n].view(shape)


def _guards_ok(buf, view):
    n = view.numel()
    assert (buf[:GUARD] == SENT).all() and (buf[GUARD + n:] == SENT).all(), "write outside the output"
    assert not (view == SENT).any(), "output element never written"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _tokens(name, seed):
    """(q, a_pos, a_neg) int64 on the CPU, pad_idx = 0."""
    V, _, _, _, k = DIMS[name]
    g = torch.Generator().manual_seed(1000 + seed)

    def rnd(n):
        return torch.randint(1, V, (n,), generator=g)

    if name == "A":
        n, Tq, Ta = 5, 6, 9
        ql, pl, nl = [6, 5, 6, 6, 4], [9, 7, k - 1, 8, 9], [7, 5, 9, 6, 8]
    else:
        n, Tq, Ta = 3, 5, 7
        ql, pl, nl = [5, 4, 5], [7, 6, k - 1], [6, 4, 7]
    q, ap, an = (torch.zeros((n, T), dtype=torch.int64) for T in (Tq, Ta, Ta))
    for i in range(n):
        q[i, : ql[i]], ap[i, : pl[i]], an[i, : nl[i]] = rnd(ql[i]), rnd(pl[i]), rnd(nl[i])
    an[1] = 0
    an[1, : ql[1]] = q[1, : ql[1]]  # a_neg == q, token for token: distance 0
    last = n - 1
    q[last, 1] = 0  # an interior pad token followed by real ones
    q[last, 3] = q[last, 0]  # a word repeated within a sentence ...
    sh = last if name == "A" else 1  # (B's last a_pos is the one shorter than k)
    ap[sh, 2] = q[sh, 0]  # ... and shared between q and a_pos
    return q, ap, an


def _model64(name, seed):
    V, D, H, Fn, k = DIMS[name]
    torch.manual_seed(seed)
    m = BiCNN(V, D, H, Fn, k, fused=False, fused_grad=False)
    with torch.no_grad():
        m.embed.weight[0] = 0.5 * torch.randn(D)  # the pad row holds values: nothing may read it as 0
    return m


def _strip(t):
    return t[: int((t != 0).nonzero().max()) + 1] if (t != 0).any() else t[:0]


def _reference(m64, offsets, numel, q, ap, an, margin):
    """fp64 autograd, one example at a time: (g [n, numel], x [n] = margin - sp + sn)."""
    params = [m64.embed.weight, m64.hidden.weight, m64.hidden.bias, m64.conv.weight, m64.conv.bias]
    n = q.shape[0]
    g = torch.zeros((n, numel), dtype=torch.float64)
    xs = []
    for i in range(n):
        eq = m64.encode(q[i: i + 1])
        ep = m64.encode(ap[i: i + 1])
        # the same sentence is the same encoding (a distance of exactly 0, as on the GPU, where
        # the encoder is padding-invariant): encode the question's own row again
        same = torch.equal(_strip(q[i]), _strip(an[i]))
        en = m64.encode(q[i: i + 1] if same else an[i: i + 1])
        x = margin - gesd(eq, ep) + gesd(eq, en)
        gs = torch.autograd.grad(F.relu(x).sum(), params)
        for t, off in zip(gs, offsets):
            g[i, off: off + t.numel()] = t.reshape(-1)
        xs.append(x.detach()[0])
    return g, torch.stack(xs)


def _kinks(m64, q, ap, an, x):
    """The distances of the fp64 reference from the gradient's discontinuities."""
    k = m64.conv.kernel_size[0]
    gaps, relus, cmax = [], [], 0.0
    with torch.no_grad():
        for tok in (q, ap, an):
            h = torch.tanh(m64.hidden(m64.embed(tok)))
            c = F.conv1d(h.transpose(1, 2), m64.conv.weight)  # [B, F, T-k+1], without the bias
            vw = (tok != 0)[:, k - 1:]
            for b in range(tok.shape[0]):
                cv = c[b][:, vw[b]]
                if cv.shape[1] == 0:
                    continue
                cmax = max(cmax, cv.abs().max().item())
                top = cv.topk(min(2, cv.shape[1]), dim=1).values
                if cv.shape[1] > 1:
                    gaps.append((top[:, 0] - top[:, 1]).min().item())
                relus.append((top[:, 0] + m64.conv.bias).abs().min().item())
    return {"gap": min(gaps), "relu": min(relus), "tol": 2.0 ** -18 * cmax, "hinge": x.abs().min().item(),
            "active": int((x > 0).sum()), "inactive": int((x < 0).sum())}


def _kinks_ok(kk):
    return (kk["gap"] >= kk["tol"] and kk["relu"] >= kk["tol"] and kk["hinge"] >= 1e-5 and kk["active"] >= 1
            and kk["inactive"] >= 1)


_CASES = {}


def _case(name):
    """Everything the GPU tests share for a shape, computed once and never modified: the fused and
    the PyTorch model on the GPU with their flat parameters, the fp64 model, the tokens, the fp64
    reference, PyTorch's fp32 result and the fused result with its intermediates."""
    if name in _CASES:
        return _CASES[name]
    seed = SEEDS[name]
    m64 = _model64(name, seed)
    V, D, H, Fn, k = DIMS[name]
    fused = BiCNN(V, D, H, Fn, k, fused=False, fused_grad=True)
    fused.load_state_dict(m64.state_dict())
    plain = copy.deepcopy(m64)
    fused, plain, m64 = fused.cuda().eval(), plain.cuda().eval(), m64.double().eval()
    ff, fp = FlatParams(fused), FlatParams(plain)
    q, ap, an = _tokens(name, seed)
    ref, x = _reference(m64, ff.offsets, ff.numel, q, ap, an, MARGIN)
    dq, dp, dn = q.cuda(), ap.cuda(), an.cuda()
    lib = M.per_example_grads(plain, fp, dq, dp, dn, MARGIN)
    parts = {}
    got, err = seq.per_example_grads(fused, ff, dq, dp, dn, MARGIN, parts=parts)
    torch.cuda.synchronize()
    c = dict(name=name, m64=m64, fused=fused, plain=plain, ff=ff, fp=fp, q=q, ap=ap, an=an, dq=dq, dp=dp, dn=dn,
             ref=ref, x=x, lib=lib, got=got, err=err, parts=parts, n=q.shape[0])
    _CASES[name] = c
    return c


def _blocks(flat):
    names = ("embed.weight", "hidden.weight", "hidden.bias", "conv.weight", "conv.bias")
    return [(nm, off, off + p.numel()) for nm, p, off in zip(names, flat.params, flat.offsets)]


# ------------------------------------------------------------------------------ CPU tier

def test_fused_grad_model_on_cpu_is_the_pytorch_path():
    torch.manual_seed(0)
    base = BiCNN(60, 8, 12, 16, 2, fused=False, fused_grad=False)
    plain, fused = copy.deepcopy(base), BiCNN(60, 8, 12, 16, 2, fused=False, fused_grad=True)
    fused.load_state_dict(base.state_dict())
    assert fused.fused_grad and not plain.fused_grad and not fused.fused
    assert not fused.fused_grad_ok(torch.zeros(1, 2, dtype=torch.int64))
    fa, fb = FlatParams(plain), FlatParams(fused)
    n, t = 7, 9
    q, ap, an = (torch.randint(1, 60, (n, t)) for _ in range(3))
    q[:, 7:] = 0
    an[2, 5:] = 0
    before = dict(seq.COUNTERS)
    la = parity_grad_(plain, fa, q, ap, an, 0.3, 0.0, 1e-4, 0.5, chunk=3)
    mid = dict(seq.COUNTERS)
    lb = parity_grad_(fused, fb, q, ap, an, 0.3, 0.0, 1e-4, 0.5, chunk=3)
    assert mid == before  # a plain model touches no counter
    assert torch.equal(_bits(fa.grad), _bits(fb.grad)) and torch.equal(_bits(la.reshape(1)), _bits(lb.reshape(1)))
    assert fa.grad.abs().max() > 0
    assert seq.COUNTERS["pegrad_fallback"] == before["pegrad_fallback"] + 1
    assert seq.COUNTERS["pegrad_fused"] == before["pegrad_fused"]
    for key in ("encode_fused", "encode_fallback", "gesd_fused", "gesd_fallback"):
        assert seq.COUNTERS[key] == before[key]


def test_fused_grad_flag_and_default(monkeypatch):
    monkeypatch.delenv("MPIT_BICNN_FUSED_GRAD", raising=False)
    monkeypatch.delenv("MPIT_BICNN_FUSED", raising=False)
    assert app.build_args(["-fusedGrad"]).fusedGrad is True
    assert not app.build_args([]).fusedGrad and not app.build_args(["-fusedEncoder"]).fusedGrad
    assert not app.build_args(["-fusedGrad"]).fusedEncoder
    assert BiCNN(30, 8, 12, 20, 2).fused_grad is False
    assert BiCNN(30, 8, 12, 20, 2, fused_grad=app.build_args([]).fusedGrad).fused_grad is False
    m = BiCNN(30, 8, 12, 20, 2, fused_grad=app.build_args(["-fusedGrad"]).fusedGrad)
    assert m.fused_grad is True and m.fused is False  # independent of the encoder's switch
    assert BiCNN(30, 8, 12, 20, 2, fused=True).fused_grad is False
    monkeypatch.setenv("MPIT_BICNN_FUSED_GRAD", "1")
    assert BiCNN(30, 8, 12, 20, 2).fused_grad is True and BiCNN(30, 8, 12, 20, 2).fused is False
    assert BiCNN(30, 8, 12, 20, 2, fused_grad=False).fused_grad is False


def test_pack_conv_weight_t_cpu():
    torch.manual_seed(3)
    for Fn, H, k in ((72, 24, 3), (300, 200, 2)):
        w = torch.randn(Fn, H, k)
        wp = seq.pack_conv_weight(w)
        wt = seq.pack_conv_weight_t(w)
        Fp, Kp = wp.shape
        assert wt.shape == (seq.round_up(Kp, 64), Fp) and wt.is_contiguous()
        assert torch.equal(wt[:Kp], wp.t()) and (wt[Kp:] == 0).all()
        again = seq.pack_conv_weight_t(w * 2, wt)  # the refill of the persistent buffer
        assert again is wt and torch.equal(wt[:Kp], 2 * wp.t()) and (wt[Kp:] == 0).all()


@pytest.mark.parametrize("name", ["A", "B"])
def test_cases_hold_what_they_promise(name):
    """The token patterns of the module docstring (no GPU needed)."""
    k = DIMS[name][4]
    q, ap, an = _tokens(name, SEEDS[name])
    lens = lambda t: (t != 0).sum(1)  # noqa: E731
    assert (lens(ap) == k - 1).any()  # shorter than k
    assert any(torch.equal(_strip(q[i]), _strip(an[i])) for i in range(q.shape[0]))
    assert any((row[: len(_strip(row))] == 0).any() for row in q)  # an interior pad
    assert any(len(set(_strip(r).tolist()) - {0}) < int((_strip(r) != 0).sum()) for r in q)  # repeated
    assert any(set(_strip(q[i]).tolist()) & set(_strip(ap[i]).tolist()) - {0} for i in range(q.shape[0]))  # shared


# ------------------------------------------------------------------------------ GPU tier

@gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_forward_identity(name):
    c = _case(name)
    P, n = c["parts"], c["n"]
    V, D, H, Fn, k = DIMS[name]
    tok = P["tok"]
    S, T = tok.shape
    Fp, Kp = seq.packed_shape(Fn, H, k)
    assert S == 3 * n and T == 9 - 2 * (name == "B") and P["c"].shape == (S * T, Fp)
    # y: the fused encoder's bits (the switch of the encoder is off on this model: call it directly)
    with torch.no_grad():
        y = seq.encode(c["fused"], tok)
        yq = seq.encode(c["fused"], c["dq"])  # ... also at the questions' own width
    assert torch.equal(_bits(P["y"]), _bits(y)) and torch.equal(_bits(P["y"][:n]), _bits(yq))
    assert torch.equal(_bits(P["y"][1]), _bits(P["y"][2 * n + 1]))  # a_neg == q: the same bits
    short = int(((c["ap"] != 0).sum(1) == k - 1).nonzero()[0])
    assert (_bits(P["y"][n + short]) == 0).all() and (P["arg"][n + short] == -1).all()
    assert P["den"][n + short].item() == torch.tensor(c["fused"].norm.eps, dtype=torch.float32).item()
    # sp, sn: gesd_gather's bits; err from them
    idx = torch.arange(n, device="cuda").unsqueeze(1)
    sp = seq.gesd_gather(P["y"][:n].contiguous(), P["y"][n: 2 * n].contiguous(), idx)[:, 0]
    sn = seq.gesd_gather(P["y"][:n].contiguous(), P["y"][2 * n:].contiguous(), idx)[:, 0]
    assert torch.equal(_bits(P["sc"][0]), _bits(sp)) and torch.equal(_bits(P["sc"][1]), _bits(sn))
    want = torch.clamp_min((torch.tensor(MARGIN, dtype=torch.float32, device="cuda") - sp) + sn, 0.0)
    assert torch.equal(_bits(c["err"]), _bits(want))
    # arg: the first arg-max of the path's own fp32 c over the valid windows
    cc = P["c"].view(S, T, Fp)[:, :, :Fn].clone()
    valid = torch.zeros((S, T), dtype=torch.bool, device="cuda")
    valid[:, : T - k + 1] = (tok != 0)[:, k - 1:]
    cc[~valid] = float("-inf")
    mx = cc.max(dim=1).values  # [S, Fn]
    hit = (cc == mx.unsqueeze(1)) & valid.unsqueeze(2)
    first = torch.where(hit.any(1), hit.to(torch.int32).argmax(dim=1), torch.full_like(mx, -1, dtype=torch.int64))
    first = torch.where(P["y"] > 0, first, torch.full_like(first, -1))
    assert torch.equal(P["arg"].long(), first)
    assert (P["arg"] >= 0).any() and (P["arg"][:, :] < T - k + 1).all()
    # dc: exactly one non-zero per (s, f) with arg >= 0 (where dm != 0), zeros elsewhere
    dc = P["dc"].view(S, T, Fp)
    want_dc = torch.zeros_like(dc)
    s_i, f_i = (P["arg"] >= 0).nonzero(as_tuple=True)
    want_dc[s_i, P["arg"][s_i, f_i].long(), f_i] = P["dm"][s_i, f_i]
    assert torch.equal(dc, want_dc)
    assert (P["dm"][P["arg"] < 0] == 0).all()
    act = (c["err"] > 0).nonzero()[:, 0]
    act = torch.cat([act, n + act, 2 * n + act])
    assert ((dc[act] != 0).sum(1)[:, :Fn] == (P["arg"][act] >= 0)).all()


@gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_accuracy_against_fp64(name):
    c = _case(name)
    kk = _kinks(c["m64"], c["q"], c["ap"], c["an"], c["x"])
    print(f"shape {name}, seed {SEEDS[name]}: {kk}")
    assert _kinks_ok(kk), kk
    ref, got, lib = c["ref"], c["got"], c["lib"]
    assert got.shape == ref.shape == lib.shape and got.dtype == torch.float32
    with torch.no_grad():
        eq, ep, en = (c["plain"].encode(t) for t in (c["dq"], c["dp"], c["dn"]))
        lib_err = F.relu(MARGIN - gesd(eq, ep) + gesd(eq, en))
    _rule(f"{name} err", c["err"], lib_err, F.relu(c["x"]))
    _rule(f"{name} whole matrix", got, lib, ref)
    for nm, lo, hi in _blocks(c["ff"]):
        assert ref[:, lo:hi].abs().max() > 0
        _rule(f"{name} {nm}", got[:, lo:hi], lib[:, lo:hi], ref[:, lo:hi])


@gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_exact_structure(name):
    c = _case(name)
    V, D = DIMS[name][:2]
    got = c["got"].cpu()
    inactive = (c["x"] < 0).nonzero()[:, 0].tolist()
    assert inactive and (c["err"].cpu()[inactive] == 0).all()
    for i in inactive:
        assert (got[i] == 0).all()  # the alignment gaps included
    offE = c["ff"].offsets[0]
    emb = got[:, offE: offE + V * D].view(-1, V, D)
    assert (emb[:, 0] == 0).all()  # pad_idx
    for i in range(c["n"]):
        words = set(c["q"][i].tolist()) | set(c["ap"][i].tolist()) | set(c["an"][i].tolist())
        out = [v for v in range(V) if v not in words]
        assert (emb[i, out] == 0).all()
        if i not in inactive:
            assert (emb[i, sorted(words - {0})].abs().sum(1) > 0).any()
    # the alignment gaps of every row
    mask = torch.ones(c["ff"].numel, dtype=torch.bool)
    for _, lo, hi in _blocks(c["ff"]):
        mask[lo:hi] = False
    assert (got[:, mask] == 0).all()


@gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_invariance(name):
    c = _case(name)
    m, ff, n = c["fused"], c["ff"], c["n"]
    dq, dp, dn = c["dq"], c["dp"], c["dn"]
    full, err = c["got"], c["err"]
    for i in range(n):  # alone
        g1, e1 = seq.per_example_grads(m, ff, dq[i: i + 1], dp[i: i + 1], dn[i: i + 1], MARGIN)
        assert torch.equal(g1[0], full[i]) and torch.equal(e1[0], err[i]), i
    gp, ep = seq.per_example_grads(m, ff, F.pad(dq, (0, 3)), F.pad(dp, (0, 3)), F.pad(dn, (0, 3)), MARGIN)
    assert torch.equal(gp, full) and torch.equal(ep, err)  # 3 more pad columns
    perm = torch.tensor([(3 * i + 1) % n for i in range(n)] if n == 5 else [2, 0, 1], device="cuda")
    gr, er = seq.per_example_grads(m, ff, dq[perm], dp[perm], dn[perm], MARGIN)
    assert torch.equal(gr, full[perm]) and torch.equal(er, err[perm])


@gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_guards_and_pad_columns(name):
    c = _case(name)
    V, D, H, Fn, k = DIMS[name]
    buf, out = _guarded((c["n"], c["ff"].numel))
    parts = {}
    g, err = seq.per_example_grads(c["fused"], c["ff"], c["dq"], c["dp"], c["dn"], MARGIN, out=out, parts=parts)
    torch.cuda.synchronize()
    assert g is out
    _guards_ok(buf, out)
    assert torch.equal(g, c["got"]) and torch.equal(err, c["err"])
    Fp, Kp = seq.packed_shape(Fn, H, k)
    assert parts["dc"].shape[1] == Fp and parts["dwin"].shape[1] == seq.round_up(Kp, 64)
    assert (_bits(parts["dc"][:, Fn:]) == 0).all()
    assert (parts["dwin"][:, k * H:] == 0).all()
    assert (parts["dwin"][:, : k * H] != 0).any()
    if name == "A":
        assert Fp > Fn and Kp > k * H and parts["dwin"].shape[1] > Kp


@gpu
def test_sees_weights_written_behind_torch():
    V, D, H, Fn, k = DIMS["A"]
    torch.manual_seed(7)
    m = BiCNN(V, D, H, Fn, k, fused_grad=True).cuda().eval()
    fm = FlatParams(m)
    q, ap, an = (t.cuda() for t in _tokens("A", 7))
    first, _ = seq.per_example_grads(m, fm, q, ap, an, 0.3)
    v = m.conv.weight._version
    m.conv.weight.data.mul_(2)
    assert m.conv.weight._version == v
    second, e2 = seq.per_example_grads(m, fm, q, ap, an, 0.3)
    fresh = BiCNN(V, D, H, Fn, k, fused_grad=True).cuda().eval()
    fresh.load_state_dict(m.state_dict())
    want, ew = seq.per_example_grads(fresh, FlatParams(fresh), q, ap, an, 0.3)
    assert torch.equal(_bits(second), _bits(want)) and torch.equal(_bits(e2), _bits(ew))
    assert not torch.equal(second, first)


def _seq_parity_loop(m64, offsets, numel, q, ap, an, margin, l1, l2, clip):
    """The reference's rule, literally, in fp64: per example G += g; G += l1 sign(p) + l2 p; clamp."""
    g, x = _reference(m64, offsets, numel, q, ap, an, margin)
    p = torch.zeros(numel, dtype=torch.float64)
    params = [m64.embed.weight, m64.hidden.weight, m64.hidden.bias, m64.conv.weight, m64.conv.bias]
    for t, off in zip(params, offsets):
        p[off: off + t.numel()] = t.detach().reshape(-1)
    G = torch.zeros(numel, dtype=torch.float64)
    for i in range(q.shape[0]):
        G += g[i]
        G += l1 * torch.sign(p) + l2 * p
        G.clamp_(-clip, clip)
    loss = F.relu(x).sum() + q.shape[0] * (l1 * p.abs().sum() + 0.5 * l2 * (p * p).sum())
    return G, loss


@gpu
def test_parity_grad_end_to_end():
    c = _case("A")
    l1, l2, clip = 0.0, 1e-4, 0.5
    n0 = seq.COUNTERS["pegrad_fused"]
    res = []
    for chunk in (2, 4):
        loss = parity_grad_(c["fused"], c["ff"], c["dq"], c["dp"], c["dn"], MARGIN, l1, l2, clip, chunk=chunk)
        res.append((c["ff"].grad[: c["ff"].numel].clone(), loss.clone()))
    assert seq.COUNTERS["pegrad_fused"] == n0 + 3 + 2  # ceil(5 / 2) + ceil(5 / 4) calls
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    f0 = seq.COUNTERS["pegrad_fallback"]
    lib_loss = parity_grad_(c["plain"], c["fp"], c["dq"], c["dp"], c["dn"], MARGIN, l1, l2, clip, chunk=4)
    assert seq.COUNTERS["pegrad_fallback"] == f0 and seq.COUNTERS["pegrad_fused"] == n0 + 5
    lib_G = c["fp"].grad[: c["fp"].numel]
    G, loss = _seq_parity_loop(c["m64"], c["ff"].offsets, c["ff"].numel, c["q"], c["ap"], c["an"], MARGIN, l1, l2, clip)
    assert (G.abs() < clip).all()  # away from the clamp's kink
    _rule("parity_grad_ G", res[0][0], lib_G, G)
    _rule("parity_grad_ loss", res[0][1], lib_loss, loss)
