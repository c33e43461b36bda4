"""The opt-in forward-only BiCNN encoder and GESD scorer (csrc/kernels/seq.hip, ops/seq.py,
``BiCNN(fused=True)``, apps/bicnn.py -fusedEncoder).

Accuracy rule (the project's, tests/test_fp32_path.py): the relative error ``|a - ref| / |ref|``
against an fp64 reference of the same math on the CPU is at most ``2 * e_torch + 1e-9``, e_torch
being the error of PyTorch's fp32 ops on the same GPU for the same inputs.

Guards: the kernels write dense row-major outputs (their interface has no output row stride), so
every output is carved out of a larger sentinel-filled buffer with guard rows before and after it;
a write past a row's last column lands in the next row (caught by the value checks, which cover
every element) or, for the last row, in the guard. The pad COLUMNS that do exist (the windows'
``k*H..Kp-1``, the GEMM output's ``F..ldc-1``) are checked / poisoned explicitly."""
import copy
import random

import pytest
import torch
import torch.nn.functional as F

from mpit_amd.apps import bicnn as app
from mpit_amd.apps.qa_data import pad_batch, synthetic_qa
from mpit_amd.models.bicnn import BiCNN, draw_negatives, first_violations, gesd
from mpit_amd.ops import seq

gpu = pytest.mark.gpu
SENT = -12345.0
GUARD = 512


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


def _lengths_tok(lengths, T, vocab, gen):
    tok = torch.zeros((len(lengths), T), dtype=torch.int64)
    for i, n in enumerate(lengths):
        tok[i, :n] = torch.randint(1, vocab, (n,), generator=gen)
    return tok


# ------------------------------------------------------------------------------ CPU tier

@pytest.mark.parametrize("Fn,H,k", [(3000, 200, 2), (72, 24, 3)])
def test_pack_conv_weight_cpu(Fn, H, k):
    torch.manual_seed(Fn)
    w = torch.randn(Fn, H, k)
    Fp, Kp = seq.packed_shape(Fn, H, k)
    assert Fp % 64 == 0 and Fn <= Fp < Fn + 64 and Kp % 16 == 0 and k * H <= Kp < k * H + 16
    want = torch.zeros(Fp, Kp)
    for f in range(Fn):
        for j in range(k):
            want[f, j * H: (j + 1) * H] = w[f, :, j]
    got = seq.pack_conv_weight(w)
    assert got.shape == (Fp, Kp) and got.is_contiguous() and torch.equal(got, want)
    # the refill of a persistent buffer: new values in, the zero pad untouched
    again = seq.pack_conv_weight(w * 2, got)
    assert again is got and torch.equal(got, want * 2)


def _cpu_pair(seed=0):
    torch.manual_seed(seed)
    d = synthetic_qa(n_answers=40, n_train=24, emb_dim=8)
    plain = BiCNN(len(d.word2idx), 8, 12, 20, 2, fused=False).eval()
    fused = BiCNN(len(d.word2idx), 8, 12, 20, 2, fused=True).eval()
    fused.load_state_dict(plain.state_dict())
    return d, plain, fused


def test_fused_model_on_cpu_is_the_pytorch_path():
    d, plain, fused = _cpu_pair()
    assert fused.fused and not plain.fused
    batch = d.train[:24]
    q = pad_batch([b[1] for b in batch])
    a = pad_batch([b[2] for b in batch])
    rng = random.Random(3)
    labs = sorted(d.answers)
    draws = [draw_negatives(rng, len(labs), labels, 30) for labels, _, _ in batch]
    before = dict(seq.COUNTERS)
    with torch.no_grad():
        out = []
        for m in (plain, fused):
            eq, ea = m.encode(q), m.encode(a)
            idx = torch.randint(0, ea.shape[0], (eq.shape[0], 5), generator=torch.Generator().manual_seed(1))
            sc = m.score(eq, ea, idx)
            sp = gesd(eq, ea)
            fv = first_violations(m, eq, sp, draws, d.answers, 0.02, pad_batch, chunk=2)
            out.append((eq, ea, sc, fv))
    (eq0, ea0, sc0, fv0), (eq1, ea1, sc1, fv1) = out
    assert torch.equal(_bits(eq0), _bits(eq1)) and torch.equal(_bits(ea0), _bits(ea1))
    assert torch.equal(_bits(sc0), _bits(sc1)) and fv0 == fv1
    assert torch.equal(sc0, gesd(eq0.unsqueeze(1).expand(-1, 5, -1), ea0[idx]))
    assert seq.COUNTERS["encode_fused"] == before["encode_fused"]
    assert seq.COUNTERS["gesd_fused"] == before["gesd_fused"]
    assert seq.COUNTERS["encode_fallback"] > before["encode_fallback"]
    assert seq.COUNTERS["gesd_fallback"] > before["gesd_fallback"]


def test_fused_encoder_flag_and_default(monkeypatch):
    monkeypatch.delenv("MPIT_BICNN_FUSED", raising=False)
    assert app.build_args(["-fusedEncoder"]).fusedEncoder is True
    assert not app.build_args([]).fusedEncoder
    assert BiCNN(30, 8, 12, 20, 2).fused is False
    assert BiCNN(30, 8, 12, 20, 2, fused=app.build_args([]).fusedEncoder).fused is False
    assert BiCNN(30, 8, 12, 20, 2, fused=app.build_args(["-fusedEncoder"]).fusedEncoder).fused is True
    monkeypatch.setenv("MPIT_BICNN_FUSED", "1")
    assert BiCNN(30, 8, 12, 20, 2).fused is True and BiCNN(30, 8, 12, 20, 2, fused=False).fused is False


# ------------------------------------------------------------------------------ GPU tier

@gpu
@pytest.mark.parametrize("B,T,D,H,k,V", [(3, 7, 100, 200, 2, 50), (2, 5, 12, 24, 3, 20)])
def test_hidden_windows(B, T, D, H, k, V):
    g = torch.Generator().manual_seed(B * T + H)
    tok = torch.randint(0, V, (B, T), generator=g)
    E = torch.randn(V, D, generator=g)
    Wh = torch.randn(H, D, generator=g) / D ** 0.5
    bh = torch.randn(H, generator=g) * 0.1
    Kp = seq.round_up(k * H, 16) + (16 if (k * H) % 16 == 0 else 0)  # always some pad columns
    buf, out = _guarded((B * T, Kp))
    got = seq.hidden_windows(tok.cuda(), E.cuda(), Wh.cuda(), bh.cuda(), k, Kp, out=out)
    torch.cuda.synchronize()
    assert got is out
    _guards_ok(buf, out)
    o = out.cpu().view(B, T, Kp)
    assert (_bits(o[:, :, k * H:]) == 0).all()  # pad columns: +0.0
    for j in range(k):
        tap = o[:, :, j * H: (j + 1) * H]
        assert (_bits(tap[:, max(0, T - j):]) == 0).all()  # missing taps: +0.0
        if j and T > j:  # tap j of row (b, t) is tap 0 of row (b, t + j), bit for bit
            assert torch.equal(_bits(tap[:, : T - j]), _bits(o[:, j:, :H]))
    ref = torch.tanh(F.linear(F.embedding(tok, E.double()), Wh.double(), bh.double()))
    lib = torch.tanh(F.linear(F.embedding(tok.cuda(), E.cuda()), Wh.cuda(), bh.cuda()))
    _rule("hidden_windows", o[:, :, :H], lib, ref)
    # without a bias
    got0 = seq.hidden_windows(tok.cuda(), E.cuda(), Wh.cuda(), None, k).view(B, T, -1)[:, :, :H]
    ref0 = torch.tanh(F.linear(F.embedding(tok, E.double()), Wh.double()))
    lib0 = torch.tanh(F.linear(F.embedding(tok.cuda(), E.cuda()), Wh.cuda()))
    _rule("hidden_windows (no bias)", got0, lib0, ref0)


def _max_norm_case(Fn, ldc, k, exact, seed):
    """B = 5 sentences of T = 33 (165 rows: sentence 3 crosses row 128) of lengths 0, k-1, k, T
    and 20; pad columns and invalid rows of c hold 1e30. exact: small-integer c and bias (m and
    sum m^2 exact in fp32), every valid value + bias of the last sentence negative."""
    g = torch.Generator().manual_seed(seed)
    B, T = 5, 33
    lengths = [0, k - 1, k, T, 20]
    tok = _lengths_tok(lengths, T, 50, g)
    if exact:
        c = torch.randint(-8, 9, (B, T, ldc), generator=g).float()
        bias = torch.randint(-3, 4, (Fn,), generator=g).float()
        c[4] = torch.randint(-8, -3, (T, ldc), generator=g).float()  # + bias <= -1
    else:
        c = torch.randn(B, T, ldc, generator=g)
        bias = torch.randn(Fn, generator=g) * 0.5
    c[:, :, Fn:] = 1e30
    for b, n in enumerate(lengths):
        c[b, max(0, n - k + 1):] = 1e30  # windows t with t + k - 1 >= n
    return tok, c.view(B * T, ldc).contiguous(), bias, lengths


def _max_norm_ref(tok, c, bias, Fn, k, dt):
    """The PyTorch chain of BiCNN.encode after the convolution, on c's F real columns."""
    B, T = tok.shape
    cw = c.view(B, T, -1)[:, : T - k + 1, :Fn].to(dt).transpose(1, 2) + bias.to(dt)[None, :, None]
    vw = (tok != 0)[:, k - 1:].unsqueeze(1)
    m = torch.nan_to_num(cw.masked_fill(~vw, float("-inf")).max(dim=-1).values, neginf=0.0)
    m = F.relu(m)
    return m / m.norm(p=2, dim=-1, keepdim=True).clamp_min(1e-10)


@gpu
@pytest.mark.parametrize("Fn,ldc,k", [(3000, 3008, 2), (72, 128, 3)])
def test_max_norm_exact(Fn, ldc, k):
    tok, c, bias, lengths = _max_norm_case(Fn, ldc, k, True, Fn)
    buf, out = _guarded((5, Fn))
    seq.max_norm(c.cuda(), tok.cuda(), k, 0, bias.cuda(), Fn, 1e-10, out=out)
    torch.cuda.synchronize()
    _guards_ok(buf, out)
    o = out.cpu()
    ref = _max_norm_ref(tok, c, bias, Fn, k, torch.float64)
    assert (ref[3] > 0).any() and (ref[2] > 0).any()
    r32 = ref.float().abs()
    ulp = (torch.nextafter(r32, torch.full_like(r32, float("inf"))) - r32).double()
    err = (o.double() - ref).abs() / ulp
    print(f"max_norm exact F={Fn}: worst error {err.max().item():.3f} ulp")
    assert (err <= 4.0).all()
    for b in (0, 1, 4):  # all padding, k-1 tokens, every value + bias negative: +0.0, never NaN
        assert (_bits(o[b]) == 0).all()


@gpu
@pytest.mark.parametrize("Fn,ldc,k", [(3000, 3008, 2), (72, 128, 3)])
def test_max_norm_random(Fn, ldc, k):
    tok, c, bias, _ = _max_norm_case(Fn, ldc, k, False, Fn + 1)
    buf, out = _guarded((5, Fn))
    seq.max_norm(c.cuda(), tok.cuda(), k, 0, bias.cuda(), Fn, 1e-10, out=out)
    torch.cuda.synchronize()
    _guards_ok(buf, out)
    ref = _max_norm_ref(tok, c, bias, Fn, k, torch.float64)
    lib = _max_norm_ref(tok.cuda(), c.cuda(), bias.cuda(), Fn, k, torch.float32)
    _rule("max_norm", out, lib, ref)
    assert (_bits(out[:2].cpu()) == 0).all()
    # no bias: the bias pointer is optional
    got0 = seq.max_norm(c.cuda(), tok.cuda(), k, 0, None, Fn)
    _rule("max_norm (no bias)", got0, _max_norm_ref(tok.cuda(), c.cuda(), torch.zeros(Fn).cuda(), Fn, k, torch.float32),
          _max_norm_ref(tok, c, torch.zeros(Fn), Fn, k, torch.float64))


_MODELS = {}


def _model(dims):
    """(fused model on the GPU, its PyTorch twin on the GPU, its fp64 copy on the CPU), shared and
    never modified by the tests that take it. The pad row of the embedding is 1e3."""
    if dims not in _MODELS:
        V, D, H, Fn, k = dims
        torch.manual_seed(sum(dims))
        plain = BiCNN(V, D, H, Fn, k, fused=False).eval()
        with torch.no_grad():
            plain.embed.weight[0] = 1e3
        fused = BiCNN(V, D, H, Fn, k, fused=True).eval()
        fused.load_state_dict(plain.state_dict())
        _MODELS[dims] = (fused.cuda(), copy.deepcopy(plain).cuda(), copy.deepcopy(plain).double())
    return _MODELS[dims]


REF_DIMS = (50, 100, 200, 3000, 2)
SMALL_DIMS = (20, 12, 24, 72, 3)


def _mixed_tok(dims, seed=5):
    k = dims[4]
    return _lengths_tok([14, 9, k, k - 1, 5, 14], 14, dims[0], torch.Generator().manual_seed(seed))


@gpu
@pytest.mark.parametrize("dims", [REF_DIMS, SMALL_DIMS])
def test_encode_end_to_end(dims):
    fused, plain, m64 = _model(dims)
    tok = _mixed_tok(dims)
    n0 = seq.COUNTERS["encode_fused"]
    with torch.no_grad():
        got = fused.encode(tok.cuda())
        assert seq.COUNTERS["encode_fused"] == n0 + 1
        lib = plain.encode(tok.cuda())
        ref = m64.encode(tok)
    assert got.shape == (6, dims[3]) and got.dtype == torch.float32
    assert (_bits(got[3].cpu()) == 0).all()  # k - 1 tokens: no window
    _rule("encode", got, lib, ref)
    # under autograd the fused model runs the PyTorch path
    nf = seq.COUNTERS["encode_fallback"]
    out = fused.encode(tok.cuda())
    assert out.requires_grad and seq.COUNTERS["encode_fused"] == n0 + 1 and seq.COUNTERS["encode_fallback"] == nf + 1


@gpu
@pytest.mark.parametrize("dims", [REF_DIMS, SMALL_DIMS])
def test_encode_batch_invariance(dims):
    fused, _, _ = _model(dims)
    k = dims[4]
    tok = _mixed_tok(dims).cuda()
    with torch.no_grad():
        full = fused.encode(tok)
        for i in range(tok.shape[0]):
            n = int((tok[i] != 0).sum())
            alone = fused.encode(tok[i: i + 1])
            short = fused.encode(tok[i: i + 1, : max(n, k)].contiguous())
            longer = fused.encode(F.pad(tok[i: i + 1], (0, 9)))
            for name, x in (("alone", alone), ("trimmed", short), ("padded", longer)):
                assert torch.equal(_bits(x[0]), _bits(full[i])), (i, name)


@gpu
def test_encode_sees_weights_written_behind_torch():
    V, D, H, Fn, k = SMALL_DIMS
    torch.manual_seed(7)
    m = BiCNN(V, D, H, Fn, k, fused=True).cuda().eval()
    tok = _mixed_tok(SMALL_DIMS).cuda()
    with torch.no_grad():
        first = m.encode(tok)
        v = m.conv.weight._version
        m.conv.weight.data.mul_(2)
        assert m.conv.weight._version == v
        second = m.encode(tok)
        fresh = BiCNN(V, D, H, Fn, k, fused=True).cuda().eval()
        fresh.load_state_dict(m.state_dict())
        want = fresh.encode(tok)
    assert torch.equal(_bits(second), _bits(want))
    assert not torch.equal(_bits(second), _bits(first))


@gpu
@pytest.mark.parametrize("n,w,m,D", [(3, 5, 7, 3000), (2, 4, 3, 37)])
def test_gesd_gather(n, w, m, D):
    g = torch.Generator().manual_seed(n * w + D)
    q = F.normalize(F.relu(torch.randn(n, D, generator=g)), dim=-1)
    cand = F.normalize(F.relu(torch.randn(m, D, generator=g)), dim=-1)
    idx = torch.randint(0, m, (n, w), generator=g)
    idx[0, 0] = idx[0, 1] = 1  # a repeated index
    cand[2] = q[1]
    idx[1, 2] = 2  # one pair of identical vectors
    buf, out = _guarded((n, w))
    qd, cd, idd = q.cuda(), cand.cuda(), idx.cuda()
    seq.gesd_gather(qd, cd, idd, out=out)
    torch.cuda.synchronize()
    _guards_ok(buf, out)
    ref = gesd(q.double().unsqueeze(1).expand(-1, w, -1), cand.double()[idx])
    lib = gesd(qd.unsqueeze(1).expand(-1, w, -1), cd[idd])
    _rule("gesd_gather", out, lib, ref)
    assert torch.equal(_bits(out[0, 0:1]), _bits(out[0, 1:2]))
    # independent of n and w, bit for bit: one row alone, one pair alone
    for r in range(n):
        row = seq.gesd_gather(qd[r: r + 1], cd, idd[r: r + 1])
        assert torch.equal(_bits(row[0]), _bits(out[r]))
        one = seq.gesd_gather(qd[r: r + 1], cd, idd[r: r + 1, w - 1:].contiguous())
        assert torch.equal(_bits(one[0]), _bits(out[r, w - 1:]))


def _sequential_first_violation(model, q_tok, a_tok, draws, answers, margin, dev):
    """The reference's scan (BiCNN/bicnn.lua:321-359): one encode and one score per draw."""
    z = torch.zeros((1, 1), dtype=torch.int64, device=dev)
    eq = model.encode(q_tok.unsqueeze(0))
    sp = model.score(eq, model.encode(a_tok.unsqueeze(0)), z)[0, 0]
    for x in draws:
        sn = model.score(eq, model.encode(pad_batch([answers[x]]).to(dev)), z)[0, 0]
        if sp - sn < margin:
            return x
    return None


@gpu
@pytest.mark.parametrize("margin", [0.0, 0.02, 0.3])
def test_first_violations_fused_is_the_sequential_scan(margin):
    torch.manual_seed(0)
    d = synthetic_qa(n_answers=40, n_train=24, emb_dim=8)
    dev = torch.device("cuda")
    m = BiCNN(len(d.word2idx), 8, 12, 20, 2, fused=True).to(dev).eval()
    batch = d.train[:24]
    q = pad_batch([b[1] for b in batch]).to(dev)
    a = pad_batch([b[2] for b in batch]).to(dev)
    rng = random.Random(3)
    labs = sorted(d.answers)
    draws = [draw_negatives(rng, len(labs), labels, 30) for labels, _, _ in batch]
    n0, g0 = seq.COUNTERS["encode_fused"], seq.COUNTERS["gesd_fused"]
    with torch.no_grad():
        eq = m.encode(q)
        sp = m.score(eq, m.encode(a), torch.arange(len(batch), device=dev).unsqueeze(1))[:, 0]
        got = first_violations(m, eq, sp, draws, d.answers, margin, pad_batch, chunk=2)
        assert seq.COUNTERS["encode_fused"] > n0 + 2 and seq.COUNTERS["gesd_fused"] > g0 + 1
        want = [_sequential_first_violation(m, q[i][q[i] != 0], a[i][a[i] != 0], draws[i], d.answers, margin, dev)
                for i in range(len(batch))]
    assert got == want
    if margin == 0.3:
        assert all(x is not None for x in got)


@gpu
def test_evaluate_fused_matches_pytorch():
    d = synthetic_qa(n_answers=60, n_train=10, n_valid=40, vocab=300, pool=10, n_tests=0)
    torch.manual_seed(1)
    plain = BiCNN(len(d.word2idx), 100, 200, 3000, 2, 1, fused=False)
    with torch.no_grad():
        plain.embed.weight.copy_(d.embedding_matrix())
    fused = BiCNN(len(d.word2idx), 100, 200, 3000, 2, 1, fused=True)
    fused.load_state_dict(plain.state_dict())
    m64 = copy.deepcopy(plain).double().eval()
    # fp64 top-2 similarity gap of every question
    labs = sorted(d.answers)
    pos = {x: i for i, x in enumerate(labs)}
    keep = []
    with torch.no_grad():
        emb = m64.encode(pad_batch([d.answers[x] for x in labs]))
        eq = m64.encode(pad_batch([qq for _, qq, _ in d.valid]))
        for item, e in zip(d.valid, eq):
            cand = torch.tensor([pos[p] for p in item[2]])
            top = gesd(e.unsqueeze(0).expand(len(cand), -1), emb[cand]).topk(2).values
            if float(top[0] - top[1]) >= 1e-5:
                keep.append(item)
    excluded = len(d.valid) - len(keep)
    print(f"evaluate: {excluded} of {len(d.valid)} questions excluded (fp64 top-2 gap < 1e-5)")
    assert excluded <= 0.1 * len(d.valid)
    dev = torch.device("cuda")
    n0, g0 = seq.COUNTERS["encode_fused"], seq.COUNTERS["gesd_fused"]
    acc_f = app.evaluate(fused.to(dev), d, keep, dev)
    assert seq.COUNTERS["encode_fused"] >= n0 + 2 and seq.COUNTERS["gesd_fused"] == g0 + len(keep)
    acc_p = app.evaluate(plain.to(dev), d, keep, dev)
    acc_64 = app.evaluate(m64, d, keep, torch.device("cpu"))
    print(f"evaluate: fused {acc_f:.4f}, PyTorch {acc_p:.4f}, fp64 {acc_64:.4f}")
    assert acc_f == acc_p == acc_64
