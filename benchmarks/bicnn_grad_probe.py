"""Fused vs PyTorch per-example gradients of the BiCNN parity rule (ops/seq.py per_example_grads
against models/bicnn.py per_example_grads, torch.func.vmap) at the reference's dimensions
(vocabulary 22354, embedding 100, hidden 200, 3000 filters, k = 2).

    python benchmarks/bicnn_grad_probe.py [--out table.md] [--iters 5] [--rounds 5] [--only fused|pytorch]

Cases: ``per_example_grads`` of n = 16 examples with T = 16, 40 and 200 (sentence lengths uniform
in [2, T]), and a whole ``parity_grad_`` of 64 examples (T = 40, chunk 16, l2 1e-4, clip 0.5: the
application's defaults). Each case times ``iters`` back-to-back calls between two device events
(issued eagerly, as the worker issues them), the two paths alternating for ``rounds`` rounds in one
process; the table gives the median and the minimum per call in milliseconds. Both paths run on
the same weights and tokens, and the outputs are compared first. ``--only`` runs one path alone
(for a kernel trace)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mpit_amd.models import bicnn as M
from mpit_amd.models.bicnn import BiCNN, parity_grad_
from mpit_amd.ops import seq
from mpit_amd.utils.flat import FlatParams


def time_call(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters  # ms per call


def ab(fns, iters, rounds):
    for fn in fns.values():  # warm-up: code objects, library algorithm choices
        for _ in range(2):
            fn()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(time_call(fn, iters))
    return {k: (statistics.median(v), min(v)) for k, v in times.items()}


def tokens(n, T, V, seed, dev):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(3):
        tok = torch.randint(1, V, (n, T), generator=g)
        for i, m in enumerate(torch.randint(2, T + 1, (n,), generator=g).tolist()):
            tok[i, m:] = 0
        out.append(tok.to(dev))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["fused", "pytorch"], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bicnn_grad_probe: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda")
    torch.manual_seed(1)
    V, margin = 22354, 0.009
    plain = BiCNN(V, 100, 200, 3000, 2, fused=False, fused_grad=False).to(dev).eval()
    fused = BiCNN(V, 100, 200, 3000, 2, fused=False, fused_grad=True).to(dev).eval()
    fused.load_state_dict(plain.state_dict())
    fp, ff = FlatParams(plain), FlatParams(fused)
    assert fused.fused_grad_ok(torch.zeros(1, 2, dtype=torch.int64, device=dev))
    rows = []

    def case(name, fns, compare):
        diff = compare()
        if a.only:
            fns = {a.only: fns[a.only]}
        r = ab(fns, a.iters, a.rounds)
        rows.append((name, r, diff))
        print(name, r, f"rel. difference {diff:.2e}", flush=True)

    for T in (16, 40, 200):
        q, p, ng = tokens(16, T, V, T, dev)

        def compare():
            g1, err = seq.per_example_grads(fused, ff, q, p, ng, margin)
            g0 = M.per_example_grads(plain, fp, q, p, ng, margin)
            assert int((err > 0).sum()) > 0
            return ((g1 - g0).norm() / g0.norm()).item()

        case(f"per_example_grads 16 x T={T}",
             {"fused": lambda: seq.per_example_grads(fused, ff, q, p, ng, margin),
              "pytorch": lambda: M.per_example_grads(plain, fp, q, p, ng, margin)}, compare)
    q, p, ng = tokens(64, 40, V, 7, dev)

    def compare():
        n0 = seq.COUNTERS["pegrad_fused"]
        l1 = parity_grad_(fused, ff, q, p, ng, margin, 0.0, 1e-4, 0.5)
        assert seq.COUNTERS["pegrad_fused"] == n0 + 4
        l0 = parity_grad_(plain, fp, q, p, ng, margin, 0.0, 1e-4, 0.5)
        print(f"parity_grad_ loss: fused {float(l1):.6f}, PyTorch {float(l0):.6f}", flush=True)
        return ((ff.grad - fp.grad).norm() / fp.grad.norm()).item()

    case("parity_grad_ 64 x T=40",
         {"fused": lambda: parity_grad_(fused, ff, q, p, ng, margin, 0.0, 1e-4, 0.5),
          "pytorch": lambda: parity_grad_(plain, fp, q, p, ng, margin, 0.0, 1e-4, 0.5)}, compare)
    lines = [f"Device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}; "
             f"{a.iters} calls per timing, {a.rounds} alternating rounds, device events, ms per call.", ""]
    if a.only:
        lines += [f"| case | {a.only} median | {a.only} min |", "|---|---|---|"]
        lines += [f"| {name} | {r[a.only][0]:.3f} | {r[a.only][1]:.3f} |" for name, r, _ in rows]
    else:
        lines += ["| case | fused median | fused min | PyTorch median | PyTorch min | PyTorch / fused (median) | "
                  "rel. difference of the outputs |", "|---|---|---|---|---|---|---|"]
        for name, r, diff in rows:
            (fm, fn_), (pm, pn) = r["fused"], r["pytorch"]
            lines.append(f"| {name} | {fm:.3f} | {fn_:.3f} | {pm:.3f} | {pn:.3f} | {pm / fm:.2f}x | {diff:.2e} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
