"""Fused vs PyTorch forward-only BiCNN encode and GESD scoring (ops/seq.py) at the reference's
dimensions (embedding 100, hidden 200, 3000 filters, k = 2).

    python benchmarks/bicnn_encode_probe.py [--out table.md] [--iters 50] [--rounds 7]

Cases: ``encode`` of 256 sentences of T = 16 and of T = 40, ``score`` of a 256 x 64 index matrix
against 256 candidate rows. Each case times ``iters`` back-to-back calls between two device
events (the calls are issued eagerly, as the negative-sampling scan and the tester issue them, so
the figure includes what the host cannot hide), the two paths alternating for ``rounds`` rounds
in one process; the table gives the median and the minimum per call. Both paths run under
``torch.no_grad()`` on the same weights and tokens, and the outputs are compared first."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mpit_amd.models.bicnn import BiCNN
from mpit_amd.ops import seq


def time_call(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters  # us per call


def ab(fns, iters, rounds):
    for fn in fns.values():  # warm-up: code objects, library algorithm choices
        for _ in range(5):
            fn()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(time_call(fn, iters))
    return {k: (statistics.median(v), min(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bicnn_encode_probe: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda")
    torch.manual_seed(1)
    V = 22354
    plain = BiCNN(V, 100, 200, 3000, 2, fused=False).to(dev).eval()
    fused = BiCNN(V, 100, 200, 3000, 2, fused=True).to(dev).eval()
    fused.load_state_dict(plain.state_dict())
    rows = []
    with torch.no_grad():
        for T in (16, 40):
            g = torch.Generator().manual_seed(T)
            tok = torch.randint(1, V, (256, T), generator=g)
            for i, n in enumerate(torch.randint(2, T + 1, (256,), generator=g).tolist()):
                tok[i, n:] = 0
            tok = tok.to(dev)
            n0 = seq.COUNTERS["encode_fused"]
            a_, b_ = fused.encode(tok), plain.encode(tok)
            assert seq.COUNTERS["encode_fused"] == n0 + 1
            diff = ((a_ - b_).norm() / b_.norm()).item()
            r = ab({"fused": lambda: fused.encode(tok), "pytorch": lambda: plain.encode(tok)}, a.iters, a.rounds)
            rows.append((f"encode 256 x T={T}", r, diff))
        g = torch.Generator().manual_seed(3)
        eq = torch.nn.functional.normalize(torch.rand(256, 3000, generator=g), dim=-1).to(dev)
        emb = torch.nn.functional.normalize(torch.rand(256, 3000, generator=g), dim=-1).to(dev)
        idx = torch.randint(0, 256, (256, 64), generator=g).to(dev)
        a_, b_ = fused.score(eq, emb, idx), plain.score(eq, emb, idx)
        diff = ((a_ - b_).norm() / b_.norm()).item()
        r = ab({"fused": lambda: fused.score(eq, emb, idx), "pytorch": lambda: plain.score(eq, emb, idx)},
               a.iters, a.rounds)
        rows.append(("score 256 x 64", r, diff))
    lines = [f"Device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}; "
             f"{a.iters} calls per timing, {a.rounds} alternating rounds, device events, us per call.", "",
             "| case | fused median | fused min | PyTorch median | PyTorch min | PyTorch / fused (median) | "
             "rel. difference of the outputs |", "|---|---|---|---|---|---|---|"]
    for name, r, diff in rows:
        (fm, fn_), (pm, pn) = r["fused"], r["pytorch"]
        lines.append(f"| {name} | {fm:.1f} | {fn_:.1f} | {pm:.1f} | {pn:.1f} | {pm / fm:.2f}x | {diff:.2e} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
