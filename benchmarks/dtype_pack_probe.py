"""Derived-datatype pack / unpack / Put on HBM: the type_copy kernel against the byte-index path
and against torch's strided copy.

    python benchmarks/dtype_pack_probe.py [--out profiles/dtype_pack.md] [--rounds 7] [--budget-ms 200]

Shapes: 1 MiB as 16,384 x 64 B at stride 128 B; a halo column, 8,192 x 16 B at stride 16 KiB;
64 MiB as 4 KiB runs at stride 8 KiB; a 12-of-16-byte struct x 1 M. Arms, per shape and direction:

* ``kernel``  Datatype.pack / unpack on the default path (one type_copy launch);
* ``index``   the same calls under MPIT_DTYPE_KERNEL=0: the byte-index gather / scatter, which is
              the code this path had before the kernel, unchanged. Its index tensor is put into the
              type's cache beforehand (built with torch arithmetic; building it in Python, as the
              first call of that path does, takes minutes at 64 MiB), so the arm is its steady state;
* ``torch``   ``view.contiguous()`` / ``view.copy_()`` on the equivalent strided view: the copy-rate
              yardstick (for the struct, a view of the same volume: 12 of every 16 bytes).

Each arm is timed as a batch of back-to-back calls between two device events (the batch sized to
about --budget-ms), the arms alternating for --rounds rounds in one process after a warm-up of
every arm; the table gives the median and the minimum per call and the payload rate at the median.
Outputs are compared bitwise before anything is timed. Then: Put of the first two shapes into a
device window with a derived target type, one launch against one peer copy per run (the fallback
path), and the host-side cost of the 262,144-entry vector: constructing it, building its plan,
and the first pack on each path."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mpit_amd import datatypes as dt


class index_path:
    """MPIT_DTYPE_KERNEL=0 for the calls inside (the switch is read per call)."""

    def __enter__(self):
        self.old = os.environ.get("MPIT_DTYPE_KERNEL")
        os.environ["MPIT_DTYPE_KERNEL"] = "0"

    def __exit__(self, *a):
        if self.old is None:
            del os.environ["MPIT_DTYPE_KERNEL"]
        else:
            os.environ["MPIT_DTYPE_KERNEL"] = self.old


def plan_index(plan, device):
    """The byte index of a plan's packed stream, in torch arithmetic (what _byte_index builds in
    a Python loop)."""
    base = torch.zeros(1, dtype=torch.int64, device=device)
    for n, s in plan.loops:
        base = (base[:, None] + torch.arange(n, device=device, dtype=torch.int64)[None, :] * s).reshape(-1)
    run = torch.cat([torch.arange(int(o), int(o + ln), device=device, dtype=torch.int64)
                     for o, ln in zip(plan.offs, plan.lens)])
    return (base[:, None] + run[None, :]).reshape(-1)


def time_batch(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters  # us per call


def ab(fns, rounds, budget_ms):
    iters = {}
    for k, fn in fns.items():  # warm-up, and the batch size from a first estimate
        for _ in range(3):
            fn()
        iters[k] = max(3, min(2000, int(budget_ms * 1e3 / max(time_batch(fn, 3), 1.0))))
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(time_batch(fn, iters[k]))
    return {k: (statistics.median(v), min(v)) for k, v in times.items()}


def shapes(dev):
    """name, type, count, buffer bytes, the equivalent strided view of `buf` (or a same-volume one), exact?"""
    out = []
    v1 = dt.Type_vector(16384, 16, 32, dt.FLOAT)
    out.append(("1 MiB: 16,384 x 64 B / 128 B", v1, 1, 16384 * 128, lambda b: b.view(torch.float32).view(16384, 32)[:, :16], True))
    v2 = dt.Type_create_hvector(8192, 4, 16384, dt.FLOAT)
    out.append(("halo: 8,192 x 16 B / 16 KiB", v2, 1, 8192 * 16384, lambda b: b.view(torch.float32).view(8192, 4096)[:, :4], True))
    v3 = dt.Type_create_resized(dt.Type_create_hvector(16, 1024, 8192, dt.FLOAT), 0, 16 * 8192)
    out.append(("64 MiB: 4 KiB / 8 KiB", v3, 1024, 16384 * 8192, lambda b: b.view(torch.float32).view(16384, 2048)[:, :1024], True))
    st = dt.Type_create_struct([1, 2], [0, 8], [dt.INT, dt.FLOAT])
    out.append(("struct 12 of 16 B x 1 M", st, 1 << 20, 16 << 20, lambda b: b.view(torch.int32).view(1 << 20, 4)[:, 1:], False))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--budget-ms", type=float, default=200.0)
    ap.add_argument("--no-put", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dtype_pack_probe: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda")
    lines = ["# Derived datatypes on HBM: type_copy vs the byte-index path (benchmarks/dtype_pack_probe.py)", "",
             f"MI355X, one process; median (minimum) us per call over {a.rounds} alternating rounds of event-timed "
             "batches; GB/s = packed payload bytes over the median.", "",
             "| shape | direction | arm | us / call | GB/s | plan |", "|---|---|---|---|---|---|"]
    slower = []
    torch.manual_seed(7)
    for name, typ, count, nbytes, view_of, exact in shapes(dev):
        plan = typ.plan(count)
        assert plan.hi <= nbytes
        buf = torch.randint(1, 256, (nbytes,), dtype=torch.uint8, device=dev)
        view = view_of(buf)
        typ._idx_cache[(count, str(buf.device))] = plan_index(plan, dev)
        packed = typ.pack(buf, count)
        with index_path():
            ref = typ.pack(buf, count)
        assert torch.equal(packed, ref), name
        if exact:
            assert torch.equal(packed, view.contiguous().view(-1).view(torch.uint8)), name
        tgt_k, tgt_i = torch.zeros_like(buf), torch.zeros_like(buf)
        typ.unpack(packed, tgt_k, count)
        with index_path():
            typ.unpack(packed, tgt_i, count)
        assert torch.equal(tgt_k, tgt_i), name
        out = torch.empty_like(packed)
        tview = view_of(tgt_k)
        pk_shaped = packed.view(view.dtype).view(view.shape)

        def k_pack():
            typ.pack(buf, count, out=out)

        def i_pack():
            with index_path():
                typ.pack(buf, count)

        def k_unpack():
            typ.unpack(packed, tgt_k, count)

        def i_unpack():
            with index_path():
                typ.unpack(packed, tgt_i, count)

        desc = f"loops {plan.loops}, R {plan.R}, L {plan.L}, unit {plan.unit(buf.data_ptr(), out.data_ptr())}"
        res = ab({"kernel": k_pack, "index": i_pack, "torch": lambda: view.contiguous()}, a.rounds, a.budget_ms)
        res_u = ab({"kernel": k_unpack, "index": i_unpack, "torch": lambda: tview.copy_(pk_shaped)}, a.rounds, a.budget_ms)
        for direction, rr in (("pack", res), ("unpack", res_u)):
            for arm, (med, mn) in rr.items():
                lines.append(f"| {name} | {direction} | {arm} | {med:.1f} ({mn:.1f}) | {plan.total / med / 1e3:.1f} | "
                             f"{desc if arm == 'kernel' else ''} |")
            if rr["kernel"][0] > rr["index"][0]:
                slower.append((name, direction, rr["kernel"][0], rr["index"][0]))
        typ._idx_cache.clear()
        del buf, tgt_k, tgt_i, packed, ref, out
        torch.cuda.empty_cache()
    lines += ["", "Kernel slower than the index arm at: " + (", ".join(f"{n} {d} ({k:.1f} vs {i:.1f} us)" for n, d, k, i in slower)
                                                           if slower else "no probed shape or direction."), ""]

    # ---- host side: the 262,144-entry vector
    t0 = time.perf_counter()
    big = dt.Type_vector(16384, 16, 32, dt.FLOAT)
    t1 = time.perf_counter()
    big.plan(1)
    t2 = time.perf_counter()
    buf = torch.zeros(big.plan(1).hi, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    big.pack(buf, 1)
    torch.cuda.synchronize()
    t4 = time.perf_counter()
    with index_path():
        big.pack(buf, 1)
    torch.cuda.synchronize()
    t5 = time.perf_counter()
    idx_bytes = big._idx_cache[(1, str(buf.device))].numel() * 8
    lines += ["## Host side: Type_vector(16384, 16, 32, FLOAT), 262,144 type-map entries, 1 MiB payload", "",
              "| step | seconds |", "|---|---|",
              f"| construct the type (unchanged code) | {t1 - t0:.3f} |", f"| build its plan (once per type) | {t2 - t1:.3f} |",
              f"| first pack, kernel path (no table: R = 1) | {t4 - t3:.4f} |",
              f"| first pack, index path (builds and uploads a {idx_bytes >> 20} MiB index) | {t5 - t4:.3f} |", ""]

    # ---- Put with a derived target type: one launch vs one copy per run
    if not a.no_put:
        import mpit_amd as mp
        from mpit_amd import mpiT

        mp.Init()
        lines += ["## Put with a derived target type into a device window (target: this rank's own window, "
                  "the only peer one process has)", "", "| shape | arm | us / Put incl. Flush | copies or launches |", "|---|---|---|---|"]
        for name, typ, count, _, _, _ in shapes(dev)[:2]:
            plan = typ.plan(count)
            win = mpiT.Win_create(torch.zeros(-(-plan.hi // 16) * 16, dtype=torch.uint8, device=dev))
            src = torch.randint(1, 256, (plan.total,), dtype=torch.uint8).to(dev)

            def put():
                mpiT.Put(src, plan.total, dt.BYTE, 0, 0, count, typ, win)
                win.Flush()

            def timed(fn, reps):
                fn()
                ts = []
                for _ in range(reps):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    fn()
                    ts.append((time.perf_counter() - t) * 1e6)
                return statistics.median(ts)

            k = timed(put, 50)
            ref = win.tensor.clone()
            win.tensor.zero_()
            with index_path():
                c = timed(put, 5)
            assert torch.equal(win.tensor, ref), name
            lines.append(f"| {name} | one launch | {k:.1f} | 1 |")
            lines.append(f"| {name} | per-run copies | {c:.1f} | {len(typ.runs(count))} |")
            mpiT.Win_free(win)
        mp.Finalize()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
