"""One-sided Accumulate on HBM: the one-launch type_accumulate path against the per-run axpby
path and against Put of the same layout.

    python benchmarks/type_acc_probe.py [--out profiles/type_accumulate.md] [--reps 30]

One process, one GPU, a device window whose only member (and so only target) is this rank.
Layouts: Type_vector(R, 2, 5, FLOAT) with R = 64, 1,024 and 16,384; one irregular type of 1,024
runs (4 to 64 B each, seeded); one contiguous 64 MiB range of FLOAT. Arms, per layout:

* ``per-run``     mpiT.Accumulate(SUM) under MPIT_DTYPE_KERNEL=0: one lock, one axpby launch and one
                  stream synchronise per contiguous run of the target type. This is the code the
                  call ran before type_accumulate existed, kept verbatim: the baseline;
* ``one launch``  the same call on the default path: one lock, one type_accumulate launch, one
                  synchronise;
* ``put``         the same layout written by one type_copy launch (Win._plan_copy) and a Flush: two
                  streams where accumulate moves three, the bandwidth yardstick.

Every call is blocking, so a call is timed by the host clock from a synchronised device to its
return, after one untimed call of the same arm; the arms alternate for --reps rounds (three for
an arm that takes over 50 ms) after a warm-up of each, and the table gives the median and the
minimum. GB/s is the payload (the packed bytes of the layout) over the median: an accumulate at
Put's memory rate shows 2/3 of Put's figure. The two accumulate arms are compared bitwise on the whole window before timing."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mpit_amd import datatypes as dt
from mpit_amd.window import contiguous_plan


class per_run_path:
    """MPIT_DTYPE_KERNEL=0 for the calls inside (the switch is read per call)."""

    def __enter__(self):
        self.old = os.environ.get("MPIT_DTYPE_KERNEL")
        os.environ["MPIT_DTYPE_KERNEL"] = "0"

    def __exit__(self, *a):
        if self.old is None:
            del os.environ["MPIT_DTYPE_KERNEL"]
        else:
            os.environ["MPIT_DTYPE_KERNEL"] = self.old


def layouts():
    """name, target type, count"""
    out = [(f"vector R = {R:,}: 8 B / 20 B", dt.Type_vector(R, 2, 5, dt.FLOAT), 1) for R in (64, 1024, 16384)]
    rng = np.random.default_rng(3)
    lens = rng.integers(1, 17, 1024)
    gaps = rng.integers(1, 9, 1024)
    offs = np.concatenate([[0], np.cumsum(lens + gaps)[:-1]]) * 4
    out.append(("irregular, 1,024 runs of 4..64 B", dt.Type_create_hindexed([int(x) for x in lens], [int(x) for x in offs], dt.FLOAT), 1))
    out.append(("contiguous 64 MiB", dt.FLOAT, 16 << 20))
    return out


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        fn()  # untimed: the arm that ran before this one leaves clocks and caches in its own state
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e6)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("type_acc_probe: needs the GPU (a CPU timing says nothing about it)")
    import mpit_amd as mp
    from mpit_amd import mpiT

    dev = torch.device("cuda")
    mp.Init()
    lines = ["# One-sided Accumulate on HBM: one type_accumulate launch vs one axpby per run (benchmarks/type_acc_probe.py)", "",
             "MI355X, one process, self-targeted device window; median "
             f"(minimum) us per blocking call by the host clock over up to {a.reps} alternating rounds; GB/s = packed "
             "payload over the median.", "",
             "| layout | arm | us / call | GB/s | locks, launches, synchronises |", "|---|---|---|---|---|"]
    torch.manual_seed(7)
    for name, typ, count in layouts():
        basic = typ.is_contiguous_basic()
        plan = contiguous_plan(typ.Get_size() * count) if basic else typ.plan(count)
        runs = 1 if basic else len(typ.runs(count))
        ne = plan.total // 4
        win = mpiT.Win_create(torch.zeros(-(-plan.hi // 16) * 4, dtype=torch.float32, device=dev))
        src = torch.randint(-8, 9, (ne,), device=dev).float()
        raw = src.view(torch.uint8)

        def acc():
            mpiT.Accumulate(src, ne, dt.FLOAT, 0, 0, count, typ, mpiT.SUM, win)

        def acc_runs():
            with per_run_path():
                acc()

        def put():
            win._plan_copy(True, raw, 0, 0, plan)
            win.Flush()

        before = dict(dt.COUNTERS)
        acc()
        one = win.tensor.clone()
        win.tensor.zero_()
        acc_runs()
        assert torch.equal(win.tensor, one) and bool(one.any()), name
        assert dt.COUNTERS["rma_acc_kernel"] == before["rma_acc_kernel"] + 1
        assert dt.COUNTERS["rma_acc_runs"] == before["rma_acc_runs"] + runs
        arms = {"per-run": acc_runs, "one launch": acc, "put": put}
        reps = {}
        for k, fn in arms.items():  # warm-up, and fewer rounds for a slow arm
            first = statistics.median(timed(fn, 2))
            reps[k] = a.reps if first < 50e3 else 3
        times = {k: [] for k in arms}
        for i in range(a.reps):
            for k, fn in arms.items():
                if i < reps[k]:
                    times[k] += timed(fn, 1)
        for k, v in times.items():
            med, mn = statistics.median(v), min(v)
            cost = f"{runs:,} each" if k == "per-run" else ("1 each" if k == "one launch" else "no lock, 1 launch, 1 Flush")
            lines.append(f"| {name} ({plan.total:,} B) | {k} | {med:.1f} ({mn:.1f}) | {plan.total / med / 1e3:.2f} | {cost} |")
        mpiT.Win_free(win)
        del win, src, raw, one
        torch.cuda.empty_cache()
    mp.Finalize()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
