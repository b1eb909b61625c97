"""Development probe: where the prefix-cell route of long analysis calls stops paying.  prefix_cells_kernel adds the n / 2N
differences of a cell one after the other, on 2N / 32 workgroups per channel, so its time grows with the rows per cell; the
partial sums + scan it replaces are parallel over the chunks and do not.  This A/B gives the bound of the route
(logic::kPrefixRowsMax in sdft_plan_logic.hpp).

Per shape (m, n), Hann, f32f64, one channel, asynchronous calls into one matrix on the caller's stream, ONE plan (hooks library):
    old   prefix_cells = 0    partial sums + scan
    new   prefix_cells = 2    prefix cells whatever the length (the hook passes the bound)
Rounds alternate old, new; a round is `steps` calls between synchronises by the host clock.  The parts of a step come from the
plan's per-stage events (profile = 1).  A shape counts FOR the route when new is faster in every round and the median
old - new is larger than the largest difference between two rounds of one side; AGAINST when the same holds the other way;
else it is a tie.

    python scripts/prefix_cells_rows_ab.py [--rounds 8] [--steps 10] [--out profiles/prefix_cells_rows_ab.txt]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from sdft_amd.sdft import SDFT
from sdft_amd.signals import sine_sweep

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "prefix_cells_rows_ab.txt"))
args = ap.parse_args()

NEAR = (1 << 19) + 4096
SHAPES = [(1024, NEAR), (1024, 1000000), (1024, 4000000), (512, 1000000), (512, 4000000), (256, NEAR), (256, 2000000), (256, 4000000),
          (128, 1000000), (128, 2000000), (64, NEAR), (64, 1000000), (64, 10000000), (8, NEAR), (8, 10000000)]
SIDES = [("old", 0), ("new", 2)]
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


torch.cuda.set_device(0)
stream = torch.cuda.Stream()
say(f"prefix cells against partial sums + scan by rows per cell: hann, f32f64, one channel, {args.rounds} rounds of {args.steps} asynchronous steps per side")
say("rows = ceil(n / 2N) per cell, wgs = workgroups of prefix_cells_kernel; pre-pass = launches in front of the row kernel (plan events), step = host clock, us")
say()
say(f"{'m':>5s} {'n':>9s} {'rows':>6s} {'wgs':>4s} {'chunks':>6s} | {'pre old':>8s} {'pre new':>8s} | {'step old':>9s} {'step new':>9s} {'old-new':>8s} {'spread':>7s} {'new wins':>8s}  verdict")
for m, n in SHAPES:
    x = torch.from_numpy(sine_sweep(n, channel=0, channels=1, dtype=np.float32)).cuda()
    out = torch.empty((n, m), dtype=torch.complex128, device="cuda")
    plan = SDFT(m, "hann", 1.0, "f32f64", hooks=True)
    plan.set_stream(stream.cuda_stream)
    plan.set_option("async", 1)

    def sync():
        plan.synchronize()
        torch.cuda.synchronize()

    pre, chunks = {}, 0
    for name, pc in SIDES:
        plan.set_option("prefix_cells", pc)
        plan.set_option("profile", 1)
        for _ in range(3):
            plan.sdft(x, out)
        sync(); plan.profile()
        for _ in range(5):
            plan.sdft(x, out)
        sync()
        pr = plan.profile()
        pre[name] = (pr["delta"][0] + pr["carry"][0]) / max(pr["forward"][1], 1) * 1e3
        chunks = plan.get_option("last_chunks")
        assert plan.get_option("last_prefix") == (1 if pc else 0) and plan.get_option("last_self") == 0, (name, m, n)
    plan.set_option("profile", 0)
    step = {name: [] for name, _ in SIDES}
    for r in range(args.rounds):
        for name, pc in SIDES:
            plan.set_option("prefix_cells", pc)
            plan.sdft(x, out)
            sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                plan.sdft(x, out)
            sync()
            step[name].append((time.perf_counter() - t0) / args.steps * 1e6)
    diff = np.array(step["old"]) - np.array(step["new"])
    spread = max(max(v) - min(v) for v in step.values())
    wins, med = int((diff > 0).sum()), float(np.median(diff))
    verdict = "for" if wins == args.rounds and med > spread else "against" if wins == 0 and -med > spread else "tie"
    say(f"{m:5d} {n:9d} {(n + 2 * m - 1) // (2 * m):6d} {(2 * m + 31) // 32:4d} {chunks:6d} | {pre['old']:8.1f} {pre['new']:8.1f} | {np.median(step['old']):9.1f} {np.median(step['new']):9.1f} "
        f"{med:8.1f} {spread:7.1f} {wins:5d}/{args.rounds:<2d}  {verdict}")
    plan.close()
    del out, x
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
