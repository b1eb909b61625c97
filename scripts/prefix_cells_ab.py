"""Development probe: A/B of the carry pre-pass of the headline (BASELINE configs[1]: n = 1e6, m = 1024, Hann, f32f64, one channel,
asynchronous calls into one placed matrix on the caller's stream) inside one process -- leases differ by more than the effect.

Sides, switched by the test hook prefix_cells and the chunk option on ONE plan (hooks library), same buffers:
    old   prefix_cells = 0            partial sums + scan (chunk_fft_kernel, carry_scan_kernel), two rounds of the chip
    new   prefix_cells = 1            prefix cells (prefix_cells_kernel) + self-carried row kernel, two rounds of the chip
    new1  prefix_cells = 1, chunk = 3912   the same in ONE round of 256 longer chunks

Each round is 20 asynchronous steps between synchronises, timed by the host clock; the plan's own events give the forward kernel's
time (profile = 2).  Rounds alternate old, new, new1, old, ...  The rule, fixed before the run: a new side's gain COUNTS if it is
faster than old in at least 11 of 12 rounds (of every 12; here: rounds - 1 of the rounds) AND the median old - new difference is
larger than the largest difference between two rounds of the same side.

--dumps PARENT_DIR THIS_DIR appends "results unchanged": the largest difference between what `bench.py --dump-outputs DIR` wrote
at the parent commit and at this one (the order of the carry sums is the only difference between the two pre-passes).

    python scripts/prefix_cells_ab.py [--rounds 12] [--dumps PARENT_DIR THIS_DIR] [--out profiles/prefix_cells_ab.txt]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import place_matrix
from sdft_amd.sdft import SDFT
from sdft_amd.signals import sine_sweep

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=12)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "prefix_cells_ab.txt"))
ap.add_argument("--dumps", nargs=2, metavar=("PARENT_DIR", "THIS_DIR"), default=None)
args = ap.parse_args()
assert args.rounds >= 12

n, m = 1000000, 1024
SIDES = [("old", {"prefix_cells": 0, "chunk": 0}), ("new", {"prefix_cells": 1, "chunk": 0}), ("new1", {"prefix_cells": 1, "chunk": 3912})]
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


torch.cuda.set_device(0)
x = torch.from_numpy(sine_sweep(n, channel=0, channels=1, dtype=np.float32)).cuda()
out, placement, holder = place_matrix(torch, (n, m), torch.complex128)
stream = torch.cuda.Stream()
plan = SDFT(m, "hann", 1.0, "f32f64", hooks=True)
plan.set_stream(stream.cuda_stream)
plan.set_option("async", 1)


def sync():
    plan.synchronize()
    torch.cuda.synchronize()


def side(opts):
    for k, v in opts.items():
        plan.set_option(k, v)


say(f"prefix cells A/B: n = {n}, m = {m}, hann, f32f64, {args.rounds} rounds of {args.steps} asynchronous steps per side, one plan, one matrix")
say(f"matrix: placed = {placement['placed']} ({placement.get('window_gbs', 0)} GB/s window)")

# warm-up and the parts of a step by the plan's per-stage events (profile = 1: every launch bracketed)
parts = {}
for name, opts in SIDES:
    side(opts)
    plan.set_option("profile", 1)
    for _ in range(3):
        plan.sdft(x, out)
    sync(); plan.profile()
    for _ in range(5):
        plan.sdft(x, out)
    sync()
    pr = plan.profile()
    calls = max(pr["forward"][1], 1)
    parts[name] = dict(chunks=plan.get_option("last_chunks"), len=plan.get_option("last_chunk_len"), prefix=plan.get_option("last_prefix"), self_=plan.get_option("last_self"),
                       prepass_us=(pr["delta"][0] + pr["carry"][0]) / calls * 1e3, forward_ms=pr["forward"][0] / calls)
say()
say("parts of a step (plan events around every launch, 5 steps):")
for name, _ in SIDES:
    q = parts[name]
    say(f"  {name:5s} chunks {q['chunks']} x {q['len']}  last_prefix {q['prefix']} last_self {q['self_']}  pre-pass launches {q['prepass_us']:.1f} us  forward kernel {q['forward_ms']:.4f} ms")

plan.set_option("profile", 2)
step = {name: [] for name, _ in SIDES}
kern = {name: [] for name, _ in SIDES}
for r in range(args.rounds):
    for name, opts in SIDES:
        side(opts)
        plan.sdft(x, out)                                    # (one untimed step after the switch: the workspace of this side is in place)
        sync(); plan.profile()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            plan.sdft(x, out)
        sync()
        dt = time.perf_counter() - t0
        pf = plan.profile()["forward"]
        step[name].append(dt / args.steps * 1e3)
        kern[name].append(pf[0] / max(pf[1], 1))

say()
say("ms per step (host clock between synchronises) | forward kernel ms (plan events)")
say("round   " + "   ".join(f"{name:>7s} {'kernel':>7s}" for name, _ in SIDES))
for r in range(args.rounds):
    say(f"{r:5d}   " + "   ".join(f"{step[name][r]:7.4f} {kern[name][r]:7.4f}" for name, _ in SIDES))
say("median  " + "   ".join(f"{np.median(step[name]):7.4f} {np.median(kern[name]):7.4f}" for name, _ in SIDES))
spread = max(max(v) - min(v) for v in step.values())
say()
say(f"largest difference between two rounds of the same side: {spread * 1e3:.1f} us  (" + ", ".join(f"{name} {(max(v) - min(v)) * 1e3:.1f}" for name, v in step.items()) + ")")
verdicts = {}
for name in ("new", "new1"):
    diff = np.array(step["old"]) - np.array(step[name])
    wins = int((diff > 0).sum())
    need = args.rounds - max(1, args.rounds // 12)
    med = float(np.median(diff))
    ok = wins >= need and med > spread
    verdicts[name] = ok
    say(f"{name:5s} against old: faster in {wins} of {args.rounds} rounds (needs {need}); median old - {name} = {med * 1e3:.1f} us (needs > {spread * 1e3:.1f} us): "
        f"{'the gain COUNTS' if ok else 'the gain does NOT count'}")
d2 = np.array(step["new"]) - np.array(step["new1"])
say(f"one round of chunks against two: new - new1 median {float(np.median(d2)) * 1e3:.1f} us, new1 faster in {int((d2 > 0).sum())} of {args.rounds} rounds")
if args.dumps:
    a, b = (np.load(os.path.join(d, "dfts.npy")) for d in args.dumps)
    ra, rb = (np.load(os.path.join(d, "dfts_rows.npy")) for d in args.dumps)
    assert a.shape == b.shape and np.array_equal(ra, rb)
    za, zb = a[..., 0] + 1j * a[..., 1], b[..., 0] + 1j * b[..., 1]
    whole = float(np.abs(zb - za).max() / np.abs(za).max())
    per_row = float((np.abs(zb - za).max(axis=1) / np.abs(za).max(axis=1)).max())
    say()
    say("results unchanged (bench.py --dump-outputs at the parent commit and at this one, the same seeded sample of rows of the last timed step):")
    say(f"rows compared: {za.shape[0]} of {za.shape[1]} bins; largest |new - parent| / largest |parent| = {whole:.3e}; largest per-row relative difference = {per_row:.3e}")
    say("(inside the 1e-11 the full-size tests hold against the oracle; the order of the carry sums is the only difference)" if per_row <= 1e-11
        else "(OUTSIDE the 1e-11 the full-size tests hold against the oracle)")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
plan.close()
if holder is not None:
    holder.free()
