"""Rates of the smoothed cross-spectrum analysis (sdft_hip_sdft_cross_smooth_n) against the pooled cross-spectrum call on the same
pairs and grid, against the smoothed power call over the same channels, and against what a host does without it, on one MI355X.

    python scripts/cross_smooth_rates.py [--out profiles/cross_smooth_rates.txt] [--reps 5]
    python scripts/cross_smooth_rates.py --step K           # one step in this process (what the driver starts, step by step)

The driver starts every step as a process of its own under a time limit of its own and stops at the first one that fails; within
a step everything runs in one process.  Device pointers, plain allocations, one plan per shape, warm-up calls first, every route
timed by a pair of HIP events on the plan's stream; the routes alternate within each repeat (so drift hits all alike); the median
of the repeats is reported with the smallest and the largest.  Per shape and `every`, all bins, decay = exp(-1 / 1000), state on
the device, disjoint pairs (0, 1), (2, 3), ...:

    smooth        sdft_hip_sdft_cross_smooth_n at `every`, first = 0
    no rows       the same call with first = n: no row is kept, so no store and no fix-up -- the recurrences, the recursion and
                  the scan of the chunks' end values alone (smooth - no rows: the stores and the fix-up kernel)
    cross sum     (a) sdft_hip_sdft_cross_sum_n on the same pairs and grid: the peer -- the same recurrences and term, an addition
                  in the recursion's place; its spread, (max - min) / median, is what the comparison is read against
    power smooth  (b) sdft_hip_sdft_power_smooth_n over the same channels on the same grid: the floor that forms no cross term (it
                  stores as many bytes: a real row per channel for a complex row per pair of channels)

and, at the north star's length (n = 48 000, m = 1024, f32f64, two channels, one pair), where a launch per row is tolerable:

    row loop      (c) sdft_sdft_n of both channels, then torch, one row at a time: s.mul_(a).add_(X0[t] * conj(X1[t]), alpha=b) --
                  the only route before this call -- against the smoothed call at every = 1, whose rows it is compared with

Shapes: one GPU's share of configs[4] (64 channels x 48 000 samples, m = 1024, Hann, f32f64, 32 pairs) at every = 100 and
every = 1; f32f32 at 16 channels (8 pairs), likewise."""

from __future__ import annotations

import argparse
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINES = [("configs[4] / GPU", 64, 48_000, 1024, "hann", "f32f64", 100),
         ("configs[4] / GPU", 64, 48_000, 1024, "hann", "f32f64", 1),
         ("16 channels", 16, 48_000, 1024, "hann", "f32f32", 100),
         ("16 channels", 16, 48_000, 1024, "hann", "f32f32", 1)]
ROW_LOOP = len(LINES)                                        # the step after the lines
LIMITS = [240, 300, 180, 240, 420]                           # seconds per step
DECAY = math.exp(-1.0 / 1000.0)


def step(k, reps):
    import numpy as np
    import torch
    from sdft_amd.sdft import SDFT, every_rows
    from sdft_amd.signals import noise, sine_sweep

    torch.cuda.set_device(0)

    def log(s):
        print(s, flush=True)

    def timed(p, fn):
        stream = torch.cuda.ExternalStream(p.api.get_stream(p._p))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        with torch.cuda.stream(stream):
            fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def stat(ts):
        return float(np.median(ts)), min(ts), max(ts)

    def samples(ch, n, m):
        x = np.stack([sine_sweep(n) * np.float32(1.0 + 0.01 * c) + noise(n, seed=m + c) * np.float32(0.25) for c in range(ch)])
        return torch.from_numpy(x.astype(np.float32)).cuda()

    if k == 0:
        log(f"# device {torch.cuda.get_device_name(0)}")
    if k < ROW_LOOP:
        name, ch, n, m, window, combo, every = LINES[k]
        double = combo.endswith("f64")
        rdt, cdt = (torch.float64, torch.complex128) if double else (torch.float32, torch.complex64)
        npairs = ch // 2
        x = samples(ch, n, m)
        with SDFT(m, window, 1.0, combo, ch) as p:
            p.set_option("pipeline", 0)
            p.set_pairs(list(range(0, ch, 2)), list(range(1, ch, 2)))
            rows = every_rows(n, every, 0)
            smooth_out = torch.empty((npairs, rows, m), dtype=cdt, device="cuda")
            other = torch.empty((npairs, rows, m), dtype=cdt, device="cuda")      # the peer's rows and the floor's, in turn
            floor_out = torch.view_as_real(other).reshape(ch, rows, m)             # (as many bytes: [channels][rows][m] real)
            state = torch.zeros((npairs, m), dtype=cdt, device="cuda")
            pstate = torch.zeros((ch, m), dtype=rdt, device="cuda")

            def smooth():
                p.cross_smooth(x, DECAY, every, 0, state=state, out=smooth_out)

            def no_rows():
                p.cross_smooth(x, DECAY, every, n, state=state)

            def cross_sum():
                p.cross_sum(x, every, 0, out=other)

            def power_smooth():
                p.power_smooth(x, DECAY, every, 0, state=pstate, out=floor_out)

            routes = [("smooth", smooth), ("no rows", no_rows), ("cross sum", cross_sum), ("power smooth", power_smooth)]
            for _ in range(3):
                for _, fn in routes:
                    p.reset()
                    fn()
            geo = None
            ts = {name_: [] for name_, _ in routes}
            for _ in range(reps):
                for name_, fn in routes:
                    ts[name_].append(timed(p, fn))
                    if name_ == "smooth":
                        geo = (p.get_option("last_kernel"), p.get_option("last_chunks"), p.get_option("last_chunk_len"), p.get_option("last_chain"))
            ms, mn, mc, mf = stat(ts["smooth"]), stat(ts["no rows"]), stat(ts["cross sum"]), stat(ts["power smooth"])
            spread = (mc[2] - mc[1]) / mc[0]
            log(f"{name} channels={ch} pairs={npairs} n={n} m={m} {window} {combo} every={every} rows={rows}: kernel {geo[0]} chunks {geo[1]} x {geo[2]} chain {geo[3]}")
            log(f"  smooth        {ms[0]:.3f} ms  [min {ms[1]:.3f} max {ms[2]:.3f}]  / cross sum {ms[0] / mc[0]:.3f}  / power smooth {ms[0] / mf[0]:.3f}")
            log(f"  no rows       {mn[0]:.3f} ms  [min {mn[1]:.3f} max {mn[2]:.3f}]  / cross sum {mn[0] / mc[0]:.3f}  rows+fix {ms[0] - mn[0]:.3f} ms")
            log(f"  cross sum     {mc[0]:.3f} ms  [min {mc[1]:.3f} max {mc[2]:.3f}]  spread {spread:.3f}")
            log(f"  power smooth  {mf[0]:.3f} ms  [min {mf[1]:.3f} max {mf[2]:.3f}]")
        return

    # (c) the only route before this call: the rows of both channels and a launch or three per row
    n, m, window, combo = 48_000, 1024, "hann", "f32f64"
    x = samples(2, n, m)
    with SDFT(m, window, 1.0, combo, 2) as p:
        p.set_option("pipeline", 0)
        p.set_pairs([0], [1])
        a, b = DECAY, 1.0 - DECAY                                  # (FD double: the call's own coefficients)
        dense = torch.empty((2, n, m), dtype=torch.complex128, device="cuda")
        looped = torch.empty((n, m), dtype=torch.complex128, device="cuda")
        smooth_out = torch.empty((1, n, m), dtype=torch.complex128, device="cuda")
        state = torch.zeros((1, m), dtype=torch.complex128, device="cuda")

        def smooth():
            state.zero_()
            p.cross_smooth(x, DECAY, 1, 0, state=state, out=smooth_out)

        def row_loop():
            p.sdft(x, out=dense)
            s = torch.zeros(m, dtype=torch.complex128, device="cuda")
            for t in range(n):
                s.mul_(a).add_(dense[0, t] * dense[1, t].conj(), alpha=b)
                looped[t] = s

        def row_loop_no_copy():
            p.sdft(x, out=dense)
            s = torch.zeros(m, dtype=torch.complex128, device="cuda")
            for t in range(n):
                s.mul_(a).add_(dense[0, t] * dense[1, t].conj(), alpha=b)

        routes = [("smooth", smooth), ("row loop", row_loop), ("row loop, last row only", row_loop_no_copy)]
        for _, fn in routes:
            p.reset()
            fn()
        ts = {name_: [] for name_, _ in routes}
        for _ in range(reps):
            for name_, fn in routes:
                ts[name_].append(timed(p, fn))
        p.reset(); smooth(); p.reset(); row_loop(); torch.cuda.synchronize()
        big = float(dense[0].abs().max()) * float(dense[1].abs().max())
        scale = big * 2.0 ** -53 / (1.0 - a)
        worst = float(torch.view_as_real(smooth_out[0] - looped).abs().max()) / scale
        ms = stat(ts["smooth"])
        log(f"north star n={n} m={m} {window} {combo} channels=2 pairs=1 every=1 rows={n}: chunks {p.get_option('last_chunks')} x {p.get_option('last_chunk_len')}; "
            f"largest |smooth - row loop| = {worst:.2f} u max|X0| max|X1| / (1 - a)")
        log(f"  smooth   {ms[0]:.3f} ms  [min {ms[1]:.3f} max {ms[2]:.3f}]")
        for name_ in ("row loop", "row loop, last row only"):
            mt = stat(ts[name_])
            log(f"  {name_:8s} {mt[0]:.3f} ms  [min {mt[1]:.3f} max {mt[2]:.3f}]  / smooth {mt[0] / ms[0]:.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_smooth_rates.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step", type=int, default=None)
    args = ap.parse_args()
    if args.step is not None:
        step(args.step, args.reps)
        return
    lines = [f"# cross_smooth_rates.py  {time.strftime('%Y-%m-%d %H:%M:%S')}  reps {args.reps} (median), 3 warm-up calls per route, a process per step",
             "# ms per call of n samples per channel, all bins; / cross sum = ms / cross-sum ms; spread = (max - min) / median of cross sum; rows+fix = smooth ms - no-rows ms"]
    print("\n".join(lines), flush=True)
    status = 0
    for k in range(ROW_LOOP + 1):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", str(k), "--reps", str(args.reps)], capture_output=True, text=True,
                               timeout=LIMITS[k])
        except subprocess.TimeoutExpired:
            print(f"step {k}: not finished within {LIMITS[k]} s; nothing further is started", flush=True)
            status = 1
            break
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            print(f"step {k}: exit status {r.returncode}; nothing further is started\n{r.stderr[-2000:]}", flush=True)
            status = 1
            break
        lines += r.stdout.splitlines()
    if args.out and status == 0:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(status)


if __name__ == "__main__":
    main()
