"""Rates of the smoothed power analysis (sdft_hip_sdft_power_smooth_n) against the pooled power call on the same grid and against what
a host does without it, in the same process, on one MI355X.

    python scripts/power_smooth_rates.py [--out profiles/power_smooth_rates.txt] [--reps 5]
    python scripts/power_smooth_rates.py --once 0|1|2        # one line's call, three times: the form a kernel trace takes

Device pointers, plain allocations, one plan per shape, warm-up calls first, every route timed by a pair of HIP events on the
plan's stream; the routes alternate within each repeat (so drift hits all alike); the median of the repeats is reported with
the smallest and the largest.  Per shape and `every`, all bins, decay = exp(-1 / 1000), state on the device:

    smooth        sdft_hip_sdft_power_smooth_n at `every`, first = 0
    no rows       the same call with first = n: no row is kept, so no store and no fix-up -- the recurrence, the recursion and
                  the scan of the chunks' end values alone (smooth - no rows: the stores and the fix-up kernel)
    pooled        (a) sdft_hip_sdft_power_sum_n on the same grid: the same recurrence and one accumulator, so the floor; its spread,
                  (max - min) / median, is the run-to-run spread the comparison is read against
    power         sdft_hip_sdft_power_n on the same grid (at every = 1 it stores what the smoothed call stores, once)

and, at the north star's shape (n = 48 000, m = 1024, f32f64), where a launch per row is still tolerable:

    row loop      (b) sdft_hip_sdft_power_n at every = 1, then torch, one row at a time: s.mul_(a).add_(p[t], alpha=b) -- the only
                  route before this call -- against the smoothed call at every = 1, whose rows it is compared with

Shapes: configs[1] (n = 1e6, m = 1024, Hann, f32f64) at every = 100 and every = 1; configs[2] (n = 262 144, m = 4096, Blackman,
f32f32) at every = 256."""

from __future__ import annotations

import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINES = [("configs[1]", 1_000_000, 1024, "hann", "f32f64", 100),
         ("configs[1]", 1_000_000, 1024, "hann", "f32f64", 1),
         ("configs[2]", 262_144, 4096, "blackman", "f32f32", 256)]
DECAY = math.exp(-1.0 / 1000.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "power_smooth_rates.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--once", type=int, default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from sdft_amd.sdft import SDFT, every_rows
    from sdft_amd.signals import noise, sine_sweep

    torch.cuda.set_device(0)
    reps = args.reps
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

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

    def samples(n, m):
        return torch.from_numpy(sine_sweep(n) + noise(n, seed=m) * np.float32(0.25)).cuda()

    if args.once is not None:
        name, n, m, window, combo, every = LINES[args.once]
        rdt = torch.float64 if combo.endswith("f64") else torch.float32
        x = samples(n, m)
        with SDFT(m, window, 1.0, combo) as p:
            p.set_option("pipeline", 0)
            out = torch.empty((every_rows(n, every, 0), m), dtype=rdt, device="cuda")
            state = torch.zeros(m, dtype=rdt, device="cuda")
            for _ in range(3):
                p.power_smooth(x, DECAY, every, 0, state=state, out=out)
            torch.cuda.synchronize()
            print(f"once: {name} n={n} m={m} {combo} every={every} chunks {p.get_option('last_chunks')} x {p.get_option('last_chunk_len')}")
        return

    log(f"# power_smooth_rates.py  {time.strftime('%Y-%m-%d %H:%M:%S')}  device {torch.cuda.get_device_name(0)}  reps {reps} (median), 3 warm-up calls per route")
    log("# ms per call of n samples, all bins; / pooled = ms / pooled ms; spread = (max - min) / median of pooled; rows+fix = smooth ms - no-rows ms")
    for name, n, m, window, combo, every in LINES:
        rdt = torch.float64 if combo.endswith("f64") else torch.float32
        x = samples(n, m)
        with SDFT(m, window, 1.0, combo) as p:
            p.set_option("pipeline", 0)
            rows = every_rows(n, every, 0)
            smooth_out = torch.empty((rows, m), dtype=rdt, device="cuda")
            other_out = torch.empty((rows, m), dtype=rdt, device="cuda")       # the pooled and the power call's rows, in turn
            state = torch.zeros(m, dtype=rdt, device="cuda")

            def smooth():
                p.power_smooth(x, DECAY, every, 0, state=state, out=smooth_out)

            def no_rows():
                p.power_smooth(x, DECAY, every, n, state=state)

            def pooled():
                p.power_sum(x, every, 0, out=other_out)

            def power():
                p.power(x, every, 0, out=other_out)

            routes = [("smooth", smooth), ("no rows", no_rows), ("pooled", pooled), ("power", power)]
            for _ in range(3):
                for _, fn in routes:
                    p.reset()
                    fn()
            geo = None
            ts = {k: [] for k, _ in routes}
            for _ in range(reps):
                for k, fn in routes:
                    ts[k].append(timed(p, fn))
                    if k == "smooth":
                        geo = (p.get_option("last_kernel"), p.get_option("last_chunks"), p.get_option("last_chunk_len"), p.get_option("last_chain"))
            ms, mn, mp, mw = stat(ts["smooth"]), stat(ts["no rows"]), stat(ts["pooled"]), stat(ts["power"])
            spread = (mp[2] - mp[1]) / mp[0]
            log(f"{name} n={n} m={m} {window} {combo} every={every} rows={rows}: kernel {geo[0]} chunks {geo[1]} x {geo[2]} chain {geo[3]}")
            log(f"  smooth   {ms[0]:.3f} ms  [min {ms[1]:.3f} max {ms[2]:.3f}]  / pooled {ms[0] / mp[0]:.3f}  / power {ms[0] / mw[0]:.3f}")
            log(f"  no rows  {mn[0]:.3f} ms  [min {mn[1]:.3f} max {mn[2]:.3f}]  / pooled {mn[0] / mp[0]:.3f}  rows+fix {ms[0] - mn[0]:.3f} ms")
            log(f"  pooled   {mp[0]:.3f} ms  [min {mp[1]:.3f} max {mp[2]:.3f}]  spread {spread:.3f}")
            log(f"  power    {mw[0]:.3f} ms  [min {mw[1]:.3f} max {mw[2]:.3f}]")
            del smooth_out, other_out
        torch.cuda.empty_cache()

    # (b) the only route before this call: the dense power call and a launch per row
    n, m, window, combo = 48_000, 1024, "hann", "f32f64"
    x = samples(n, m)
    with SDFT(m, window, 1.0, combo) as p:
        p.set_option("pipeline", 0)
        a, b = DECAY, 1.0 - DECAY                                  # (FD double: the call's own coefficients)
        dense = torch.empty((n, m), dtype=torch.float64, device="cuda")
        looped = torch.empty((n, m), dtype=torch.float64, device="cuda")
        smooth_out = torch.empty((n, m), dtype=torch.float64, device="cuda")
        state = torch.zeros(m, dtype=torch.float64, device="cuda")

        def smooth():
            state.zero_()
            p.power_smooth(x, DECAY, 1, 0, state=state, out=smooth_out)

        def row_loop():
            p.power(x, 1, 0, out=dense)
            s = torch.zeros(m, dtype=torch.float64, device="cuda")
            for t in range(n):
                s.mul_(a).add_(dense[t], alpha=b)
                looped[t] = s

        def row_loop_no_copy():
            p.power(x, 1, 0, out=dense)
            s = torch.zeros(m, dtype=torch.float64, device="cuda")
            for t in range(n):
                s.mul_(a).add_(dense[t], alpha=b)

        routes = [("smooth", smooth), ("row loop", row_loop), ("row loop, last row only", row_loop_no_copy)]
        for _, fn in routes:
            p.reset()
            fn()
        ts = {k: [] for k, _ in routes}
        for _ in range(reps):
            for k, fn in routes:
                ts[k].append(timed(p, fn))
        p.reset(); smooth(); p.reset(); row_loop(); torch.cuda.synchronize()
        scale = float(dense.max()) * 2.0 ** -53 / (1.0 - a)
        worst = float((smooth_out - looped).abs().max()) / scale
        ms = stat(ts["smooth"])
        log(f"north star n={n} m={m} {window} {combo} every=1 rows={n}: chunks {p.get_option('last_chunks')} x {p.get_option('last_chunk_len')}; "
            f"largest |smooth - row loop| = {worst:.2f} u pmax / (1 - a)")
        log(f"  smooth   {ms[0]:.3f} ms  [min {ms[1]:.3f} max {ms[2]:.3f}]")
        for k in ("row loop", "row loop, last row only"):
            mt = stat(ts[k])
            log(f"  {k:8s} {mt[0]:.3f} ms  [min {mt[1]:.3f} max {mt[2]:.3f}]  / smooth {mt[0] / ms[0]:.1f}")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
