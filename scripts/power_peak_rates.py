"""Rates of the peak-hold analysis (sdft_hip_sdft_power_peak_n) against the pooled power call on the same grid and against what a
host does without it, in the same process, on one MI355X.

    python scripts/power_peak_rates.py [--out profiles/power_peak_rates.txt] [--reps 5]

Device pointers, plain allocations, one plan per shape, warm-up calls first, every route timed by a pair of HIP events on the
plan's stream; the routes alternate within each repeat (so drift hits all alike); the median of the repeats is reported with
the smallest and the largest.  Per shape and `every`, all bins:

    max, min      sdft_hip_sdft_power_peak_n at `every`, first = 0, hold = max / min
    pooled        (a) sdft_hip_sdft_power_sum_n on the same grid: the same stores and the same recurrence, so the floor; its spread,
                  (max - min) / median, is the run-to-run spread the comparison is read against
    two-pass      (b) sdft_hip_sdft_power_n at every = 1, then torch: the [n][m] powers reshaped to [rows][every][m] and amax over the
                  middle axis on the same stream (every divides the samples used; the ragged last window is left to the host)

Shapes: configs[1] (n = 1e6, m = 1024, Hann, f32f64) at every = 100 and every = n; configs[2] (n = 262 144, m = 4096, Blackman,
f32f32) at every = 256.  Every max line is checked against the two-pass result, which holds the same terms (both calls cut time
alike): the count of elements whose bits differ is printed and has to be 0."""

from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "power_peak_rates.txt"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    from sdft_amd.sdft import SDFT, power_sum_rows
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

    log(f"# power_peak_rates.py  {time.strftime('%Y-%m-%d %H:%M:%S')}  device {torch.cuda.get_device_name(0)}  reps {reps} (median), 3 warm-up calls per route")
    log("# ms per call of n samples, all bins; / pooled = ms / pooled ms; two-pass / max = two-pass ms / max ms; spread = (max - min) / median of pooled")
    log("# differ = elements of the max call whose bits are not the two-pass result's")
    shapes = [("configs[1]", 1_000_000, 1024, "hann", "f32f64", (100, 1_000_000)),
              ("configs[2]", 262_144, 4096, "blackman", "f32f32", (256,))]
    for name, n, m, window, combo, everies in shapes:
        x = torch.from_numpy(sine_sweep(n) + noise(n, seed=m) * np.float32(0.25)).cuda()
        rdt = torch.float64 if combo.endswith("f64") else torch.float32
        with SDFT(m, window, 1.0, combo) as p:
            p.set_option("pipeline", 0)
            dense_out = torch.empty((n, m), dtype=rdt, device="cuda")
            for every in everies:
                rows = power_sum_rows(n, every, 0)
                whole = n // every                                     # windows the torch pass can reshape
                max_out = torch.empty((rows, m), dtype=rdt, device="cuda")
                min_out = torch.empty((rows, m), dtype=rdt, device="cuda")
                pooled_out = torch.empty((rows, m), dtype=rdt, device="cuda")
                second = torch.empty((whole, m), dtype=rdt, device="cuda")

                def hold_max():
                    p.power_peak(x, every, 0, hold="max", out=max_out)

                def hold_min():
                    p.power_peak(x, every, 0, hold="min", out=min_out)

                def pooled():
                    p.power_sum(x, every, 0, out=pooled_out)

                def two_pass():
                    p.power(x, 1, 0, out=dense_out)
                    torch.amax(dense_out[:whole * every].view(whole, every, m), dim=1, out=second)

                routes = [("max", hold_max), ("min", hold_min), ("pooled", pooled), ("two-pass", two_pass)]
                for _ in range(3):
                    for _, fn in routes:
                        p.reset()
                        fn()
                geo = None
                ts = {k: [] for k, _ in routes}
                for _ in range(reps):
                    for k, fn in routes:
                        ts[k].append(timed(p, fn))
                        if k == "max":
                            geo = (p.get_option("last_kernel"), p.get_option("last_chunks"), p.get_option("last_chunk_len"), p.get_option("last_chain"))
                # the same samples from the same state through both routes
                p.reset(); hold_max(); p.reset(); two_pass(); torch.cuda.synchronize()
                differ = int((max_out[:whole] != second).sum())
                mx, mn, mp, mt = stat(ts["max"]), stat(ts["min"]), stat(ts["pooled"]), stat(ts["two-pass"])
                spread = (mp[2] - mp[1]) / mp[0]
                log(f"{name} n={n} m={m} {window} {combo} every={every} rows={rows}: kernel {geo[0]} chunks {geo[1]} x {geo[2]} chain {geo[3]}  differ {differ}")
                log(f"  max      {mx[0]:.3f} ms  [min {mx[1]:.3f} max {mx[2]:.3f}]  / pooled {mx[0] / mp[0]:.3f}")
                log(f"  min      {mn[0]:.3f} ms  [min {mn[1]:.3f} max {mn[2]:.3f}]  / pooled {mn[0] / mp[0]:.3f}")
                log(f"  pooled   {mp[0]:.3f} ms  [min {mp[1]:.3f} max {mp[2]:.3f}]  spread {spread:.3f}")
                log(f"  two-pass {mt[0]:.3f} ms  [min {mt[1]:.3f} max {mt[2]:.3f}]  two-pass / max {mt[0] / mx[0]:.2f}")
                del max_out, min_out, pooled_out, second
            del dense_out
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
