"""Rates of the smoothed peak-hold analysis (sdft_hip_sdft_smooth_peak_n) against the peak-hold call on the same grid, against the
only route before it and against the smoothed call sampled on the grid, in the same process, on one MI355X.

    python scripts/smooth_peak_rates.py [--out profiles/smooth_peak_rates.txt] [--reps 5]
    python scripts/smooth_peak_rates.py --once 0|1|2|3       # one line's call, three times: the form a kernel trace takes

Device pointers, plain allocations, one plan per shape, warm-up calls first, every route timed by a pair of HIP events on the
plan's stream; the routes alternate within each repeat (so drift hits all alike); the median of the repeats is reported with
the smallest and the largest.  Per shape and `every`, all bins, hold = min, decay = exp(-1 / 1000), state on the device:

    hold          sdft_hip_sdft_smooth_peak_n at `every`, first = 0
    peak          (a) sdft_hip_sdft_power_peak_n on the same grid: the peer, one pass of the same recurrence; its spread,
                  (max - min) / median, is the run-to-run spread the comparison is read against
    dense + amin  (b) sdft_hip_sdft_power_smooth_n at every = 1 into nsamples x nbins numbers, then torch: amin over each window of
                  rows -- the only route before this call, the same statistic; the call's rows are compared with it
    sampled       (c) sdft_hip_sdft_power_smooth_n at the same `every`: cheaper, a weaker statistic (it sees one value per window)

Shapes: configs[1] (n = 1e6, m = 1024, Hann, f32f64) at every = 100 and every = n; configs[2] (n = 262 144, m = 4096, Blackman,
f32f32) at every = 256; the north star's shape (n = 48 000, m = 1024, Hann, f32f64) at every = 1."""

from __future__ import annotations

import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINES = [("configs[1]", 1_000_000, 1024, "hann", "f32f64", 100),
         ("configs[1]", 1_000_000, 1024, "hann", "f32f64", 1_000_000),
         ("configs[2]", 262_144, 4096, "blackman", "f32f32", 256),
         ("north star", 48_000, 1024, "hann", "f32f64", 1)]
DECAY = math.exp(-1.0 / 1000.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_peak_rates.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--once", type=int, default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from sdft_amd.sdft import SDFT, every_rows, power_sum_rows
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
            out = torch.empty((power_sum_rows(n, every, 0), m), dtype=rdt, device="cuda")
            state = torch.zeros(m, dtype=rdt, device="cuda")
            for _ in range(3):
                p.smooth_peak(x, DECAY, every, 0, hold="min", state=state, out=out)
            torch.cuda.synchronize()
            print(f"once: {name} n={n} m={m} {combo} every={every} chunks {p.get_option('last_chunks')} x {p.get_option('last_chunk_len')}")
        return

    log(f"# smooth_peak_rates.py  {time.strftime('%Y-%m-%d %H:%M:%S')}  device {torch.cuda.get_device_name(0)}  reps {reps} (median), 3 warm-up calls per route")
    log("# ms per call of n samples, all bins, hold = min; / x = hold ms / x ms; spread = (max - min) / median of peak")
    for name, n, m, window, combo, every in LINES:
        rdt = torch.float64 if combo.endswith("f64") else torch.float32
        u = 2.0 ** (-53 if combo.endswith("f64") else -24)
        x = samples(n, m)
        with SDFT(m, window, 1.0, combo) as p:
            p.set_option("pipeline", 0)
            rows = power_sum_rows(n, every, 0)
            hold_out = torch.empty((rows, m), dtype=rdt, device="cuda")
            other_out = torch.empty((rows, m), dtype=rdt, device="cuda")       # the peak-hold and the sampled call's rows, in turn
            dense = torch.empty((n, m), dtype=rdt, device="cuda")
            state = torch.zeros(m, dtype=rdt, device="cuda")
            whole = n // every                                                  # windows of `every` samples; the last may be shorter
            amin = torch.empty((rows, m), dtype=rdt, device="cuda")

            def hold():
                state.zero_()
                p.smooth_peak(x, DECAY, every, 0, hold="min", state=state, out=hold_out)

            def peak():
                p.power_peak(x, every, 0, hold="min", out=other_out)

            def dense_amin():
                state.zero_()
                p.power_smooth(x, DECAY, 1, 0, state=state, out=dense)
                if every > 1:
                    torch.amin(dense[:whole * every].view(whole, every, m), dim=1, out=amin[:whole])
                    if whole < rows:
                        torch.amin(dense[whole * every:], dim=0, out=amin[whole])

            def sampled():
                state.zero_()
                p.power_smooth(x, DECAY, every, 0, state=state, out=other_out[:every_rows(n, every, 0)])

            routes = [("hold", hold), ("peak", peak), ("dense + amin", dense_amin), ("sampled", sampled)]
            for _ in range(3):
                for _, fn in routes:
                    p.reset()
                    fn()
            geo = None
            ts = {k: [] for k, _ in routes}
            for _ in range(reps):
                for k, fn in routes:
                    ts[k].append(timed(p, fn))
                    if k == "hold":
                        geo = (p.get_option("last_kernel"), p.get_option("last_chunks"), p.get_option("last_chunk_len"), p.get_option("last_chain"))
            p.reset(); hold(); p.reset(); dense_amin(); torch.cuda.synchronize()
            scale = float(dense.max()) * u / (1.0 - DECAY)
            worst = float((hold_out - (amin if every > 1 else dense)).abs().max()) / scale     # (windows of one sample: the dense rows themselves)
            mh, mp, md, mc = stat(ts["hold"]), stat(ts["peak"]), stat(ts["dense + amin"]), stat(ts["sampled"])
            spread = (mp[2] - mp[1]) / mp[0]
            log(f"{name} n={n} m={m} {window} {combo} every={every} rows={rows}: kernel {geo[0]} chunks {geo[1]} x {geo[2]} chain {geo[3]}; "
                f"largest |hold - (dense + amin)| = {worst:.2f} u smax / (1 - a)")
            log(f"  hold          {mh[0]:.3f} ms  [min {mh[1]:.3f} max {mh[2]:.3f}]  / peak {mh[0] / mp[0]:.3f}  / dense + amin {mh[0] / md[0]:.3f}  / sampled {mh[0] / mc[0]:.3f}")
            log(f"  peak          {mp[0]:.3f} ms  [min {mp[1]:.3f} max {mp[2]:.3f}]  spread {spread:.3f}")
            log(f"  dense + amin  {md[0]:.3f} ms  [min {md[1]:.3f} max {md[2]:.3f}]  / hold {md[0] / mh[0]:.2f}")
            log(f"  sampled       {mc[0]:.3f} ms  [min {mc[1]:.3f} max {mc[2]:.3f}]")
            del hold_out, other_out, dense, amin
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
