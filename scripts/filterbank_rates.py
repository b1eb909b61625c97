"""Rates of the filterbank analysis (sdft_hip_sdft_filterbank_n) against what a host does without it, in the same process, on one
MI355X.

    python scripts/filterbank_rates.py [--out FILE] [--reps 20]
    rocprofv3 --kernel-trace --stats -d <dir> -o filterbank -- python scripts/filterbank_rates.py --once   (a run of its own, no counters)

Device pointers, plain allocations, one plan per shape, warm-up calls first, every route timed by a pair of HIP events on the
plan's stream; the routes alternate within each repeat (so drift hits all alike); the median of the repeats is reported with the
smallest and the largest, and the spread of each side -- (max - min) / median -- is the run-to-run spread the comparison is read
against.  Per shape and `every`, a mel filterbank on all bins:

    filterbank    sdft_hip_sdft_filterbank_n at `every`, first = 0: [rows][nbands] reach memory
    power         sdft_hip_sdft_power_n alone on the same grid: [rows][m] reach memory
    two-pass      that call, then torch: its [rows][m] output times the dense [m][nbands] band matrix on the same stream

Shapes: configs[1] (n = 1e6, m = 1024, Hann, f32f64) with 80 mel bands at every = 1, 100, 160; configs[2] (n = 262 144, m = 4096,
Blackman, f32f32) with 128 mel bands at every = 1, 256.  Every filterbank line is checked against the two-pass result: the largest
deviation relative to the largest band sum is printed (the two add a band's terms in different orders)."""

from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filterbank_rates.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--once", action="store_true", help="one warm-up and one timed filterbank call per shape and grid, no file (for a trace run)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from sdft_amd import filterbank as F
    from sdft_amd.sdft import SDFT, every_rows
    from sdft_amd.signals import noise, sine_sweep

    torch.cuda.set_device(0)
    reps = 1 if args.once else args.reps
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

    def spread(s):
        return (s[2] - s[1]) / s[0]

    log(f"# filterbank_rates.py  {time.strftime('%Y-%m-%d %H:%M:%S')}  device {torch.cuda.get_device_name(0)}  reps {reps} (median), 3 warm-up calls per route")
    log("# ms per call of n samples; x power = power ms / filterbank ms; x two-pass = two-pass ms / filterbank ms; spread = (max - min) / median of the side")
    log("# dev = largest |filterbank - two-pass| / largest two-pass value over all elements")
    shapes = [("configs[1]", 1_000_000, 1024, "hann", "f32f64", 80, (1, 100, 160)),
              ("configs[2]", 262_144, 4096, "blackman", "f32f32", 128, (1, 256))]
    for name, n, m, window, combo, nbands, everies in shapes:
        x = torch.from_numpy(sine_sweep(n) + noise(n, seed=m) * np.float32(0.25)).cuda()
        rdt = torch.float64 if combo.endswith("f64") else torch.float32
        bank = F.mel(m, 48000, nbands)
        W = torch.from_numpy(F.dense(m, *bank)).to(rdt).cuda().T.contiguous()          # [m][nbands]
        with SDFT(m, window, 1.0, combo) as p:
            p.set_option("pipeline", 0)
            p.set_filterbank(*bank)
            nb = p.filterbank_bands
            for every in everies:
                rows = every_rows(n, every, 0)
                fb_out = torch.empty((rows, nb), dtype=rdt, device="cuda")
                power_out = torch.empty((rows, m), dtype=rdt, device="cuda")
                second = torch.empty((rows, nb), dtype=rdt, device="cuda")

                def filterbank():
                    p.filterbank(x, every, 0, out=fb_out)

                def power():
                    p.power(x, every, 0, out=power_out)

                def two_pass():
                    p.power(x, every, 0, out=power_out)
                    torch.matmul(power_out, W, out=second)

                routes = [("filterbank", filterbank), ("power", power), ("two-pass", two_pass)]
                if args.once:
                    routes = routes[:1]
                for _ in range(1 if args.once else 3):
                    for _, fn in routes:
                        p.reset()
                        fn()
                geo = None
                ts = {k: [] for k, _ in routes}
                for _ in range(reps):
                    for k, fn in routes:
                        ts[k].append(timed(p, fn))
                        if k == "filterbank":
                            geo = (p.get_option("last_kernel"), p.get_option("last_chunks"), p.get_option("last_chunk_len"), p.get_option("last_chain"))
                if args.once:
                    log(f"{name} every={every}: filterbank {ts['filterbank'][0]:.3f} ms  kernel {geo[0]} chunks {geo[1]} x {geo[2]}")
                    continue
                # the same samples from the same state through both routes
                p.reset(); filterbank(); p.reset(); two_pass(); torch.cuda.synchronize()
                dev = float((fb_out - second).abs().max() / second.abs().max())
                mf, mp, mt = stat(ts["filterbank"]), stat(ts["power"]), stat(ts["two-pass"])
                log(f"{name} n={n} m={m} {window} {combo} bands={nb} every={every} rows={rows}: kernel {geo[0]} chunks {geo[1]} x {geo[2]} chain {geo[3]}  dev {dev:.2e}")
                log(f"  filterbank {mf[0]:.3f} ms  [min {mf[1]:.3f} max {mf[2]:.3f}]  spread {spread(mf):.3f}")
                log(f"  power      {mp[0]:.3f} ms  [min {mp[1]:.3f} max {mp[2]:.3f}]  spread {spread(mp):.3f}  x power {mp[0] / mf[0]:.2f}")
                log(f"  two-pass   {mt[0]:.3f} ms  [min {mt[1]:.3f} max {mt[2]:.3f}]  spread {spread(mt):.3f}  x two-pass {mt[0] / mf[0]:.2f}")
                del fb_out, power_out, second
            torch.cuda.empty_cache()
    if not args.once and args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
