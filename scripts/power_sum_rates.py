"""Rates of the pooled power analysis (sdft_hip_sdft_power_sum_n) against what a host does without it, in the same process, on
one MI355X.

    python scripts/power_sum_rates.py [--out profiles/power_sum_rates.txt] [--reps 20]
    rocprofv3 --kernel-trace --stats -d <dir> -o power_sum -- python scripts/power_sum_rates.py --once   (a run of its own, no counters)

Device pointers, plain allocations, one plan per shape, warm-up calls first, every route timed by a pair of HIP events on the
plan's stream; the routes alternate within each repeat (so drift hits all alike); the median of the repeats is reported with
the smallest and the largest, and the spread of the dense power call -- (max - min) / median -- is the run-to-run spread the
comparison is read against.  Per shape and `every`, all bins:

    pooled        sdft_hip_sdft_power_sum_n at `every`, first = 0
    dense         sdft_hip_sdft_power_n at every = 1 alone (the [n][m] powers reach memory)
    two-pass      sdft_hip_sdft_power_n at every = 1, then torch: the [n][m] powers reshaped to [rows][every][m] and summed over
                  the middle axis on the same stream (every divides the samples used; the ragged last window is left to the host)
    sampled       sdft_hip_sdft_power_n at the same `every`: one row in `every`, no averaging -- the fast preview

Shapes: configs[1] (n = 1e6, m = 1024, Hann, f32f64) at every = 100 and every = n; configs[2] (n = 262 144, m = 4096, Blackman,
f32f32) at every = 256 and every = n.  Every pooled line is checked against the two-pass result: the relative deviation, element
by element, is printed (the two add a window's terms in different orders; both obey gamma_L).  Then the chunk length of
forward_pooled_power_kernel for configs[1] (option "chunk"), to check the library's own choice."""

from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "power_sum_rates.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--once", action="store_true", help="one warm-up and one timed pooled call per shape, no file (for a trace run)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from sdft_amd.sdft import SDFT, every_rows, power_sum_rows
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

    log(f"# power_sum_rates.py  {time.strftime('%Y-%m-%d %H:%M:%S')}  device {torch.cuda.get_device_name(0)}  reps {reps} (median), 3 warm-up calls per route")
    log("# ms per call of n samples, all bins; x dense = dense ms / pooled ms; x two-pass = two-pass ms / pooled ms; spread = (max - min) / median of dense")
    log("# dev = largest |pooled - two-pass| / two-pass over all elements")
    shapes = [("configs[1]", 1_000_000, 1024, "hann", "f32f64", 100),
              ("configs[2]", 262_144, 4096, "blackman", "f32f32", 256)]
    for name, n, m, window, combo, every_short in shapes:
        x = torch.from_numpy(sine_sweep(n) + noise(n, seed=m) * np.float32(0.25)).cuda()
        rdt = torch.float64 if combo.endswith("f64") else torch.float32
        with SDFT(m, window, 1.0, combo) as p:
            p.set_option("pipeline", 0)
            dense_out = torch.empty((n, m), dtype=rdt, device="cuda")
            for every in (every_short, n):
                rows = power_sum_rows(n, every, 0)
                whole = n // every                                     # windows the torch pass can reshape
                pooled_out = torch.empty((rows, m), dtype=rdt, device="cuda")
                second = torch.empty((whole, m), dtype=rdt, device="cuda")
                sampled_out = torch.empty((every_rows(n, every, 0), m), dtype=rdt, device="cuda")

                def pooled():
                    p.power_sum(x, every, 0, out=pooled_out)

                def dense():
                    p.power(x, 1, 0, out=dense_out)

                def two_pass():
                    p.power(x, 1, 0, out=dense_out)
                    torch.sum(dense_out[:whole * every].view(whole, every, m), dim=1, out=second)

                def sampled():
                    p.power(x, every, 0, out=sampled_out)

                routes = [("pooled", pooled), ("dense", dense), ("two-pass", two_pass), ("sampled", sampled)]
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
                        if k == "pooled":
                            geo = (p.get_option("last_kernel"), p.get_option("last_chunks"), p.get_option("last_chunk_len"), p.get_option("last_chain"))
                if args.once:
                    log(f"{name} every={every}: pooled {ts['pooled'][0]:.3f} ms  kernel {geo[0]} chunks {geo[1]} x {geo[2]}")
                    continue
                # the same samples from the same state through both routes
                p.reset(); pooled(); p.reset(); two_pass(); torch.cuda.synchronize()
                dev = float(((pooled_out[:whole] - second).abs() / second).max())
                mp, md, mt, ms = stat(ts["pooled"]), stat(ts["dense"]), stat(ts["two-pass"]), stat(ts["sampled"])
                spread = (md[2] - md[1]) / md[0]
                log(f"{name} n={n} m={m} {window} {combo} every={every} rows={rows}: kernel {geo[0]} chunks {geo[1]} x {geo[2]} chain {geo[3]}  dev {dev:.2e}")
                log(f"  pooled   {mp[0]:.3f} ms  [min {mp[1]:.3f} max {mp[2]:.3f}]")
                log(f"  dense    {md[0]:.3f} ms  [min {md[1]:.3f} max {md[2]:.3f}]  x dense {md[0] / mp[0]:.2f}  spread {spread:.3f}")
                log(f"  two-pass {mt[0]:.3f} ms  [min {mt[1]:.3f} max {mt[2]:.3f}]  x two-pass {mt[0] / mp[0]:.2f}")
                log(f"  sampled  {ms[0]:.3f} ms  [min {ms[1]:.3f} max {ms[2]:.3f}]")
                del pooled_out, second, sampled_out
            del dense_out
            torch.cuda.empty_cache()
    if not args.once:
        n, m = 1_000_000, 1024
        x = torch.from_numpy(sine_sweep(n)).cuda()
        log("# configs[1], all bins: chunk length of forward_pooled_power_kernel (option chunk; 0 = the library's choice)")
        with SDFT(m, "hann", 1.0, "f32f64") as p:
            for every in (100, n):
                out = torch.empty((power_sum_rows(n, every, 0), m), dtype=torch.float64, device="cuda")
                for chunk in (0, 256, 512, 1024, 2048, 4632, 9264):
                    p.set_option("chunk", chunk)
                    for _ in range(3):
                        p.power_sum(x, every, 0, out=out)
                    ts = [timed(p, lambda: p.power_sum(x, every, 0, out=out)) for _ in range(reps)]
                    log(f"  every={every:7d} chunk={chunk:6d} ({p.get_option('last_chunks')} chunks of {p.get_option('last_chunk_len')}): {float(np.median(ts)):.3f} ms")
                del out
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
