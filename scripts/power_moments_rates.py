"""Rates of the power-moments analysis (sdft_hip_sdft_power_moments_n) against the pooled power call on the same grid and against
what a host does without it, in the same process, on one MI355X.

    python scripts/power_moments_rates.py [--out profiles/power_moments_rates.txt] [--reps 5]

Device pointers, plain allocations, one plan per shape, warm-up calls first, every route timed by a pair of HIP events on the
plan's stream; the routes alternate within each repeat (so drift hits all alike); the median of the repeats is reported with
the smallest and the largest.  Per shape and `every`, all bins:

    moments       sdft_hip_sdft_power_moments_n at `every`, first = 0
    pooled        (a) sdft_hip_sdft_power_sum_n on the same grid: the same recurrence with half the stores and one accumulator, so
                  the floor; its spread, (max - min) / median, is the run-to-run spread the comparison is read against
    two-pass      (b) sdft_hip_sdft_power_n at every = 1, then torch on the same stream: the [n][m] powers reshaped to
                  [rows][every][m] and summed over the middle axis, then squared into a second [n][m] buffer and summed likewise
                  (every divides the samples used; the ragged last window is left to the host)

Shapes: configs[1] (n = 1e6, m = 1024, Hann, f32f64) at every = 100 and every = n; configs[2] (n = 262 144, m = 4096, Blackman,
f32f32) at every = 256.  Every moments line is checked against (a), whose bits [..., 0] must have (the count of elements that
differ is printed and has to be 0), and against (b), which holds the same terms (both calls cut time alike) summed in another
order: with L the window's length and gamma_L = L u / (1 - L u) each side lies within gamma_L of the exact sum of non-negative
terms, so |call - two-pass| <= 2 gamma_L * two-pass; the largest |call - two-pass| / (gamma_L * two-pass) is printed per component
and has to stay below 2."""

from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "power_moments_rates.txt"))
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

    log(f"# power_moments_rates.py  {time.strftime('%Y-%m-%d %H:%M:%S')}  device {torch.cuda.get_device_name(0)}  reps {reps} (median), 3 warm-up calls per route")
    log("# ms per call of n samples, all bins; / pooled = ms / pooled ms; two-pass / moments = two-pass ms / moments ms; spread = (max - min) / median of pooled")
    log("# differ = elements of moments[..., 0] whose bits are not the pooled call's; gamma s1, s2 = largest |call - two-pass| / (gamma_L * two-pass), bound 2")
    shapes = [("configs[1]", 1_000_000, 1024, "hann", "f32f64", (100, 1_000_000)),
              ("configs[2]", 262_144, 4096, "blackman", "f32f32", (256,))]
    for name, n, m, window, combo, everies in shapes:
        x = torch.from_numpy(sine_sweep(n) + noise(n, seed=m) * np.float32(0.25)).cuda()
        rdt = torch.float64 if combo.endswith("f64") else torch.float32
        u = 2.0 ** -53 if combo.endswith("f64") else 2.0 ** -24
        with SDFT(m, window, 1.0, combo) as p:
            p.set_option("pipeline", 0)
            dense_out = torch.empty((n, m), dtype=rdt, device="cuda")
            dense_sq = torch.empty((n, m), dtype=rdt, device="cuda")
            for every in everies:
                rows = power_sum_rows(n, every, 0)
                whole = n // every                                     # windows the torch pass can reshape
                mom_out = torch.empty((rows, m, 2), dtype=rdt, device="cuda")
                pooled_out = torch.empty((rows, m), dtype=rdt, device="cuda")
                second1 = torch.empty((whole, m), dtype=rdt, device="cuda")
                second2 = torch.empty((whole, m), dtype=rdt, device="cuda")

                def moments():
                    p.power_moments(x, every, 0, out=mom_out)

                def pooled():
                    p.power_sum(x, every, 0, out=pooled_out)

                def two_pass():
                    p.power(x, 1, 0, out=dense_out)
                    torch.sum(dense_out[:whole * every].view(whole, every, m), dim=1, out=second1)
                    torch.mul(dense_out, dense_out, out=dense_sq)
                    torch.sum(dense_sq[:whole * every].view(whole, every, m), dim=1, out=second2)

                routes = [("moments", moments), ("pooled", pooled), ("two-pass", two_pass)]
                for _ in range(3):
                    for _, fn in routes:
                        p.reset()
                        fn()
                geo = None
                ts = {k: [] for k, _ in routes}
                for _ in range(reps):
                    for k, fn in routes:
                        ts[k].append(timed(p, fn))
                        if k == "moments":
                            geo = (p.get_option("last_kernel"), p.get_option("last_chunks"), p.get_option("last_chunk_len"), p.get_option("last_chain"))
                        if k == "pooled":
                            assert geo[1:3] == (p.get_option("last_chunks"), p.get_option("last_chunk_len")), "the pooled call cut time differently"
                # the same samples from the same state through the three routes
                p.reset(); moments(); p.reset(); pooled(); p.reset(); two_pass(); torch.cuda.synchronize()
                differ = int((mom_out[..., 0] != pooled_out).sum())
                L = float(every)
                gamma = L * u / (1.0 - L * u)
                worst = []
                for comp, second in ((0, second1), (1, second2)):
                    got = mom_out[:whole, :, comp].to(torch.float64)
                    want = second.to(torch.float64)
                    worst.append(float(((got - want).abs() / (gamma * want).clamp_min(1e-300)).max()))
                mm, mp, mt = stat(ts["moments"]), stat(ts["pooled"]), stat(ts["two-pass"])
                spread = (mp[2] - mp[1]) / mp[0]
                log(f"{name} n={n} m={m} {window} {combo} every={every} rows={rows}: kernel {geo[0]} chunks {geo[1]} x {geo[2]} chain {geo[3]}  differ {differ}  "
                    f"gamma s1 {worst[0]:.3f} s2 {worst[1]:.3f}")
                log(f"  moments  {mm[0]:.3f} ms  [min {mm[1]:.3f} max {mm[2]:.3f}]  / pooled {mm[0] / mp[0]:.3f}")
                log(f"  pooled   {mp[0]:.3f} ms  [min {mp[1]:.3f} max {mp[2]:.3f}]  spread {spread:.3f}")
                log(f"  two-pass {mt[0]:.3f} ms  [min {mt[1]:.3f} max {mt[2]:.3f}]  two-pass / moments {mt[0] / mm[0]:.2f}")
                del mom_out, pooled_out, second1, second2
            del dense_out, dense_sq
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
