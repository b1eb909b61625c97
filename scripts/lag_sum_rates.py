"""Rates of the lag-product analysis (sdft_hip_sdft_lag_sum_n) against the pooled power call on the same grid and against the two
ways a host reaches the same sums without it, in the same process, on one MI355X.

    python scripts/lag_sum_rates.py [--out profiles/lag_sum_rates.txt] [--reps 5] [--shapes 1,2]

Device pointers, plain allocations, one plan per route and shape, warm-up calls first, every route timed by a pair of HIP events on
the plan's stream; the routes alternate within each repeat (so drift hits all alike); the median of the repeats is reported with
the smallest and the largest.  Per shape and `every`, all bins, first = 0:

    lag           sdft_hip_sdft_lag_sum_n at `every`
    pooled        (a) sdft_hip_sdft_power_sum_n on the same grid: the same recurrence with half the stored bytes, so the floor; its
                  spread, (max - min) / median, is the run-to-run spread the comparison is read against
    cross         (b) sdft_hip_sdft_cross_sum_n on a two-channel plan whose second channel is the signal delayed by one sample, pair
                  (0, 1): the only one-pass route without the call; two recurrences, twice the samples
    two-pass      (c) sdft_sdft_n, then torch: rows[1:] * conj(rows[:-1]) and a reshape-and-sum over the windows on the same stream
                  (every divides the samples used; the ragged last window is left to the host)

Shapes: configs[1] (n = 1e6, m = 1024, Hann, f32f64) at every = 100 and every = n; configs[2] (n = 262 144, m = 4096, Blackman,
f32f32) at every = 256.  Every lag line is compared with the cross and the two-pass result: the largest deviation relative to the
largest |sum| is printed (the three routes start their chunks from different carries, so FD double differs in the last digits)."""

from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lag_sum_rates.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="1,2", help="which of configs[1], configs[2] to run")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
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

    def worst(a, b):
        scale = float(b.abs().max())
        return float((a - b).abs().max()) / (scale if scale > 0 else 1.0)

    if not args.append:
        log(f"# lag_sum_rates.py  {time.strftime('%Y-%m-%d %H:%M:%S')}  device {torch.cuda.get_device_name(0)}  reps {reps} (median), 3 warm-up calls per route")
        log("# ms per call of n samples, all bins, first = 0; / pooled = ms / pooled ms; x / lag = that route's ms / lag ms; spread = (max - min) / median of pooled")
        log("# deviates = largest |lag - route| over the whole windows, relative to the largest |sum|")
    shapes = [("configs[1]", 1_000_000, 1024, "hann", "f32f64", (100, 1_000_000)),
              ("configs[2]", 262_144, 4096, "blackman", "f32f32", (256,))]
    wanted = {int(s) for s in args.shapes.split(",") if s}
    for idx, (name, n, m, window, combo, everies) in enumerate(shapes, start=1):
        if idx not in wanted:
            continue
        xh = sine_sweep(n) + noise(n, seed=m) * np.float32(0.25)
        x = torch.from_numpy(xh).cuda()
        delayed = np.concatenate([np.zeros(1, dtype=xh.dtype), xh[:-1]])
        x2 = torch.from_numpy(np.stack([xh, delayed])).cuda()
        cdt = torch.complex128 if combo.endswith("f64") else torch.complex64
        rdt = torch.float64 if combo.endswith("f64") else torch.float32
        with SDFT(m, window, 1.0, combo) as p, SDFT(m, window, 1.0, combo, 2) as p2:
            p.set_option("pipeline", 0)
            p2.set_option("pipeline", 0)
            p2.set_pairs([0], [1])
            dense = torch.empty((n, m), dtype=cdt, device="cuda")
            prod = torch.zeros((n, m), dtype=cdt, device="cuda")       # (row 0 stays zero: the row before it is the zero row)
            for every in everies:
                rows = power_sum_rows(n, every, 0)
                whole = n // every                                     # windows the torch pass can reshape
                lag_out = torch.empty((rows, m), dtype=cdt, device="cuda")
                pooled_out = torch.empty((rows, m), dtype=rdt, device="cuda")
                cross_out = torch.empty((1, rows, m), dtype=cdt, device="cuda")
                second = torch.empty((whole, m), dtype=cdt, device="cuda")

                def lag():
                    p.lag_sum(x, every, 0, out=lag_out)

                def pooled():
                    p.power_sum(x, every, 0, out=pooled_out)

                def cross():
                    p2.cross_sum(x2, every, 0, out=cross_out)

                def two_pass():
                    p.sdft(x, out=dense)
                    torch.mul(dense[1:], dense[:-1].conj(), out=prod[1:])
                    torch.sum(prod[:whole * every].view(whole, every, m), dim=1, out=second)

                routes = [("lag", p, lag), ("pooled", p, pooled), ("cross", p2, cross), ("two-pass", p, two_pass)]
                for _ in range(3):
                    for _, q, fn in routes:
                        q.reset()
                        fn()
                geo = None
                ts = {k: [] for k, _, _ in routes}
                for _ in range(reps):
                    for k, q, fn in routes:
                        ts[k].append(timed(q, fn))
                        if k == "lag":
                            geo = (p.get_option("last_kernel"), p.get_option("last_chunks"), p.get_option("last_chunk_len"), p.get_option("last_chain"))
                # the same samples from the same state through the three routes
                p.reset(); lag(); p2.reset(); cross(); p.reset(); two_pass(); torch.cuda.synchronize()
                dev_cross, dev_two = worst(cross_out[0], lag_out), worst(second, lag_out[:whole])
                ml, mp, mc, mt = stat(ts["lag"]), stat(ts["pooled"]), stat(ts["cross"]), stat(ts["two-pass"])
                spread = (mp[2] - mp[1]) / mp[0]
                log(f"{name} n={n} m={m} {window} {combo} every={every} rows={rows}: kernel {geo[0]} chunks {geo[1]} x {geo[2]} chain {geo[3]}  deviates cross {dev_cross:.1e} two-pass {dev_two:.1e}")
                log(f"  lag      {ml[0]:.3f} ms  [min {ml[1]:.3f} max {ml[2]:.3f}]  / pooled {ml[0] / mp[0]:.3f}")
                log(f"  pooled   {mp[0]:.3f} ms  [min {mp[1]:.3f} max {mp[2]:.3f}]  spread {spread:.3f}")
                log(f"  cross    {mc[0]:.3f} ms  [min {mc[1]:.3f} max {mc[2]:.3f}]  cross / lag {mc[0] / ml[0]:.2f}")
                log(f"  two-pass {mt[0]:.3f} ms  [min {mt[1]:.3f} max {mt[2]:.3f}]  two-pass / lag {mt[0] / ml[0]:.2f}")
                del lag_out, pooled_out, cross_out, second
            del dense, prod
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a" if args.append else "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
