"""Rates of the pooled cross-spectrum analysis (sdft_hip_sdft_cross_sum_n) against what a host does without it, in the same
process, on one MI355X.

    python scripts/cross_sum_rates.py [--out profiles/cross_sum_rates.txt] [--reps 20]
    rocprofv3 --kernel-trace --stats -d <dir> -o cross_sum -- python scripts/cross_sum_rates.py --once   (a run of its own, no counters)

Device pointers, plain allocations, one plan, warm-up calls first, every route timed by a pair of HIP events on the plan's
stream; the routes alternate within each repeat (so drift hits all alike); the median of the repeats is reported with the
smallest and the largest, and the spread of the pooled power call -- (max - min) / median -- is the run-to-run spread the
comparison is read against.

The shape is one GPU's share of configs[4]: 64 channels x 48000 samples, m = 1024, Hann, f32f64, all bins, with the 32 disjoint
pairs (0, 1), (2, 3), ... (62, 63).  Per `every`:

    cross         sdft_hip_sdft_cross_sum_n at `every`, first = 0: [32][rows][m] complex sums
    pooled power  sdft_hip_sdft_power_sum_n over the same 64 channels, unchanged code: the arithmetic floor -- the cross call steps
                  the same 64 recurrences and windows the same 64 x m bins, and forms four products per pair and bin where this forms
                  two per channel and bin; it delivers no cross term
    two-pass      sdft_sdft_n (the [64][n][m] complex matrix reaches memory: 16 KiB per sample and channel), then torch on the same
                  stream: X[0::2] * conj(X[1::2]) reshaped to [32][rows][every][m] and summed over the window axis (every divides the
                  samples used; the ragged last window is left to the host)

Every cross line is checked against the two-pass result: the largest deviation relative to the largest sum is printed (the two
add a window's terms in different orders and torch may fuse; both obey the window's gamma_L).

The known cost, plainly: P pairs step 2P channel recurrences (P for a == b), so the 32 disjoint pairs here are the call's best
case -- every recurrence is stepped once.  A list in which every channel is in k pairs costs k times that; an all-pairs
covariance over 64 channels is not what this kernel is for (the last block of the table prices a list of 64 and of 128 pairs)."""

from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_sum_rates.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--once", action="store_true", help="one warm-up and one timed cross call per `every`, no file (for a trace run)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from sdft_amd.sdft import SDFT, power_sum_rows
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

    log(f"# cross_sum_rates.py  {time.strftime('%Y-%m-%d %H:%M:%S')}  device {torch.cuda.get_device_name(0)}  reps {reps} (median), 3 warm-up calls per route")
    log("# ms per call of 64 channels x n samples, all bins; x floor = cross ms / pooled power ms; x two-pass = two-pass ms / cross ms;")
    log("# spread = (max - min) / median of the pooled power call; dev = largest |cross - two-pass| / largest |two-pass|")
    ch, n, m, window, combo = 64, 48000, 1024, "hann", "f32f64"
    base = sine_sweep(n)
    x = torch.from_numpy(np.stack([base + noise(n, seed=100 + c) * np.float32(0.25) for c in range(ch)]).astype(np.float32)).cuda()
    pa, pb = list(range(0, ch, 2)), list(range(1, ch, 2))
    with SDFT(m, window, 1.0, combo, ch) as p:
        p.set_option("pipeline", 0)
        p.set_pairs(pa, pb)
        matrix = None if args.once else torch.empty((ch, n, m), dtype=torch.complex128, device="cuda")
        for every in (100, 480, n):
            rows = power_sum_rows(n, every, 0)
            whole = n // every                                     # windows the torch pass can reshape
            cross_out = torch.empty((len(pa), rows, m), dtype=torch.complex128, device="cuda")
            power_out = torch.empty((ch, rows, m), dtype=torch.float64, device="cuda")

            def cross():
                p.cross_sum(x, every, 0, out=cross_out)

            def pooled_power():
                p.power_sum(x, every, 0, out=power_out)

            def two_pass():
                p.sdft(x, out=matrix)
                a = matrix[0::2, :whole * every].view(len(pa), whole, every, m)
                b = matrix[1::2, :whole * every].view(len(pa), whole, every, m)
                return torch.sum(a * b.conj(), dim=2)

            routes = [("cross", cross)] if args.once else [("cross", cross), ("pooled power", pooled_power), ("two-pass", two_pass)]
            for _ in range(1 if args.once else 3):
                for _, fn in routes:
                    p.reset()
                    fn()
            geo = None
            ts = {k: [] for k, _ in routes}
            for _ in range(reps):
                for k, fn in routes:
                    ts[k].append(timed(p, fn))
                    if k == "cross":
                        geo = (p.get_option("last_kernel"), p.get_option("last_chunks"), p.get_option("last_chunk_len"))
            if args.once:
                log(f"every={every}: cross {ts['cross'][0]:.3f} ms  kernel {geo[0]} chunks {geo[1]} x {geo[2]}")
                continue
            # the same samples from the same state through both routes
            p.reset(); cross(); p.reset(); second = two_pass(); torch.cuda.synchronize()
            dev = float((cross_out[:, :whole] - second).abs().max() / second.abs().max())
            del second
            mc, mf, mt = stat(ts["cross"]), stat(ts["pooled power"]), stat(ts["two-pass"])
            spread = (mf[2] - mf[1]) / mf[0]
            log(f"configs[4] share: {ch} x n={n} m={m} {window} {combo} 32 disjoint pairs every={every} rows={rows}: kernel {geo[0]} chunks {geo[1]} x {geo[2]}  dev {dev:.2e}")
            log(f"  cross        {mc[0]:.3f} ms  [min {mc[1]:.3f} max {mc[2]:.3f}]")
            log(f"  pooled power {mf[0]:.3f} ms  [min {mf[1]:.3f} max {mf[2]:.3f}]  x floor {mc[0] / mf[0]:.2f}  spread {spread:.3f}")
            log(f"  two-pass     {mt[0]:.3f} ms  [min {mt[1]:.3f} max {mt[2]:.3f}]  x two-pass {mt[0] / mc[0]:.2f}")
            del cross_out, power_out
        del matrix
        torch.cuda.empty_cache()
        if not args.once:
            # what a list costs in which channels repeat: every channel in 2 pairs (a ring), every channel in 4 (a ring and its second neighbours)
            log("# lists in which channels repeat, every = 480: a ring (64 pairs, 128 recurrences), a ring and its second neighbours (128 pairs, 256 recurrences)")
            every = 480
            for name, a, b in [("ring", list(range(ch)), [(c + 1) % ch for c in range(ch)]),
                               ("ring + second neighbours", list(range(ch)) * 2, [(c + 1) % ch for c in range(ch)] + [(c + 2) % ch for c in range(ch)])]:
                p.set_pairs(a, b)
                out = torch.empty((len(a), power_sum_rows(n, every, 0), m), dtype=torch.complex128, device="cuda")
                for _ in range(3):
                    p.cross_sum(x, every, 0, out=out)
                t = stat([timed(p, lambda: p.cross_sum(x, every, 0, out=out)) for _ in range(reps)])
                log(f"  {name}: {len(a)} pairs  {t[0]:.3f} ms  [min {t[1]:.3f} max {t[2]:.3f}]  chunks {p.get_option('last_chunks')} x {p.get_option('last_chunk_len')}")
                del out
    if not args.once and args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
