"""Rates of the power-spectrogram analysis (sdft_hip_sdft_power_n) against what a host does without it, in the same process,
on one MI355X.

    python scripts/power_rates.py [--out profiles/power_rates.txt] [--reps 7]
    rocprofv3 --kernel-trace --stats -d <dir> -o power -- python scripts/power_rates.py --once     (a run of its own, no counters)

Device pointers, plain allocations, one plan per shape, warm-up calls first, every route timed by a pair of HIP events on the
plan's stream; the routes alternate within each repeat (so drift hits all alike); the median of the repeats is reported.
Per shape and grid:

    sdft_n        sdft_sdft_n alone (the complex matrix, all rows)
    two-pass      sdft_sdft_n, then re*re + im*im over the whole matrix into a real tensor with torch on the same stream
                  (torch.mul(re, re, out=pw); pw.addcmul_(im, im): two kernels, no temporaries) -- what a host that wants the
                  spectrogram does without the call, whatever rows and bins it looks at afterwards
    power         sdft_hip_sdft_power_n on the grid and the band

Shapes: configs[1] (n = 1e6, m = 1024, Hann, f32f64) at every = 1, 16, 100, band all and (0, 256); configs[2] (n = 262 144,
m = 4096, Blackman, f32f32) at every = 1, 256.  Every line is checked: the call's output against re*re + im*im (unfused, as
numpy evaluates it) of sdft_sdft_n's matrix of the same samples on the grid and the band -- bit-identical for FD float, within
2.1e-11 of the largest power for FD double (the bar of tests/test_gpu_power.py); the deviation is printed.  Then the chunk
length of forward_power_kernel for configs[1] at every = 1, 16, 100 (option "chunk"), to check the library's own choice."""

from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BAR = 2.1e-11


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "power_rates.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--once", action="store_true", help="one warm-up and one timed call per route, no chunk sweep, no file (for a trace run)")
    args = ap.parse_args()
    import numpy as np
    import torch
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

    def deviation(got, full, every, band, bitwise, step=1 << 16):
        """largest |got - (re*re + im*im)| over the grid's rows of `full` and the band, relative to the largest power"""
        worst, top, equal = 0.0, 0.0, True
        rows = full[::every]
        for r in range(0, rows.shape[0], step):
            d = rows[r:r + step, band[0]:band[0] + band[1]]
            re, im = d.real, d.imag
            want = re * re + im * im
            g = got[r:r + step]
            equal = equal and bool(torch.equal(g, want))
            worst = max(worst, float((g - want).abs().max()))
            top = max(top, float(want.max()))
        dev = worst / top if top > 0 else 0.0
        assert (equal if bitwise else dev <= BAR), (dev, equal)
        return dev, equal

    log(f"# power_rates.py  {time.strftime('%Y-%m-%d %H:%M:%S')}  device {torch.cuda.get_device_name(0)}  reps {reps} (median)")
    log("# ms per call of n samples; x sdft_n = sdft_sdft_n ms / power ms; x two-pass = (sdft_sdft_n + torch re*re + im*im) ms / power ms")
    log("# dev = largest deviation from re*re + im*im of sdft_sdft_n's matrix, relative to the largest power (bit-identical: =)")
    shapes = [("configs[1]", 1_000_000, 1024, "hann", "f32f64", (1, 16, 100), [None, (0, 256)]),
              ("configs[2]", 262_144, 4096, "blackman", "f32f32", (1, 256), [None])]
    for name, n, m, window, combo, everys, bands in shapes:
        x = torch.from_numpy(sine_sweep(n) + noise(n, seed=m) * np.float32(0.25)).cuda()
        bitwise = combo.endswith("f32")
        with SDFT(m, window, 1.0, combo) as p:
            cdt, rdt = (torch.complex128, torch.float64) if combo.endswith("f64") else (torch.complex64, torch.float32)
            full = torch.empty((n, m), dtype=cdt, device="cuda")
            pw = torch.empty((n, m), dtype=rdt, device="cuda")
            re, im = full.real, full.imag

            def two_pass():
                p.sdft(x, out=full)
                torch.mul(re, re, out=pw)
                pw.addcmul_(im, im)

            cases = [(e, b if b else (0, m)) for e in everys for b in bands]
            outs = {c: torch.empty((every_rows(n, c[0], 0), c[1][1]), dtype=rdt, device="cuda") for c in cases}
            p.set_option("pipeline", 0)
            # correctness first (it is the warm-up too): the same samples from the same state through both routes
            devs = {}
            for c in cases:
                p.reset()
                p.sdft(x, out=full)
                p.reset()
                p.power(x, c[0], 0, bins=c[1], out=outs[c])
                devs[c] = deviation(outs[c], full, c[0], c[1], bitwise)
            two_pass()
            t_full, t_two, t_pow, geo = [], [], {c: [] for c in cases}, {}
            for _ in range(reps):
                t_full.append(timed(p, lambda: p.sdft(x, out=full)))
                t_two.append(timed(p, two_pass))
                for c in cases:
                    t_pow[c].append(timed(p, lambda: p.power(x, c[0], 0, bins=c[1], out=outs[c])))
                    geo[c] = (p.get_option("last_kernel"), p.get_option("last_chunks"), p.get_option("last_chunk_len"), p.get_option("last_chain"))
            mf, mt = float(np.median(t_full)), float(np.median(t_two))
            log(f"{name} n={n} m={m} {window} {combo}: sdft_n {mf:.3f} ms  two-pass {mt:.3f} ms  [two-pass min {min(t_two):.3f} max {max(t_two):.3f}]")
            for c in cases:
                mp = float(np.median(t_pow[c]))
                g = geo[c]
                dev, equal = devs[c]
                log(f"  every={c[0]:4d} band=({c[1][0]},{c[1][1]:4d}) rows={every_rows(n, c[0], 0):7d}: power {mp:.3f} ms  x sdft_n {mf / mp:.2f}  x two-pass {mt / mp:.2f}"
                    f"  kernel {g[0]} chunks {g[1]} x {g[2]} chain {g[3]}  dev {'=' if equal else f'{dev:.2e}'}  [min {min(t_pow[c]):.3f} max {max(t_pow[c]):.3f}]")
            del full, pw, re, im, outs
            torch.cuda.empty_cache()
    if not args.once:
        n, m = 1_000_000, 1024
        x = torch.from_numpy(sine_sweep(n)).cuda()
        log("# configs[1], band all: chunk length of forward_power_kernel (option chunk; 0 = the library's choice)")
        with SDFT(m, "hann", 1.0, "f32f64") as p:
            for every in (1, 16, 100):
                out = torch.empty((every_rows(n, every, 0), m), dtype=torch.float64, device="cuda")
                for chunk in (0, 256, 512, 1024, 2048, 4632, 9264):
                    p.set_option("chunk", chunk)
                    p.power(x, every, 0, out=out)
                    ts = [timed(p, lambda: p.power(x, every, 0, out=out)) for _ in range(reps)]
                    log(f"  every={every:4d} chunk={chunk:6d} ({p.get_option('last_chunks')} chunks of {p.get_option('last_chunk_len')}): {float(np.median(ts)):.3f} ms")
                del out
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
