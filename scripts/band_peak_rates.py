"""Rates of the band-peak analysis (sdft_hip_sdft_band_peak_n) against the filterbank call on the same bank and grid and against
what a host does without it, in the same process, on one MI355X.

    python scripts/band_peak_rates.py [--out profiles/band_peak_rates.txt] [--reps 5]

Device pointers, plain allocations, one plan per shape, warm-up calls first, every route timed by a pair of HIP events on the
plan's stream; the routes alternate within each repeat (so drift hits all alike); the median of the repeats is reported with
the smallest and the largest.  Per shape, filterbank and `every`:

    peak          sdft_hip_sdft_band_peak_n at `every`, first = 0
    filterbank    (a) sdft_hip_sdft_filterbank_n on the same bank and grid: the same recurrence, strip and walk with an addition in
                  the place of the rule and half the stored numbers, so the peer; its spread, (max - min) / median, is the
                  run-to-run spread the comparison is read against
    two-pass      (b) sdft_hip_sdft_power_n on the same grid, then torch on the same stream: per band w * p[:, s:e] and its
                  max over the band (values and indices) -- the only route before

Shapes: configs[1] (n = 1e6, m = 1024, Hann, f32f64) with a 40-band mel bank and with a third-octave bank, each at every = 1 and
every = 100; configs[2] (n = 262 144, m = 4096, Blackman, f32f32) with a 40-band mel bank at every = 256.  Every peak line is
checked against (b): both calls cut time alike (the chunk counts are asserted), so the values must agree bit for bit and the bins
wherever torch's choice among equal values is the lowest bin; the counts of elements that differ are printed, and the values' has
to be 0."""

from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "band_peak_rates.txt"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    from sdft_amd import filterbank as F
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

    log(f"# band_peak_rates.py  {time.strftime('%Y-%m-%d %H:%M:%S')}  device {torch.cuda.get_device_name(0)}  reps {reps} (median), 3 warm-up calls per route")
    log("# ms per call of n samples; / filterbank = ms / filterbank ms; two-pass / peak = two-pass ms / peak ms; spread = (max - min) / median of filterbank")
    log("# differ = elements whose bits (values) or bins are not the two-pass route's")
    shapes = [("configs[1]", 1_000_000, 1024, "hann", "f32f64", [("mel40", (1, 100)), ("third-octave", (1, 100))]),
              ("configs[2]", 262_144, 4096, "blackman", "f32f32", [("mel40", (256,))])]
    for name, n, m, window, combo, banks in shapes:
        x = torch.from_numpy(sine_sweep(n) + noise(n, seed=m) * np.float32(0.25)).cuda()
        rdt = torch.float64 if combo.endswith("f64") else torch.float32
        fd = np.float64 if combo.endswith("f64") else np.float32
        with SDFT(m, window, 1.0, combo) as p:
            p.set_option("pipeline", 0)
            for bank_name, everies in banks:
                b0, nb, w = F.mel(m, 48000, 40) if bank_name == "mel40" else F.fractional_octave(m, 48000, 3)
                w = w.astype(fd)
                p.set_filterbank(b0, nb, w)
                nbands = int(b0.size)
                wd = torch.from_numpy(w).cuda()
                spans = [(int(s), int(s + k)) for s, k in zip(b0, nb)]
                offs = np.concatenate([[0], np.cumsum(nb.astype(np.int64))])
                for every in everies:
                    rows = every_rows(n, every, 0)
                    peak_out = torch.empty((rows, nbands, 2), dtype=rdt, device="cuda")
                    fb_out = torch.empty((rows, nbands), dtype=rdt, device="cuda")
                    dense_out = torch.empty((rows, m), dtype=rdt, device="cuda")
                    val2 = torch.empty((rows, nbands), dtype=rdt, device="cuda")
                    idx2 = torch.empty((rows, nbands), dtype=torch.int64, device="cuda")

                    def peak():
                        p.band_peak(x, every, 0, out=peak_out)

                    def fbank():
                        p.filterbank(x, every, 0, out=fb_out)

                    def two_pass():
                        p.power(x, every, 0, out=dense_out)
                        for b, (s, e) in enumerate(spans):
                            v, i = torch.max(wd[offs[b]:offs[b + 1]] * dense_out[:, s:e], dim=1)
                            val2[:, b] = v
                            idx2[:, b] = i + s

                    routes = [("peak", peak), ("filterbank", fbank), ("two-pass", two_pass)]
                    for _ in range(3):
                        for _, fn in routes:
                            p.reset()
                            fn()
                    geo = None
                    ts = {k: [] for k, _ in routes}
                    for _ in range(reps):
                        for k, fn in routes:
                            ts[k].append(timed(p, fn))
                            if k == "peak":
                                geo = (p.get_option("last_kernel"), p.get_option("last_chunks"), p.get_option("last_chunk_len"), p.get_option("last_band_peak_launches"))
                            else:
                                assert geo[1:3] == (p.get_option("last_chunks"), p.get_option("last_chunk_len")), f"the {k} route cut time differently"
                    # the same samples from the same state through the peak and the two-pass route
                    p.reset(); peak(); p.reset(); two_pass(); torch.cuda.synchronize()
                    iv = torch.int64 if rdt == torch.float64 else torch.int32
                    differ_v = int((peak_out[..., 0].contiguous().view(iv) != val2.view(iv)).sum())
                    differ_b = int((peak_out[..., 1].to(torch.int64) != idx2).sum())
                    assert differ_v == 0, differ_v
                    mk, mf, mt = stat(ts["peak"]), stat(ts["filterbank"]), stat(ts["two-pass"])
                    spread = (mf[2] - mf[1]) / mf[0]
                    log(f"{name} n={n} m={m} {window} {combo} {bank_name} ({nbands} bands) every={every} rows={rows}: kernel {geo[0]} chunks {geo[1]} x {geo[2]} "
                        f"launches {geo[3]}  differ values {differ_v} bins {differ_b}")
                    log(f"  peak       {mk[0]:.3f} ms  [min {mk[1]:.3f} max {mk[2]:.3f}]  / filterbank {mk[0] / mf[0]:.3f}")
                    log(f"  filterbank {mf[0]:.3f} ms  [min {mf[1]:.3f} max {mf[2]:.3f}]  spread {spread:.3f}")
                    log(f"  two-pass   {mt[0]:.3f} ms  [min {mt[1]:.3f} max {mt[2]:.3f}]  two-pass / peak {mt[0] / mk[0]:.2f}")
                    del peak_out, fb_out, dense_out, val2, idx2
                    torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
