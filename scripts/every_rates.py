"""Rates of the decimated analysis (sdft_hip_sdft_every_n) against sdft_sdft_n, in the same process, on one MI355X.

    python scripts/every_rates.py [--out profiles/every_rates.txt] [--reps 7]

Device pointers, one plan per type pair and shape, warm-up calls first, every call timed by a pair of HIP events on the
plan's stream; sdft_sdft_n and the decimated call alternate within each repeat (so drift hits both alike); the median
of the repeats is reported.  Shapes: configs[1] (n = 1e6, m = 1024, Hann, FD double) at every = 1, 16, 100, 1000;
configs[2] (n = 262 144, m = 4096, Blackman, FD float) at every = 1, 256.  Then the chunk length of the decimated kernel
for configs[1] at every = 100 (option "chunk"), to check the library's own choice.  A kernel trace belongs to a separate
run under rocprofv3 --kernel-trace --stats (see the file's header for the command)."""

from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "every_rates.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="fewer repeats, no chunk sweep (for a trace run)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from sdft_amd.sdft import SDFT, every_rows
    from sdft_amd.signals import sine_sweep

    torch.cuda.set_device(0)
    reps = 2 if args.quick else args.reps
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    def timed(p, fn):
        stream = torch.cuda.ExternalStream(p.api.get_stream(p._p))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    log(f"# every_rates.py  {time.strftime('%Y-%m-%d %H:%M:%S')}  device {torch.cuda.get_device_name(0)}  reps {reps} (median)")
    log("# Msamples/s = n / median ms / 1e3; speedup = sdft_sdft_n ms / sdft_every_n ms")
    shapes = [("configs[1]", 1_000_000, 1024, "hann", "f32f64", (1, 16, 100, 1000)),
              ("configs[2]", 262_144, 4096, "blackman", "f32f32", (1, 256))]
    for name, n, m, window, combo, everys in shapes:
        x = torch.from_numpy(sine_sweep(n)).cuda()
        with SDFT(m, window, 1.0, combo) as p:
            cdt = torch.complex128 if combo.endswith("f64") else torch.complex64
            full = torch.empty((n, m), dtype=cdt, device="cuda")
            outs = {e: torch.empty((every_rows(n, e, 0), m), dtype=cdt, device="cuda") for e in everys if e != 1}
            for _ in range(2):                                            # warm-up (allocations, pinned buffers, tables)
                p.sdft(x, out=full)
                for e in everys:
                    if e != 1:
                        p.sdft_every(x, e, 0, out=outs[e])
            p.set_option("pipeline", 0)
            t_full, t_every = [], {e: [] for e in everys}
            geo = {}
            for _ in range(reps):
                t_full.append(timed(p, lambda: p.sdft(x, out=full)))
                for e in everys:
                    if e == 1:
                        t_every[e].append(timed(p, lambda: p.sdft_every(x, 1, 0, out=full)))
                    else:
                        t_every[e].append(timed(p, lambda: p.sdft_every(x, e, 0, out=outs[e])))
                        geo[e] = (p.get_option("last_kernel"), p.get_option("last_chunks"), p.get_option("last_chunk_len"), p.get_option("last_chain"))
            mf = float(np.median(t_full))
            log(f"{name} n={n} m={m} {window} {combo}: sdft_sdft_n {mf:.3f} ms  {n / mf / 1e3:.1f} Msamples/s")
            for e in everys:
                me = float(np.median(t_every[e]))
                g = geo.get(e)
                gs = f"  kernel {g[0]} chunks {g[1]} x {g[2]} chain {g[3]}" if g else "  (sdft_sdft_n route)"
                log(f"  every={e:5d} rows={every_rows(n, e, 0):7d}: {me:.3f} ms  {n / me / 1e3:.1f} Msamples/s  speedup {mf / me:.2f}x{gs}"
                    f"  [min {min(t_every[e]):.3f} max {max(t_every[e]):.3f}]")
            del full, outs
            torch.cuda.empty_cache()
    if not args.quick:
        n, m = 1_000_000, 1024
        x = torch.from_numpy(sine_sweep(n)).cuda()
        log("# configs[1], every = 100: chunk length of forward_every_kernel (option chunk; 0 = the library's choice)")
        with SDFT(m, "hann", 1.0, "f32f64") as p:
            out = torch.empty((every_rows(n, 100, 0), m), dtype=torch.complex128, device="cuda")
            for chunk in (0, 1024, 2048, 4632, 9264, 18528):
                p.set_option("chunk", chunk)
                p.sdft_every(x, 100, 0, out=out)
                ts = [timed(p, lambda: p.sdft_every(x, 100, 0, out=out)) for _ in range(reps)]
                log(f"  chunk={chunk:6d} ({p.get_option('last_chunks')} chunks of {p.get_option('last_chunk_len')}): {float(np.median(ts)):.3f} ms")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
