"""Rates of the channel-mix analysis (sdft_hip_sdft_mix_n) against the two-pass route it replaces and against its arithmetic
floor, in the same process, on one MI355X.

    python scripts/mix_rates.py [--out profiles/mix_rates.txt] [--reps 5]

Device pointers, plain allocations, warm-up calls first, every route timed by a pair of HIP events on its plan's stream; the routes
alternate within each repeat (so drift hits all alike); the median of the repeats is reported with the smallest and the largest,
and each route's run-to-run spread (max - min) / median.

One GPU's share of BASELINE configs[4] -- 64 channels x 48000 samples, m = 1024, Hann, f32f64 -- and f32f32 at 16 channels; the
mix = all channels, all bins, nout in {1, 4}, every in {1, 100}.  Per line:

    mix           sdft_hip_sdft_mix_n at the product's group and block size: [nout][rows][m] complex
    two-pass      (a) sdft_hip_sdft_every_n over the same channels, [nch][rows][m] complex, then torch.einsum with the weights: what a
                  host did before this call (every = 1, first = 0 is sdft_sdft_n itself)
    power         (b) sdft_hip_sdft_power_n over the same channels: the arithmetic floor -- every recurrence and window once, no
                  weights, and it delivers no mix
    G, O          the mix at each candidate of the hooks build (options "mix_group", "mix_block"), timed one after the other, so
                  that the kept pair is on record

The mix's values are compared with the two-pass result, both from a fresh state (largest deviation relative to the largest
value; the einsum sums in an order of its own)."""

from __future__ import annotations

import argparse
import contextlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_rates.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="f32f64:64,f32f32:16")
    ap.add_argument("--candidates", type=int, default=1)
    args = ap.parse_args()
    import numpy as np
    import torch
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

    def fmt(name, s, tail=""):
        return f"  {name:<13s}{s[0]:9.3f} ms  [min {s[1]:.3f} max {s[2]:.3f}]  spread {(s[2] - s[1]) / s[0]:.3f}{tail}"

    log(f"# mix_rates.py  {time.strftime('%Y-%m-%d %H:%M:%S')}  device {torch.cuda.get_device_name(0)}  reps {reps} (median), 2 warm-up calls per route")
    log("# ms per call of nch channels x n samples, all bins, the mix = all channels; x two-pass = two-pass ms / mix ms; x floor = mix ms / power ms;")
    log("# spread = (max - min) / median of the route itself; dev = largest |mix - two-pass| / largest |two-pass|")
    n, m, window = 48000, 1024, "hann"
    base = sine_sweep(n)
    for shape in args.shapes.split(","):
        combo, nch = shape.split(":")
        nch = int(nch)
        double = combo.endswith("f64")
        cdtype = torch.complex128 if double else torch.complex64
        x = torch.from_numpy(np.stack([base + noise(n, seed=100 + c) * np.float32(0.25) for c in range(nch)]).astype(np.float32)).cuda()
        rng = np.random.default_rng(nch)
        for nout in (1, 4):
            w = (rng.standard_normal((nout, nch, m)) + 1j * rng.standard_normal((nout, nch, m))).astype(np.complex128 if double else np.complex64)
            dw = torch.from_numpy(w).cuda()
            for every in (1, 100):
                rows = every_rows(n, every, 0)
                with contextlib.ExitStack() as stack:
                    p = stack.enter_context(SDFT(m, window, 1.0, combo, nch))
                    q = stack.enter_context(SDFT(m, window, 1.0, combo, nch))
                    for plan in (p, q):
                        plan.set_option("pipeline", 0)
                    p.set_mix(w)
                    kept = (p.get_option("mix_group"), p.get_option("mix_block"))
                    mix_out = torch.empty((nout, rows, m), dtype=cdtype, device="cuda")
                    rows_out = torch.empty((nch, rows, m), dtype=cdtype, device="cuda")
                    power_out = torch.empty((nch, rows, m), dtype=torch.float64 if double else torch.float32, device="cuda")
                    two = {}

                    def two_pass():
                        if every == 1:
                            q.sdft(x, out=rows_out)
                        else:
                            q.sdft_every(x, every, 0, out=rows_out)
                        two["y"] = torch.einsum("ock,ctk->otk", dw, rows_out)

                    routes = [("mix", p, lambda: p.mix(x, every, 0, out=mix_out)), ("two-pass", q, two_pass),
                              ("power", q, lambda: q.power(x, every, 0, out=power_out))]
                    for _ in range(2):
                        for _, _, fn in routes:
                            fn()
                    geo = {}
                    ts = {k: [] for k, _, _ in routes}
                    for _ in range(reps):
                        for k, plan, fn in routes:
                            ts[k].append(timed(plan, fn))
                            geo[k] = (plan.get_option("last_kernel"), plan.get_option("last_chunks"), plan.get_option("last_chunk_len"))
                    # the values: the same samples from the same (fresh) state on both plans
                    p.reset()
                    q.reset()
                    p.mix(x, every, 0, out=mix_out)
                    two_pass()
                    torch.cuda.synchronize()
                    dev = float((mix_out - two["y"]).abs().max() / two["y"].abs().max())
                    s = {k: stat(v) for k, v in ts.items()}
                    log(f"{nch} x n={n} m={m} {window} {combo} nout={nout} every={every} rows={rows}: kept (G, O) = {kept}; dev {dev:.1e}")
                    log(fmt("mix", s["mix"], f"  kernel {geo['mix'][0]} chunks {geo['mix'][1]} x {geo['mix'][2]}  x two-pass {s['two-pass'][0] / s['mix'][0]:.2f}  x floor {s['mix'][0] / s['power'][0]:.2f}"))
                    log(fmt("two-pass", s["two-pass"], f"  kernel {geo['two-pass'][0]} chunks {geo['two-pass'][1]} x {geo['two-pass'][2]}"))
                    log(fmt("power", s["power"], f"  kernel {geo['power'][0]} chunks {geo['power'][1]} x {geo['power'][2]}"))
                    del rows_out, power_out, two
                    torch.cuda.empty_cache()
                    if args.candidates:
                        # the candidates, one after the other on a plan of the hooks build (a change of the block size rebuilds the
                        # plan's item table: inside the warm-up calls, not inside a timed one)
                        h = stack.enter_context(SDFT(m, window, 1.0, combo, nch, hooks=True))
                        h.set_option("pipeline", 0)
                        h.set_mix(w)
                        cells = []
                        for g in (2, 4, 8):
                            for o in (1, 2, 4):
                                if o > 1 and nout == 1 and o != kept[1]:
                                    continue                   # (one output: every block size runs the same wave)
                                h.set_option("mix_group", g)
                                h.set_option("mix_block", o)
                                for _ in range(2):
                                    h.mix(x, every, 0, out=mix_out)
                                c = stat([timed(h, lambda: h.mix(x, every, 0, out=mix_out)) for _ in range(reps)])
                                cells.append(f"({g}, {o}) {c[0]:.3f} [{c[1]:.3f} {c[2]:.3f}]")
                        log("  G, O         " + "  ".join(cells))
                    del mix_out
                torch.cuda.empty_cache()
        del x
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
