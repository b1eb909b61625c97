"""Rates of the array covariance analysis (sdft_hip_sdft_covariance_n) against the same matrix as a pair list of the pooled
cross-spectrum call, in the same process, on one MI355X.

    python scripts/covariance_rates.py [--out profiles/covariance_rates.txt] [--reps 9]

Device pointers, plain allocations, warm-up calls first, every route timed by a pair of HIP events on its plan's stream; the routes
alternate within each repeat (so drift hits all alike); the median of the repeats is reported with the smallest and the largest.
The run-to-run spread a comparison is read against is the pair list's own: (max - min) / median.

Plans of nch channels x 48000 samples, m = 1024, Hann, all bins, every = 480 (100 rows), the array = all channels:
f32f64 at nch = 8, 16 and 64, f32f32 at nch = 16.  Per line:

    covariance    sdft_hip_sdft_covariance_n at the product's group size: [nch (nch + 1) / 2][rows][m] complex sums
    G = 1, 2, 4   the same call at each candidate group size (the hooks build's option "array_group"), so the kept one is on record
    pair list     sdft_hip_sdft_cross_sum_n with covariance_pairs(nch) on a twin plan: unchanged code, the same output
    pooled power  sdft_hip_sdft_power_sum_n over the same channels: the arithmetic floor -- every recurrence once, no cross term

The covariance call's output is compared with the pair list's for equal bits.  FD double's default carries depend on where time is
cut, and the two calls cut it differently (their launches have different numbers of work items), so the comparison is made with
option "chunk" set to the covariance call's chunk length on both plans; the timed calls run with default options."""

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covariance_rates.txt"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", default="f32f64:8,f32f64:16,f32f64:64,f32f32:16")
    args = ap.parse_args()
    import numpy as np
    import torch
    from sdft_amd.sdft import SDFT, covariance_pairs, power_sum_rows
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
        return f"  {name:<13s}{s[0]:9.3f} ms  [min {s[1]:.3f} max {s[2]:.3f}]{tail}"

    log(f"# covariance_rates.py  {time.strftime('%Y-%m-%d %H:%M:%S')}  device {torch.cuda.get_device_name(0)}  reps {reps} (median), 2 warm-up calls per route")
    log("# ms per call of nch channels x n samples, all bins, the array = all channels; x pair list = pair list ms / covariance ms;")
    log("# spread = (max - min) / median of the pair list; x floor = covariance ms / pooled power ms; bits: covariance against pair list at equal chunks")
    n, m, window, every = 48000, 1024, "hann", 480
    rows = power_sum_rows(n, every, 0)
    base = sine_sweep(n)
    for shape in args.shapes.split(","):
        combo, nch = shape.split(":")
        nch = int(nch)
        T = nch * (nch + 1) // 2
        cdtype = torch.complex128 if combo.endswith("f64") else torch.complex64
        x = torch.from_numpy(np.stack([base + noise(n, seed=100 + c) * np.float32(0.25) for c in range(nch)]).astype(np.float32)).cuda()
        a, b = covariance_pairs(nch)
        groups = {"covariance": 0, "G = 1": 1, "G = 2": 2, "G = 4": 4}
        with contextlib.ExitStack() as stack:
            # a plan per route (a change of the group size rebuilds the plan's item table: not inside a timed call)
            plans = {k: stack.enter_context(SDFT(m, window, 1.0, combo, nch, hooks=True)) for k in list(groups) + ["pair list"]}
            plans["pooled power"] = plans["pair list"]
            p, q = plans["covariance"], plans["pair list"]
            for k, plan in plans.items():
                plan.set_option("pipeline", 0)
                if k in groups:
                    plan.set_option("array_group", groups[k])
                    plan.set_array(nch)
            q.set_pairs(a, b)
            kept = p.get_option("array_group")
            cov_out = torch.empty((T, rows, m), dtype=cdtype, device="cuda")
            pair_out = torch.empty((T, rows, m), dtype=cdtype, device="cuda")
            power_out = torch.empty((nch, rows, m), dtype=torch.float64 if combo.endswith("f64") else torch.float32, device="cuda")
            routes = [(k, (lambda k=k: plans[k].covariance(x, every, 0, out=cov_out))) for k in groups]
            routes += [("pair list", lambda: q.cross_sum(x, every, 0, out=pair_out)), ("pooled power", lambda: q.power_sum(x, every, 0, out=power_out))]
            for _ in range(2):
                for _, fn in routes:
                    fn()
            geo = {}
            ts = {k: [] for k, _ in routes}
            for _ in range(reps):
                for k, fn in routes:
                    ts[k].append(timed(plans[k], fn))
                    geo[k] = (plans[k].get_option("last_kernel"), plans[k].get_option("last_chunks"), plans[k].get_option("last_chunk_len"))
            # equal bits: the same samples from the same state, time cut alike on both plans
            chunk = geo["covariance"][2]
            for plan in (p, q):
                plan.set_option("chunk", chunk)
                plan.reset()
            p.covariance(x, every, 0, out=cov_out)
            q.cross_sum(x, every, 0, out=pair_out)
            torch.cuda.synchronize()
            assert p.get_option("last_chunk_len") == q.get_option("last_chunk_len") == chunk
            equal = bool(torch.equal(torch.view_as_real(cov_out).view(torch.int64 if combo.endswith("f64") else torch.int32),
                                     torch.view_as_real(pair_out).view(torch.int64 if combo.endswith("f64") else torch.int32)))
            s = {k: stat(v) for k, v in ts.items()}
            spread = (s["pair list"][2] - s["pair list"][1]) / s["pair list"][0]
            log(f"{nch} x n={n} m={m} {window} {combo} every={every} rows={rows} pairs={T}: group size kept G = {kept}; bits {'equal' if equal else 'DIFFER'} at chunks of {chunk}")
            log(fmt("covariance", s["covariance"], f"  kernel {geo['covariance'][0]} chunks {geo['covariance'][1]} x {geo['covariance'][2]}  x pair list {s['pair list'][0] / s['covariance'][0]:.2f}  x floor {s['covariance'][0] / s['pooled power'][0]:.2f}"))
            for g in (1, 2, 4):
                k = f"G = {g}"
                log(fmt(k, s[k], f"  chunks {geo[k][1]} x {geo[k][2]}  x pair list {s['pair list'][0] / s[k][0]:.2f}"))
            log(fmt("pair list", s["pair list"], f"  kernel {geo['pair list'][0]} chunks {geo['pair list'][1]} x {geo['pair list'][2]}  spread {spread:.3f}"))
            log(fmt("pooled power", s["pooled power"]))
            del cov_out, pair_out, power_out
        del x
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
