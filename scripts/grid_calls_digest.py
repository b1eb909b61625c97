"""One SHA-256 per case of a fixed table over the nine grid analysis calls (sdft_hip_sdft_every_n, _power_n, _filterbank_n, _mix_n,
_power_sum_n, _power_peak_n, _cross_sum_n, _lag_sum_n, _covariance_n): the acceptance test of a change to their host side, which
must leave every line as it was.

    python scripts/grid_calls_digest.py [--root TREE] [--out FILE]

--root: the tree whose package (and built library) is run, by default this one -- a built checkout of the parent commit gives the
other side of the comparison; the two outputs are compared with diff.

Per case the digest is over the output buffer's bytes (pre-filled with 0x5A, so what a call leaves unwritten counts) followed by
the plan's state after the call (sdft_hip_get_state: acc, fid, hist, cursor).  The table: type pairs f32f32 and f64f64; dftsize
64, 3 channels, n = 1000 seeded samples after a 100-sample analysis (so no call starts from the zero state); (every, first) in
(1, 0), (7, 5), (7, 0), (64, 0), (1000, 3); the band (3, 17), and the full band at (7, 5); samples and output each in host and in
device memory.  The calls go through the C-ABI with raw pointers, since the Python methods tie the output's kind to the samples'.
stage_bytes is two output rows of the call, so a host output goes in segments of two rows -- 500, 72, 8 segments; at every = 1000
the one or two the samples' hop floor allows -- and with (7, 5) the pooled calls' segments start inside windows (head rows,
joins); host samples into a device output take two segments, cut to whole windows at (7, 0) and (64, 0).  These are the smallest
shapes at which a wrong row0, stride, head join or segment size shows; the whole table takes a few seconds."""

from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch
    from sdft_amd.sdft import SDFT, every_rows, power_sum_rows

    torch.cuda.set_device(0)
    m, ch, n, warm = 64, 3, 1000, 100
    grids = [(1, 0), (7, 5), (7, 0), (64, 0), (1000, 3)]
    lines = []

    def filled(shape, dtype):
        count = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return np.full(count, 0x5A, dtype=np.uint8).view(dtype).reshape(shape)

    for combo in ("f32f32", "f64f64"):
        rng = np.random.default_rng(20240)
        with SDFT(m, "hann", 1.0, combo, ch) as p:
            xw = rng.standard_normal((ch, warm)).astype(p.td)
            xh = rng.standard_normal((ch, n)).astype(p.td)
            xd = torch.from_numpy(xh).cuda()
            p.set_filterbank([2, 10, 30], [12, 25, 34], rng.uniform(0.0, 1.0, 12 + 25 + 34))
            p.set_pairs([0, 1, 2, 0], [1, 2, 2, 0])
            p.set_array([2, 0, 1])
            p.set_mix(rng.standard_normal((2, ch, m)) + 1j * rng.standard_normal((2, ch, m)))
            # name -> (C function, pooled, banded, leading dimension, trailing dimension of a band of nb bins, dtype, arguments after the band)
            calls = {
                "every": ("sdft_every_n", False, False, ch, lambda nb: m, p.fdx, ()),
                "power": ("sdft_power_n", False, True, ch, lambda nb: nb, p.fd, ()),
                "filterbank": ("sdft_filterbank_n", False, False, ch, lambda nb: 3, p.fd, ()),
                "mix": ("sdft_mix_n", False, True, 2, lambda nb: nb, p.fdx, ()),
                "power_sum": ("sdft_power_sum_n", True, True, ch, lambda nb: nb, p.fd, ()),
                "power_peak_max": ("sdft_power_peak_n", True, True, ch, lambda nb: nb, p.fd, (0,)),
                "power_peak_min": ("sdft_power_peak_n", True, True, ch, lambda nb: nb, p.fd, (1,)),
                "cross_sum": ("sdft_cross_sum_n", True, True, 4, lambda nb: nb, p.fdx, ()),
                "lag_sum": ("sdft_lag_sum_n", True, True, ch, lambda nb: nb, p.fdx, ()),
                "covariance": ("sdft_covariance_n", True, True, 6, lambda nb: nb, p.fdx, ()),
            }
            for name, (cfn, pooled, banded, lead, trail, dtype, extra) in calls.items():
                fn = getattr(p.api, cfn)
                for every, first in grids:
                    bands = [(3, 17)] + ([(0, m)] if (every, first) == (7, 5) else [])
                    for bin0, nb in bands if banded else [(0, m)]:
                        rows = (power_sum_rows if pooled else every_rows)(n, every, first)
                        shape = (lead, rows, trail(nb))
                        row_bytes = lead * trail(nb) * np.dtype(dtype).itemsize
                        for x_dev in (False, True):
                            for o_dev in (False, True):
                                p.reset()
                                p.set_option("stage_bytes", 2 * row_bytes)
                                p.sdft(xw)
                                oh = filled(shape, dtype)
                                od = torch.from_numpy(oh).cuda() if o_dev else None
                                xp = xd.data_ptr() if x_dev else xh.ctypes.data
                                op = od.data_ptr() if o_dev else oh.ctypes.data
                                p.api.clear()
                                band = (bin0, nb) if banded else ()
                                got = fn(p._p, n, C.c_void_p(xp), every, first, *band, *extra, C.c_void_p(op))
                                p.api.check()
                                p.synchronize()
                                torch.cuda.synchronize()
                                out = od.cpu().numpy() if o_dev else oh
                                acc, fid, hist, cur = p.state()
                                h = hashlib.sha256()
                                for part in (out, acc, fid, hist):
                                    h.update(np.ascontiguousarray(part).tobytes())
                                h.update(str(cur).encode())
                                where = f"x={'dev' if x_dev else 'host'} out={'dev' if o_dev else 'host'}"
                                lines.append(f"{combo} {name:<14} every={every:<4} first={first} band={bin0}+{nb:<2} {where:<16} rows={got:<4} {h.hexdigest()}")
                                assert got == rows, (lines[-1], rows)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
