"""Pooled power analysis (sdft_hip_sdft_power_sum_n, SDFT.power_sum) on a real MI355X against the oracle.

The reference row is the sum, over the row's window, of the oracle's powers in the FD dtype (re*re + im*im of its rows, as
tests/test_gpu_power.py forms them), by a summation whose own error is below u S: float64 sums for FD float; for FD double
np.longdouble sums for windows under 2048 samples, math.fsum for longer ones.

The bar, element by element, with L the window's length, u = 2^-24 (float) or 2^-53 (double), gamma_L = L u / (1 - L u):
gamma_L * want on the bit-identical routes (FD float, FD double with carry = 1, calls of one time chunk); for FD double with
default carries L * 2.1e-11 * (largest power compared) comes on top.  The library promises gamma_(L-1); the step to gamma_L pays
for the reference's own rounding.

Inputs are sine_sweep(n) + 0.25 noise(n), the signal of tests/test_gpu_power.py."""

import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import guarded as G
from oracle import oracle as O
from sdft_amd.sdft import every_next_first, power_sum_rows
from sdft_amd.signals import noise
from test_gpu_power import BAR, WINDOWS, bands_of, exact_combo, expected, make, oracle_power, rel, signal, to_dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(1, 0), (1, 3), (7, 6), (100, 0), (100, 37), (1024, 1023), (6000, 0), (10000, 0), (50, 7000)]
assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "the FD double reference needs an extended long double"


def windows(n, every, first):
    """[begin, end) of every row of a call, by the issue's definition"""
    w = [(0, min(first, n))] if first > 0 and n > 0 else []
    w += [(b, min(b + every, n)) for b in range(first, n, every)]
    assert len(w) == power_sum_rows(n, every, first)
    return w


def wide(fd):
    return np.float64 if np.dtype(fd) == np.float32 else np.longdouble


@functools.lru_cache(maxsize=8)
def long_window(combo, window, m, n, b, e):
    """FD double, a window of 2048 samples or more: math.fsum per bin (exact, rounded once)"""
    p = expected(combo, window, m, n)[1][b:e]
    out = np.array([math.fsum(p[:, k]) for k in range(p.shape[1])], dtype=np.longdouble)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=4)
def pooled(combo, window, m, n, every, first):
    """(rows, m) reference sums of one shape and grid in the wide dtype, and the rows' window lengths; shared, never written"""
    p = expected(combo, window, m, n)[1]
    hi = wide(p.dtype)
    w = windows(n, every, first)
    out = np.empty((len(w), m), dtype=hi)
    for r, (b, e) in enumerate(w):
        if e - b == 1:
            out[r] = p[b]
        elif hi is np.float64 or e - b < 2048:
            out[r] = p[b:e].astype(hi).sum(axis=0)
        else:
            out[r] = long_window(combo, window, m, n, b, e)
    lens = np.array([e - b for b, e in w])
    out.setflags(write=False)
    return out, lens


def check(got, want, lens, exact, pmax, what):
    """|got - want| <= gamma_L want (+ L * BAR * pmax on the routes that are not bit-identical), element by element"""
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    fd = np.float32 if want.dtype == np.float64 else np.float64
    assert got.shape == want.shape and got.dtype == fd, (what, got.shape, want.shape, got.dtype)
    if want.size == 0:
        return
    u = want.dtype.type(2.0 ** -24 if fd == np.float32 else 2.0 ** -53)
    L = np.asarray(lens, dtype=want.dtype)[:, None]
    bar = L * u / (1 - L * u) * want
    if not exact:
        bar = bar + L * want.dtype.type(BAR) * want.dtype.type(pmax)
    err = np.abs(got.astype(want.dtype) - want)
    bad = err > bar
    assert not bad.any(), (what, int(bad.sum()), float((err / np.maximum(bar, np.finfo(want.dtype).tiny)).max()))


def check_band(got, combo, window, m, n, every, first, band, exact, what):
    want, lens = pooled(combo, window, m, n, every, first)
    pmax = float(expected(combo, window, m, n)[1][:, band[0]:band[0] + band[1]].max())
    check(got, want[:, band[0]:band[0] + band[1]], lens, exact, pmax, what)


# ---------------------------------------------------------------------------------------------
# parity: every type pair x window x dftsize x grid x band
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("window", WINDOWS)
def test_power_sum_parity(combo, window):
    call = 0
    n = 6000                                    # several chunks, and a roll-over at 2N
    for m in (1, 2, 3, 5, 64, 125, 1000, 1024):
        x = expected(combo, window, m, n)[0]
        dx = to_dev(x)
        with make(m, window, combo) as p:
            bands = bands_of(m, p)
            for every, first in GRIDS:
                for band in bands:
                    p.reset()
                    call += 1
                    got = p.power_sum(dx if call % 2 else x, every, first, bins=band)
                    assert p.get_option("last_kernel") == 6, (m, every, first, band)
                    if m >= 1000:
                        assert p.get_option("last_chunks") > 1, (m, every, first, band)
                    assert got.shape == (power_sum_rows(n, every, first), band[1])
                    check_band(got, combo, window, m, n, every, first, band, exact_combo(combo), (combo, window, m, every, first, band))
            # bins=None is the whole row
            p.reset()
            check_band(p.power_sum(x, 7, 6), combo, window, m, n, 7, 6, (0, m), exact_combo(combo), (combo, window, m, "bins=None"))


@pytest.mark.parametrize("combo", O.COMBOS)
def test_power_sum_parity_4096(combo):
    m, n = 4096, 10000
    x = expected(combo, "hann", m, n)[0]
    with make(m, "hann", combo) as p:
        for i, (every, first, band) in enumerate([(100, 37, (0, m)), (1024, 1023, (1, m - 2)), (10000, 0, (4000, 96)), (7, 6, (61, 3))]):
            p.reset()
            got = p.power_sum(to_dev(x) if i % 2 else x, every, first, bins=band)
            assert p.get_option("last_kernel") == 6 and p.get_option("last_chunks") > 1
            check_band(got, combo, "hann", m, n, every, first, band, exact_combo(combo), (combo, m, every, first, band))


# ---------------------------------------------------------------------------------------------
# bitwise anchors, determinism
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
def test_power_sum_of_one_sample_windows_is_power_bit_for_bit(combo):
    n = 6000
    for m in (5, 125, 1024):
        x = expected(combo, "hann", m, n)[0]
        with make(m, "hann", combo) as p, make(m, "hann", combo) as q:
            for i, band in enumerate(bands_of(m, p)):
                p.reset()
                q.reset()
                xs = to_dev(x) if i % 2 else x
                a, b = p.power_sum(xs, 1, 0, bins=band), q.power(xs, 1, 0, bins=band)
                a, b = (a.cpu().numpy(), b.cpu().numpy()) if i % 2 else (a, b)
                assert p.get_option("last_kernel") == 6 and q.get_option("last_kernel") == 5
                assert a.shape == b.shape == (n, band[1]) and np.array_equal(a, b), (combo, m, band)


def test_power_sum_row_counts():
    combo, m = "f32f32", 64
    x = signal(6000, np.float32, 3)
    with make(m, "hann", combo) as p:
        for every, first in GRIDS:
            for n in (0, 1, 37, 38, 511, 6000):
                p.reset()
                got = p.power_sum(x[:n], every, first, bins=(3, 5))
                assert got.shape == (power_sum_rows(n, every, first), 5) == (len(windows(n, every, first)), 5), (n, every, first)
                assert (got.shape[0] == 0) == (n == 0)
        # the C call answers the same count
        out = np.zeros((70, m), dtype=np.float32)
        for every, first in GRIDS:
            rows = power_sum_rows(3000, every, first)
            if rows <= out.shape[0]:
                p.reset()
                assert p.api.sdft_power_sum_n(p._p, 3000, x.ctypes.data, every, first, 0, m, out.ctypes.data) == rows, (every, first)


@pytest.mark.parametrize("combo", ["f32f64", "f64f32"])
def test_power_sum_same_bits_on_every_run(combo):
    m, n = 1000, 6000
    x = expected(combo, "hann", m, n)[0]
    for device in (False, True):
        xs = to_dev(x) if device else x
        with make(m, "hann", combo) as p:
            for every, first in [(100, 37), (6000, 0)]:
                runs = []
                for _ in range(3):
                    p.reset()
                    d = p.power_sum(xs, every, first)
                    assert p.get_option("last_chunks") > 1
                    runs.append(d.cpu().numpy() if device else d)
                assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2]), (combo, device, every, first)


# ---------------------------------------------------------------------------------------------
# streaming: uneven calls, head rows added to the previous tails; state; what follows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("every,first0", [(100, 37), (1024, 1023), (6000, 0)])
def test_power_sum_streaming(combo, every, first0):
    m, n, band = 1000, 6000, (10, 300)
    lengths = [1, 99, 100, 511, 512, 513, 3000]
    lengths.append(n - sum(lengths))
    x = expected(combo, "hann", m, n)[0]
    ref = O.best(m, "hann", 1.0, combo)
    for t in range(0, n, 2048):
        ref.sdft(x[t:t + 2048])
    bitwise = exact_combo(combo)
    with make(m, "hann", combo) as p:
        rows, t, first = [], 0, first0
        for i, k in enumerate(lengths):
            xs = x[t:t + k]
            d = p.power_sum(to_dev(xs) if i % 3 == 1 else xs, every, first, bins=band)
            d = d.cpu().numpy() if hasattr(d, "cpu") else d
            assert d.shape == (power_sum_rows(k, every, first), band[1])
            if first > 0 and t > 0:
                rows[-1] = rows[-1] + d[0]               # the head completes the previous call's last row: the host adds the two
                d = d[1:]
            rows += list(d)
            first = every_next_first(k, every, first)
            t += k
        check_band(np.array(rows), combo, "hann", m, n, every, first0, band, bitwise, (combo, every, first0, "streamed"))
        acc, fid, hist, cur = p.state()
        ra, rf, rh, rc = [np.array(v) for v in ref.state()[:3]] + [ref.state()[3]]
        assert cur == rc and np.array_equal(hist, rh)
        if bitwise:
            assert np.array_equal(acc, ra) and np.array_equal(fid, rf)
        else:
            assert rel(acc, ra) <= 1e-10 and rel(fid, rf) <= 1e-10, (rel(acc, ra), rel(fid, rf))


@pytest.mark.parametrize("combo", O.COMBOS)
def test_power_sum_leaves_the_state_of_power(combo):
    """after a pooled call a following sdft_n or isdft_n continues as after power of the same samples"""
    td = O.combo_types(combo)[0]
    m, n = 1000, 6000
    x = expected(combo, "hann", m, n)[0]
    hop = noise(100, seed=12, dtype=td)
    for device in (False, True):
        with make(m, "hann", combo) as p, make(m, "hann", combo) as q:
            xs = to_dev(x) if device else x
            p.power_sum(xs, 100, 37, bins=(10, 300))
            # the twin forms the same terms: power at every sample.  (The pooled call cuts time as that call does --
            # logic::choose_power_sum_chunks -- so FD double's fast carries round alike; power on a sparse grid cuts time
            # differently and agrees bit for bit only where the carries are exact.)
            q.power(xs, 1, 0, bins=(10, 300))
            if exact_combo(combo):
                with make(m, "hann", combo) as r:
                    r.power(xs, 100, 37, bins=(10, 300))
                    assert all(np.array_equal(a, b) for a, b in zip(p.state()[:3], r.state()[:3]))
            for a, b in zip(p.state()[:3], q.state()[:3]):
                assert np.array_equal(a, b)
            assert p.state()[3] == q.state()[3]
            dp, dq = p.sdft(hop), q.sdft(hop)
            assert np.array_equal(dp, dq)
            assert np.array_equal(p.isdft(dp), q.isdft(dq))


# ---------------------------------------------------------------------------------------------
# batched plans, exact carries, forced routes, host staging
# ---------------------------------------------------------------------------------------------
def check_channels(got, x, combo, window, m, every, first, band, exact, what):
    fd = O.combo_types(combo)[1]
    hi = wide(fd)
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    w = windows(x.shape[1], every, first)
    assert got.shape == (x.shape[0], len(w), band[1]), (what, got.shape)
    for c in range(x.shape[0]):
        p = oracle_power(O.best(m, window, 1.0, combo), x[c])[:, band[0]:band[0] + band[1]]
        want = np.array([[math.fsum(p[b:e, k]) for k in range(band[1])] for b, e in w], dtype=hi)
        check(got[c], want, [e - b for b, e in w], exact, float(p.max()), (what, c))


@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_power_sum_batched_channels(combo):
    td = O.combo_types(combo)[0]
    ch, m, n, band = 3, 64, 3000, (17, 30)
    x = np.stack([signal(n, td, 100 + c) for c in range(ch)])
    for device in (False, True):
        with make(m, "blackman", combo, channels=ch) as p:
            for every, first in [(100, 37), (3000, 0)]:
                p.reset()
                got = p.power_sum(to_dev(x) if device else x, every, first, bins=band)
                assert p.get_option("last_kernel") == 6 and p.get_option("last_chunks") > 1
                check_channels(got, x, combo, "blackman", m, every, first, band, exact_combo(combo), (combo, device, every))


@pytest.mark.parametrize("combo", ["f32f64", "f64f64"])
def test_power_sum_exact_carries(combo):
    """FD double with option carry = 1: a bit-identical route, the bar is gamma_L alone"""
    n = 6000
    for m in (5, 1000):
        x = expected(combo, "hann", m, n)[0]
        band = (3, max(1, m - 5))
        with make(m, "hann", combo, carry=1) as p:
            for i, (every, first) in enumerate([(7, 6), (100, 37), (1024, 1023), (6000, 0)]):
                p.reset()
                got = p.power_sum(to_dev(x) if i % 2 else x, every, first, bins=band)
                assert p.get_option("last_chunks") > 1 and p.get_option("last_kernel") == 6
                check_band(got, combo, "hann", m, n, every, first, band, True, (combo, m, every, first))


@pytest.mark.parametrize("opts", [dict(chunk=128), dict(chunk=1000), dict(carry=1, segments=3), dict(carry=1, chain=2), dict(carry=1, chain=0)],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_power_sum_forced_routes(opts):
    combo, m, n, band = "f32f64", 1000, 6000, (1, 998)
    x = expected(combo, "hann", m, n)[0]
    with make(m, "hann", combo, **opts) as p:
        for every, first in [(100, 37), (6000, 0)]:
            p.reset()
            got = p.power_sum(to_dev(x), every, first, bins=band)
            assert p.get_option("last_chunks") > 1 and p.get_option("last_kernel") == 6
            check_band(got, combo, "hann", m, n, every, first, band, "carry" in opts, (opts, every, first))


@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_power_sum_host_staging_in_segments(combo):
    """stage_bytes small enough for several segments: windows shorter than a segment, longer than one, and one over all of them;
    host samples with host and with device sums"""
    import torch
    fd = O.combo_types(combo)[1]
    m, n, band = 1000, 6000, (10, 300)
    x = expected(combo, "hann", m, n)[0]
    row = band[1] * np.dtype(fd).itemsize
    for stage, grids in [(7 * row, [(100, 37), (100, 0)]), (2 * row, [(1024, 1023), (6000, 0), (700, 0)])]:
        with make(m, "hann", combo, stage_bytes=stage) as p:
            for every, first in grids:
                rows = power_sum_rows(n, every, first)
                p.reset()
                check_band(p.power_sum(x, every, first, bins=band), combo, "hann", m, n, every, first, band, exact_combo(combo), (combo, stage, every, first, "host"))
                p.reset()
                out = torch.zeros((rows, band[1]), dtype=getattr(torch, np.dtype(fd).name), device="cuda")
                got = p.api.sdft_power_sum_n(p._p, n, C.c_void_p(x.ctypes.data), every, first, band[0], band[1], C.c_void_p(out.data_ptr()))
                p.synchronize()
                assert got == rows, p.api.last_error()
                check_band(out, combo, "hann", m, n, every, first, band, exact_combo(combo), (combo, stage, every, first, "host samples, device sums"))


def test_power_sum_async_device_pointers():
    m, n = 1000, 6000
    x = expected("f32f64", "hann", m, n)[0]
    with make(m, "hann", "f32f64", **{"async": 1}) as p:
        a = p.power_sum(to_dev(x), 100, 37, bins=(0, 256))
        p.synchronize()
        check_band(a, "f32f64", "hann", m, n, 100, 37, (0, 256), False, "async")


# ---------------------------------------------------------------------------------------------
# errors leave the state alone
# ---------------------------------------------------------------------------------------------
def test_power_sum_errors():
    combo, m = "f32f32", 64
    x = signal(3000, np.float32, 5)
    top = C.c_size_t(-1).value
    with make(m, "hann", combo) as p:
        api = p.api
        p.power_sum(x[:300], 7, 3)                          # (errors against a plan that is mid-stream)
        out = np.zeros((12, m), dtype=np.float32)
        before = p.state()
        refused = [(100, 0, 0, 0, m, out.ctypes.data, "every"),                 # every == 0
                   (100, 10, 0, 0, 0, out.ctypes.data, "nbins"),                # nbins == 0
                   (100, 10, 0, 1, m, out.ctypes.data, "band"),                 # bin0 + nbins > dftsize
                   (100, 10, 0, m, 1, out.ctypes.data, "band"),
                   (100, 10, 0, 2, top, out.ctypes.data, "band"),               # bin0 + nbins overflows to 1
                   (100, 10, 0, top, 2, out.ctypes.data, "band"),
                   (100, 10, 0, 0, m, None, "NULL"),                            # rows > 0, sums NULL
                   (100, 10, 5000, 0, m, None, "NULL")]                         # first >= n: the head row is a row
        for n, every, first, bin0, nb, ptr, word in refused:
            api.clear()
            assert api.sdft_power_sum_n(p._p, n, x.ctypes.data, every, first, bin0, nb, ptr) == -1, (every, bin0, nb)
            err = api.last_error()
            assert err and "sdft_hip_sdft_power_sum_n" in err and word in err, err
            api.clear()
            after = p.state()
            assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3], (every, bin0, nb)
        assert np.count_nonzero(out) == 0
        # n == 0: no rows, nothing moves, sums may be NULL
        assert api.sdft_power_sum_n(p._p, 0, x.ctypes.data, 10, 3, 0, m, None) == 0 and api.last_error() is None
        assert p.state()[3] == before[3]
        for bad in ((0, 0), (m, 1), (1, m), (-1, 2)):
            with pytest.raises(ValueError):
                p.power_sum(x[:10], bins=bad)
        with pytest.raises(ValueError):
            p.power_sum(x[:10], every=0)


# ---------------------------------------------------------------------------------------------
# no overrun, no hole, at every alignment of the output an element size allows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("combo", ["f32f32", "f32f64"])
def test_power_sum_guarded_misaligned_output(combo, host):
    """sums carved from a guarded arena at every residue modulo 16 its element size allows, and at 16 mod 128; a band of 999
    bins (an odd row length: consecutive rows change alignment), windows of 7 samples after a head of 3, many of them cut by
    chunk boundaries"""
    td, fd, _ = O.combo_types(combo)
    m, n, every, first, band = 1000, 2000, 7, 3, (1, 999)
    x = expected(combo, "hann", m, n)[0]
    rows = power_sum_rows(n, every, first)
    size = np.dtype(fd).itemsize
    places = [(r, 16) for r in range(size, 16, size)] + [(16, 128)]
    with make(m, "hann", combo) as p:
        for r, mod in places:
            arena = (G.HostArena if host else G.DeviceArena)(G.room(((n,), td), ((rows, band[1]), fd)))
            xv = G.put(arena.carve((n,), td, np.dtype(td).itemsize, 16, name="x"), x)
            out = arena.carve((rows, band[1]), fd, r, mod, name="sums")
            assert G.ptr_of(out) % mod == r
            p.reset()
            p.api.clear()
            got = p.api.sdft_power_sum_n(p._p, n, C.c_void_p(G.ptr_of(xv)), every, first, band[0], band[1], C.c_void_p(G.ptr_of(out)))
            p.synchronize()
            assert got == rows, p.api.last_error()
            assert p.get_option("last_kernel") == 6 and p.get_option("last_chunks") > 1
            arena.check()
            assert G.view_unwritten(out) == 0
            assert np.array_equal(G.to_numpy(xv), x)
            check_band(G.to_numpy(out), combo, "hann", m, n, every, first, band, exact_combo(combo), (combo, host, r, mod))


# ---------------------------------------------------------------------------------------------
# a plain C host: a stream in blocks, head rows added to the previous tails
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,combo", [([], "f32f64"), (["-DSDFT_FD_FLOAT"], "f32f32")])
def test_c_host_power_sum(tmp_path, hip_library, flags, combo):
    td, fd, _ = O.combo_types(combo)
    libdir = os.path.dirname(hip_library)
    rt = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    exe = tmp_path / "host_power_sum"
    cmd = ["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), *flags,
           os.path.join(ROOT, "tests", "c", "host_power_sum.c"), "-o", str(exe),
           "-L", libdir, "-lsdft_hip", "-L", rt, "-lamdhip64", "-lm", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{rt}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m, n, every, block, band = 1000, 6000, 100, 730, (0, 400)
    x = expected(combo, "hann", m, n)[0]
    x.tofile(tmp_path / "x.raw")
    r = subprocess.run([str(exe), str(m), str(every), str(block), str(band[0]), str(band[1]), str(tmp_path / "x.raw"), str(tmp_path / "s.raw")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "C-HOST-POWER-SUM ok" in r.stdout
    got = np.fromfile(tmp_path / "s.raw", dtype=fd).reshape(-1, band[1])
    check_band(got, combo, "hann", m, n, every, 0, band, exact_combo(combo), "C host")
