"""Power-spectrogram analysis (sdft_hip_sdft_power_n, SDFT.power) on a real MI355X against the oracle.

The oracle is fed in blocks and only re*re + im*im of its rows is kept, in the FD dtype -- the expression the call promises --
so no complex matrix is held on the host.  Bars: bit-identical wherever sdft_sdft_n is (FD float with its default exact
carries, FD double with carry = 1, calls of one time chunk), else 2.1e-11 of the largest power compared: the row bar of
tests/test_gpu_every.py (1e-11 of the largest bin) through | |X|^2 - |X'|^2 | <= (|X| + |X'|) |X - X'|, plus two roundings.

Inputs are sine_sweep(n) + 0.25 noise(n): for these the oracle's powers and both squares stay in the normal range, so
bit-identity does not hinge on subnormal handling."""

import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import guarded as G
from oracle import oracle as O
from sdft_amd.signals import noise, sine_sweep

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 2.1e-11
WINDOWS = ["boxcar", "hann", "hamming", "blackman"]
GRIDS = [(1, 0), (1, 3), (7, 6), (100, 0), (1024, 1023)]


def make(m, window="hann", combo="f32f64", channels=1, **opts):
    from sdft_amd.sdft import SDFT
    p = SDFT(m, window, 1.0, combo, channels)
    for k, v in opts.items():
        p.set_option(k, v)
    return p


def signal(n, td, seed):
    return sine_sweep(n).astype(td) + noise(n, seed=seed, dtype=td) * td(0.25)


def power_of(d):
    """re*re + im*im in the FD dtype: two rounded products, one rounded sum"""
    return d.real * d.real + d.imag * d.imag


def oracle_power(ref, x, block=2048):
    """(len(x), dftsize) powers of the oracle's matrix, fed in blocks"""
    fd = np.empty(0, dtype=ref.fdx).real.dtype
    out = np.empty((x.size, ref.dftsize), dtype=fd)
    for t in range(0, x.size, block):
        out[t:t + block] = power_of(ref.sdft(x[t:t + block]))
    return out


@functools.lru_cache(maxsize=2)
def expected(combo, window, m, n):
    """(samples, powers of every row) of one shape; computed once, shared, never written"""
    td = O.combo_types(combo)[0]
    x = signal(n, td, m)
    p = oracle_power(O.best(m, window, 1.0, combo), x)
    x.setflags(write=False)
    p.setflags(write=False)
    return x, p


def on_grid(p, every, first, band=None):
    rows = p[first::every]
    return rows if band is None else rows[:, band[0]:band[0] + band[1]]


def exact_combo(combo):
    return combo.endswith("f32")


def to_dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()             # (a copy: the shared expectations are read-only)


def deviation(got, want):
    """largest deviation relative to the largest power compared"""
    if want.size == 0:
        return 0.0
    scale = float(want.max())
    return float(np.abs(got - want).max()) / (scale if scale > 0 else 1.0)


def check(got, want, bitwise, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    if bitwise:
        assert np.array_equal(got, want), (what, deviation(got, want))
    else:
        assert deviation(got, want) <= BAR, (what, deviation(got, want))


def bands_of(m, p):
    """the bands of the parity test for a plan of m bins"""
    per = p.get_option("interior") * p.get_option("bins_per_lane")          # bins a tile owns
    last = (p.get_option("tiles") - 1) * per                                # the last tile's first bin
    assert 0 <= last < m
    inside = (last + (m - last) // 3, max(1, (m - last) // 3))              # wholly inside the last tile
    assert last <= inside[0] and inside[0] + inside[1] <= m
    bands = [(0, m), (0, 1), (m - 1, 1)]
    if m >= 3:
        bands.append((1, m - 2))            # the odd start puts the float pairs off 8-byte alignment
    # (61, 3) and (123, 3) lie across the first boundaries of tiles of 62 bins, the geometry of the test hook interior = 62 at FD
    # double; no default tile (56 or 64 lanes: 56 / 64 bins at FD double, 112 / 128 at FD float) ends inside them.  Of the default
    # tiles' boundaries (50, 100) crosses the first, and the two narrow bands from the plan's own per sit on it: the last bin of
    # tile 0 with the first of tile 1, and the first bin of tile 1 alone
    bands += [b for b in ((61, 3), (123, 3), (50, 100), (per - 1, 2), (per, 1)) if b[0] + b[1] <= m]
    bands.append(inside)
    return list(dict.fromkeys(bands))


# ---------------------------------------------------------------------------------------------
# parity: every type pair x window x dftsize x grid x band
# ---------------------------------------------------------------------------------------------
MS = (1, 2, 3, 5, 64, 125, 1000, 1024, 4096)


@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("window", WINDOWS)
def test_power_parity(combo, window):
    call = 0
    for m in MS:
        n = 10000 if m == 4096 else 6000        # several chunks, and a roll-over at 2N
        x, want = expected(combo, window, m, n)
        dx = to_dev(x)
        with make(m, window, combo) as p:
            for band in bands_of(m, p):
                for every, first in GRIDS:
                    p.reset()
                    call += 1
                    got = p.power(dx if call % 2 else x, every, first, bins=band)
                    assert p.get_option("last_kernel") == 5, (m, every, first, band)
                    if m >= 1000:
                        assert p.get_option("last_chunks") > 1, (m, every, first, band)
                    check(got, on_grid(want, every, first, band), exact_combo(combo), (combo, window, m, every, first, band))
            # bins=None is the whole row
            p.reset()
            check(p.power(x, 7, 6), on_grid(want, 7, 6), exact_combo(combo), (combo, window, m, "bins=None"))


@pytest.mark.parametrize("combo", ["f32f64", "f64f64"])
@pytest.mark.parametrize("window", ["hann", "blackman"])
def test_power_exact_carries_bit_identical(combo, window):
    """FD double with option carry = 1: the exact carries (relay or serial pass) feed the kernel, the powers are those of the
    reference's bits.  The band is (3, m - 5); at m = 5 that is empty, so the one bin (3, 1) stands in for it."""
    for m in (5, 1000, 1024):
        x, want = expected(combo, window, m, 12000)
        band = (3, max(1, m - 5))
        with make(m, window, combo, carry=1) as p:
            for i, (every, first) in enumerate(GRIDS):
                p.reset()
                got = p.power(to_dev(x) if i % 2 else x, every, first, bins=band)
                assert p.get_option("last_chunks") > 1 and p.get_option("last_kernel") == 5
                check(got, on_grid(want, every, first, band), True, (combo, window, m, every, first))


@pytest.mark.parametrize("combo", O.COMBOS)
def test_power_one_chunk_bit_identical(combo):
    for m in (1, 64, 1000):
        x, want = expected(combo, "hann", m, 500)
        with make(m, "hann", combo) as p:
            for band in [(0, m)] + ([(1, m - 2)] if m >= 3 else []):
                for i, (every, first) in enumerate([(1, 0), (1, 3), (7, 6), (100, 0)]):
                    p.reset()
                    got = p.power(to_dev(x) if i % 2 else x, every, first, bins=band)
                    assert p.get_option("last_chunks") == 1 and p.get_option("last_kernel") == 5
                    check(got, on_grid(want, every, first, band), True, (combo, m, every, first, band))


# ---------------------------------------------------------------------------------------------
# streaming: uneven calls, first carried as documented; state; a following hop
# ---------------------------------------------------------------------------------------------
def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    scale = float(np.abs(b).max())
    return float(np.abs(a - b).max()) / (scale if scale > 0 else 1.0)


@pytest.mark.parametrize("combo", O.COMBOS)
def test_power_streaming_state_and_next_hop(combo):
    from sdft_amd.sdft import every_next_first, every_rows
    td = O.combo_types(combo)[0]
    m, every, first0, band = 1000, 100, 37, (10, 300)
    lengths = [100, 3000, 37, 700, 5000, 1, 511, 512, 2600, 9000, 0, 64]
    x = signal(sum(lengths), td, 11)
    ref = O.best(m, "hann", 1.0, combo)
    want = on_grid(oracle_power(ref, x), every, first0, band)
    bitwise = exact_combo(combo)
    with make(m, "hann", combo) as p, make(m, "hann", combo) as q:
        got, t, first = [], 0, first0
        for i, k in enumerate(lengths):
            xs = x[t:t + k]
            d = p.power(to_dev(xs) if i % 3 else xs, every, first, bins=band)
            assert d.shape == (every_rows(k, every, first), band[1])
            got.append(d.cpu().numpy() if hasattr(d, "cpu") else d)
            if k:
                q.sdft(to_dev(xs))                       # the same samples through sdft_sdft_n
            first = every_next_first(k, every, first)
            t += k
        check(np.concatenate(got), want, bitwise, (combo, "streamed rows"))
        acc, fid, hist, cur = p.state()
        qa, qf, qh, qc = q.state()
        ra, rf, rh, rc = [np.array(v) for v in ref.state()[:3]] + [ref.state()[3]]
        assert cur == qc == rc and np.array_equal(hist, qh) and np.array_equal(hist, rh)
        if bitwise:
            assert np.array_equal(acc, qa) and np.array_equal(fid, qf) and np.array_equal(acc, ra) and np.array_equal(fid, rf)
        else:
            assert rel(acc, ra) <= 1e-10 and rel(fid, rf) <= 1e-10, (rel(acc, ra), rel(fid, rf))
        # a following hop through the reference's two calls
        hop = noise(100, seed=12, dtype=td)
        dh = p.sdft(hop)
        wh = ref.sdft(hop)
        if bitwise:
            assert np.array_equal(dh, wh)
        else:
            assert rel(dh, wh) <= 1e-11, rel(dh, wh)
        tol = 1e-6 if combo.endswith("f64") else 1e-4
        assert rel(p.isdft(dh), ref.isdft(wh)) <= tol


# ---------------------------------------------------------------------------------------------
# batched plans
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_power_batched_channels(combo):
    td = O.combo_types(combo)[0]
    ch, m, n, band = 8, 256, 10000, (17, 100)
    x = np.stack([signal(n, td, 100 + c) for c in range(ch)])
    wants = [oracle_power(O.best(m, "blackman", 1.0, combo), x[c]) for c in range(ch)]
    for device in (False, True):
        with make(m, "blackman", combo, channels=ch) as p:
            for every, first in [(100, 50), (3, 1)]:
                p.reset()
                got = p.power(to_dev(x) if device else x, every, first, bins=band)
                got = got.cpu().numpy() if device else got
                assert got.shape == (ch, wants[0][first::every].shape[0], band[1])
                assert p.get_option("last_kernel") == 5
                for c in range(ch):
                    check(got[c], on_grid(wants[c], every, first, band), exact_combo(combo), (combo, device, every, c))


# ---------------------------------------------------------------------------------------------
# pointers, async, edge cases
# ---------------------------------------------------------------------------------------------
def test_power_async_device_pointers():
    m, n = 1024, 30000
    x, want = expected("f32f64", "hann", m, n)
    dx = to_dev(x)
    with make(m, "hann", "f32f64", **{"async": 1}) as p:
        a = p.power(dx, 100, 99, bins=(0, 256))
        p.synchronize()
        check(a, on_grid(want, 100, 99, (0, 256)), False, "async, sparse grid")
        p.reset()
        b = p.power(dx[:4000], 1, 0)
        p.synchronize()
        check(b, on_grid(want[:4000], 1, 0), False, "async, dense grid")


def test_power_errors_and_edges():
    import torch
    combo, m = "f32f32", 64
    x = signal(3000, np.float32, 5)
    top = C.c_size_t(-1).value
    with make(m, "hann", combo) as p:
        ref = O.best(m, "hann", 1.0, combo)
        api = p.api
        p.power(x[:300])                                    # (errors against a plan that is mid-stream)
        ref.sdft(x[:300])
        out = np.zeros((10, m), dtype=np.float32)
        before = p.state()
        refused = [(100, 0, 0, 0, m, out.ctypes.data, "every"),                 # every == 0
                   (100, 10, 0, 0, 0, out.ctypes.data, "nbins"),                # nbins == 0
                   (100, 10, 0, 1, m, out.ctypes.data, "band"),                 # bin0 + nbins > dftsize
                   (100, 10, 0, m, 1, out.ctypes.data, "band"),
                   (100, 10, 0, 2, top, out.ctypes.data, "band"),               # bin0 + nbins overflows to 1
                   (100, 10, 0, top, 2, out.ctypes.data, "band"),
                   (100, 10, 0, 0, m, None, "NULL")]                            # rows > 0, power NULL
        for n, every, first, bin0, nb, ptr, word in refused:
            api.clear()
            assert api.sdft_power_n(p._p, n, x.ctypes.data, every, first, bin0, nb, ptr) == -1, (every, bin0, nb)
            err = api.last_error()
            assert err and "sdft_hip_sdft_power_n" in err and word in err, err
            api.clear()
            after = p.state()
            assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3], (every, bin0, nb)
        # n == 0: no rows, nothing moves
        assert api.sdft_power_n(p._p, 0, x.ctypes.data, 10, 0, 0, m, None) == 0 and api.last_error() is None
        assert p.state()[3] == before[3]
        # first >= n: no rows, the state still advances (numpy and device)
        assert p.power(x[300:700], 10, 400).shape == (0, m)
        ref.sdft(x[300:700])
        assert p.power(to_dev(x[700:1500]), 10, 5000, bins=(3, 9)).shape == (0, 9)
        ref.sdft(x[700:1500])
        ra, rf, rh, rc = ref.state()
        acc, fid, hist, cur = p.state()
        assert cur == rc and np.array_equal(acc, ra) and np.array_equal(fid, rf) and np.array_equal(hist, rh)
        # every > n: one row, at first
        d = p.power(x[1500:1900], 100000, 17, bins=(5, 40))
        w = power_of(ref.sdft(x[1500:1900]))
        assert d.shape == (1, 40) and np.array_equal(d[0], w[17, 5:45])
        # the Python wrapper refuses what the library would
        for bad in ((0, 0), (m, 1), (1, m), (-1, 2)):
            with pytest.raises(ValueError):
                p.power(x[:10], bins=bad)
    # m = 1 plan: every grid of the parity test's kind, a device tensor
    with make(1, "hann", combo) as p1:
        w1 = oracle_power(O.best(1, "hann", 1.0, combo), x)
        for every, first in [(1, 0), (1000, 999), (100000, 2999)]:
            p1.reset()
            d1 = p1.power(torch.from_numpy(x).cuda(), every, first)
            assert p1.get_option("last_kernel") == 5
            assert np.array_equal(d1.cpu().numpy(), on_grid(w1, every, first))


# ---------------------------------------------------------------------------------------------
# no overrun, no hole, at every alignment of the output an element size allows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("combo", ["f32f32", "f32f64"])
def test_power_guarded_misaligned_output(combo, host):
    """power carved from a guarded arena at every residue modulo 16 its element size allows, and at 16 mod 128; a band of 999
    bins (an odd row length: consecutive rows change alignment) on a grid of every third sample."""
    td, fd, _ = O.combo_types(combo)
    m, n, every, first, band = 1000, 2000, 3, 1, (1, 999)
    x, p_all = expected(combo, "hann", m, n)
    want = on_grid(p_all, every, first, band)
    rows = want.shape[0]
    size = np.dtype(fd).itemsize
    places = [(r, 16) for r in range(size, 16, size)] + [(16, 128)]
    assert places == ([(4, 16), (8, 16), (12, 16), (16, 128)] if size == 4 else [(8, 16), (16, 128)])
    with make(m, "hann", combo) as p:
        for r, mod in places:
            arena = (G.HostArena if host else G.DeviceArena)(G.room(((n,), td), ((rows, band[1]), fd)))
            xv = G.put(arena.carve((n,), td, np.dtype(td).itemsize, 16, name="x"), x)
            out = arena.carve((rows, band[1]), fd, r, mod, name="power")
            assert G.ptr_of(out) % mod == r
            p.reset()
            p.api.clear()
            got = p.api.sdft_power_n(p._p, n, C.c_void_p(G.ptr_of(xv)), every, first, band[0], band[1], C.c_void_p(G.ptr_of(out)))
            p.synchronize()
            assert got == rows, p.api.last_error()
            assert p.get_option("last_kernel") == 5 and p.get_option("last_chunks") > 1
            arena.check()
            assert G.view_unwritten(out) == 0
            assert np.array_equal(G.to_numpy(xv), x)
            check(G.to_numpy(out), want, exact_combo(combo), (combo, host, r, mod))


# ---------------------------------------------------------------------------------------------
# a plain C host: a band-limited spectrogram in ONE call
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,combo", [([], "f32f64"), (["-DSDFT_FD_FLOAT"], "f32f32")])
def test_c_host_power(tmp_path, hip_library, flags, combo):
    td, fd, _ = O.combo_types(combo)
    libdir = os.path.dirname(hip_library)
    rt = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    exe = tmp_path / "host_power"
    cmd = ["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), *flags,
           os.path.join(ROOT, "tests", "c", "host_power.c"), "-o", str(exe),
           "-L", libdir, "-lsdft_hip", "-L", rt, "-lamdhip64", "-lm", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{rt}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m, hop, band = 1000, 100, (0, 400)
    x = signal(48000, td, 48) * td(0.5)
    x.tofile(tmp_path / "x.raw")
    r = subprocess.run([str(exe), str(m), str(hop), str(band[0]), str(band[1]), str(tmp_path / "x.raw"), str(tmp_path / "p.raw")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "C-HOST-POWER ok" in r.stdout
    want = on_grid(oracle_power(O.best(m, "hann", 1.0, combo), x), hop, 0, band)
    got = np.fromfile(tmp_path / "p.raw", dtype=fd).reshape(-1, band[1])
    check(got, want, exact_combo(combo), "C host")
