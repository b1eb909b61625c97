"""Decimated analysis (sdft_hip_sdft_every_n, SDFT.sdft_every) on a real MI355X against the oracle.

The oracle is fed in blocks and only the grid's rows are kept, so no full matrix is built on the host.  Bars: bit-identical
wherever sdft_sdft_n is (FD float with its default exact carries, FD double with carry = 1, calls of one time chunk), else
1e-11 relative to the largest bin, the bar of the chunk-parallel analysis tests."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from sdft_amd.signals import noise, sine_sweep

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-11


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.size == 0 and b.size == 0:
        return 0.0
    scale = float(np.abs(b).max())
    return float(np.abs(a - b).max()) / (scale if scale > 0 else 1.0)


def make(m, window="hann", combo="f32f64", channels=1, **opts):
    from sdft_amd.sdft import SDFT
    p = SDFT(m, window, 1.0, combo, channels)
    for k, v in opts.items():
        p.set_option(k, v)
    return p


def grid_first(t0, every, first):
    """first of the grid relative to sample t0 (the grid's first sample at or after t0, minus t0)"""
    if first >= t0:
        return first - t0
    past = (t0 - first) % every
    return every - past if past else 0


def oracle_rows(ref, x, grids, block=2048, limit=None):
    """{(every, first): rows of the oracle's matrix at first, first + every, ... < len(x) (or < limit[grid])}; one pass"""
    out = {g: [] for g in grids}
    for t in range(0, x.size, block):
        d = ref.sdft(x[t:t + block])
        for (every, first) in grids:
            end = min(d.shape[0], (limit or {}).get((every, first), x.size) - t)
            if end <= 0:
                continue
            idx = np.arange(grid_first(t, every, first), end, every)
            if idx.size:
                out[(every, first)].append(d[idx].copy())
    m = ref.dftsize
    return {g: (np.concatenate(v) if v else np.empty((0, m), dtype=ref.fdx)) for g, v in out.items()}


def exact_combo(combo):
    return combo.endswith("f32")


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check(got, want, bitwise, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if bitwise:
        assert np.array_equal(got, want), (what, rel(got, want))
    else:
        assert rel(got, want) <= BAR, (what, rel(got, want))


# ---------------------------------------------------------------------------------------------
# parity: every type pair x window x dftsize x grid
# ---------------------------------------------------------------------------------------------
MS = (1, 2, 3, 5, 8, 64, 1000, 1024, 2048, 4096)
EVERYS = (1, 7, 100, 1024)


@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("window", ["boxcar", "hann", "hamming", "blackman"])
def test_every_parity(combo, window):
    td = O.combo_types(combo)[0]
    for m in MS:
        n = 20000 if m <= 64 else (12000 if m <= 1024 else 6000)
        n1 = n if m <= 64 else (2048 if m <= 1024 else 1024)         # every = 1: rows are the matrix, kept short
        x = sine_sweep(n).astype(td) + noise(n, seed=m, dtype=td) * td(0.25)
        grids = sorted({(e, f) for e in EVERYS for f in (0, e - 1)} | {(1, 3)})
        limit = {g: n1 for g in grids if g[0] == 1}
        want = oracle_rows(O.best(m, window, 1.0, combo), x, grids, limit=limit)
        with make(m, window, combo) as p:
            for i, (every, first) in enumerate(grids):
                xs = x[:limit.get((every, first), n)]
                p.reset()
                got = p.sdft_every(to_dev(xs) if i % 2 else xs, every, first)
                if not (every == 1 and first == 0):
                    assert p.get_option("last_kernel") == 4, (m, every, first)
                check(got, want[(every, first)], exact_combo(combo), (combo, window, m, every, first))


@pytest.mark.parametrize("combo", ["f32f64", "f64f64"])
@pytest.mark.parametrize("window", ["hann", "blackman"])
def test_every_exact_carries_bit_identical(combo, window):
    """FD double with option carry = 1: the exact carries (relay or serial pass) feed the kernel, the rows are the reference's bits."""
    td = O.combo_types(combo)[0]
    for m in (5, 1000, 1024):
        n = 12000
        x = noise(n, seed=7 + m, dtype=td)
        grids = [(7, 6), (100, 0), (1024, 1023)]
        want = oracle_rows(O.best(m, window, 1.0, combo), x, grids)
        with make(m, window, combo, carry=1) as p:
            for every, first in grids:
                p.reset()
                got = p.sdft_every(to_dev(x), every, first)
                assert p.get_option("last_chunks") > 1
                check(got, want[(every, first)], True, (combo, window, m, every, first))


@pytest.mark.parametrize("combo", O.COMBOS)
def test_every_one_chunk_bit_identical(combo):
    td = O.combo_types(combo)[0]
    for m in (1, 64, 1000):
        x = noise(500, seed=m, dtype=td)
        grids = [(7, 6), (100, 0), (1, 5)]
        want = oracle_rows(O.best(m, "hann", 1.0, combo), x, grids)
        with make(m, "hann", combo) as p:
            for every, first in grids:
                p.reset()
                got = p.sdft_every(x, every, first)
                assert p.get_option("last_chunks") == 1 and p.get_option("last_kernel") == 4
                check(got, want[(every, first)], True, (combo, m, every, first))


# ---------------------------------------------------------------------------------------------
# streaming: uneven calls, first carried as documented; state; a following hop
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
def test_every_streaming_state_and_next_hop(combo):
    from sdft_amd.sdft import every_next_first, every_rows
    td = O.combo_types(combo)[0]
    m, every, first0 = 1000, 100, 37
    lengths = [100, 3000, 37, 700, 5000, 1, 511, 512, 2600, 9000, 0, 64]
    x = noise(sum(lengths), seed=11, dtype=td)
    ref = O.best(m, "hann", 1.0, combo)
    want = oracle_rows(ref, x, [(every, first0)])[(every, first0)]
    bitwise = exact_combo(combo)
    with make(m, "hann", combo) as p, make(m, "hann", combo) as q:
        got, t, first = [], 0, first0
        for i, k in enumerate(lengths):
            xs = x[t:t + k]
            d = p.sdft_every(to_dev(xs) if i % 3 else xs, every, first)
            assert d.shape[0] == every_rows(k, every, first)
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
        check(dh, wh, bitwise, (combo, "next hop"))
        tol = 1e-6 if combo.endswith("f64") else 1e-4
        assert rel(p.isdft(dh), ref.isdft(wh)) <= tol


# ---------------------------------------------------------------------------------------------
# batched plans
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_every_batched_channels(combo):
    td = O.combo_types(combo)[0]
    ch, m, n, every, first = 8, 256, 10000, 100, 50
    x = np.stack([noise(n, seed=100 + c, dtype=td) for c in range(ch)])
    wants = [oracle_rows(O.best(m, "blackman", 1.0, combo), x[c], [(every, first)])[(every, first)] for c in range(ch)]
    for device in (False, True):
        with make(m, "blackman", combo, channels=ch) as p:
            got = p.sdft_every(to_dev(x) if device else x, every, first)
            got = got.cpu().numpy() if device else got
            assert got.shape == (ch, wants[0].shape[0], m)
            for c in range(ch):
                check(got[c], wants[c], exact_combo(combo), (combo, device, c))


# ---------------------------------------------------------------------------------------------
# pointers, async, edge cases, no overrun
# ---------------------------------------------------------------------------------------------
def test_every_async_device_pointers():
    m, n, every, first = 1024, 30000, 100, 99
    x = noise(n, seed=21, dtype=np.float32)
    want = oracle_rows(O.best(m, "hann", 1.0, "f32f64"), x, [(every, first)])[(every, first)]
    with make(m, "hann", "f32f64", **{"async": 1}) as p:
        got = p.sdft_every(to_dev(x), every, first)
        p.synchronize()
        check(got, want, False, "async")


def test_every_edge_cases():
    import torch
    combo, m = "f32f32", 64
    x = noise(3000, seed=5, dtype=np.float32)
    with make(m, "hann", combo) as p:
        ref = O.best(m, "hann", 1.0, combo)
        api = p.api
        out = np.zeros((10, m), dtype=np.complex64)
        before = p.state()
        api.clear()
        assert api.sdft_every_n(p._p, 100, x.ctypes.data, 0, 0, out.ctypes.data) == -1      # every == 0
        assert "every" in api.last_error()
        api.clear()
        assert api.sdft_every_n(p._p, 100, x.ctypes.data, 10, 0, None) == -1                # rows > 0, dfts NULL
        api.clear()
        after = p.state()
        assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3]
        # n == 0: no rows, nothing moves
        assert api.sdft_every_n(p._p, 0, x.ctypes.data, 10, 0, None) == 0
        assert p.state()[3] == 0
        # first >= n: no rows, the state still advances (numpy and device)
        assert p.sdft_every(x[:700], 10, 700).shape == (0, m)
        ref.sdft(x[:700])
        assert p.sdft_every(to_dev(x[700:1500]), 10, 5000).shape[0] == 0
        ref.sdft(x[700:1500])
        ra, rf, rh, rc = ref.state()
        acc, fid, hist, cur = p.state()
        assert cur == rc and np.array_equal(acc, ra) and np.array_equal(fid, rf) and np.array_equal(hist, rh)
        # every > n: one row, at first
        d = p.sdft_every(x[1500:1900], 100000, 17)
        w = ref.sdft(x[1500:1900])
        assert d.shape == (1, m) and np.array_equal(d[0], w[17])
        # m = 1 plan, every > n and a device tensor
        with make(1, "hann", combo) as p1:
            r1 = O.best(1, "hann", 1.0, combo)
            d1 = p1.sdft_every(torch.from_numpy(x).cuda(), 1000, 999)
            w1 = oracle_rows(r1, x, [(1000, 999)])[(1000, 999)]
            assert np.array_equal(d1.cpu().numpy(), w1)


@pytest.mark.parametrize("device", [False, True])
def test_every_no_overrun(device):
    """A sentinel-filled output larger than rows x m is untouched past the last row."""
    import torch
    m, n, every, first = 1000, 20000, 100, 42
    x = noise(n, seed=31, dtype=np.float32)
    rows = (n - first + every - 1) // every
    want = oracle_rows(O.best(m, "hamming", 1.0, "f32f64"), x, [(every, first)])[(every, first)]
    sentinel = np.complex128(complex(-7.25e300, 3.5e-300))
    buf = np.full((rows + 7) * m, sentinel, dtype=np.complex128)
    with make(m, "hamming", "f32f64") as p:
        if device:
            dbuf, dx = torch.from_numpy(buf).cuda(), torch.from_numpy(x).cuda()
            got = p.api.sdft_every_n(p._p, n, C.c_void_p(dx.data_ptr()), every, first, C.c_void_p(dbuf.data_ptr()))
            torch.cuda.synchronize()
            res = dbuf.cpu().numpy()
        else:
            got = p.api.sdft_every_n(p._p, n, C.c_void_p(x.ctypes.data), every, first, C.c_void_p(buf.ctypes.data))
            res = buf
        assert got == rows, p.api.last_error()
        assert np.all(res[rows * m:] == sentinel)
        check(res[:rows * m].reshape(rows, m), want, False, ("no overrun", device))


# ---------------------------------------------------------------------------------------------
# full size
# ---------------------------------------------------------------------------------------------
def test_every_full_size_configs1():
    """n = 1e6, m = 1024, Hann, FD double (configs[1]), every = 100: all 10 000 rows against the oracle."""
    n, m, every = 1_000_000, 1024, 100
    x = sine_sweep(n).astype(np.float32)
    want = oracle_rows(O.best(m, "hann", 1.0, "f32f64"), x, [(every, 0)], block=4096)[(every, 0)]
    assert want.shape == (10000, m)
    with make(m, "hann", "f32f64") as p:
        got = p.sdft_every(to_dev(x), every, 0)
        assert p.get_option("last_kernel") == 4
        check(got, want, False, "configs[1]")


def test_every_full_size_configs2_bit_identical():
    """configs[2] shape: m = 4096, Blackman, FD float, n = 262 144, every = 256: bit-identical."""
    n, m, every = 262_144, 4096, 256
    x = sine_sweep(n).astype(np.float32)
    want = oracle_rows(O.best(m, "blackman", 1.0, "f32f32"), x, [(every, 0)], block=1024)[(every, 0)]
    with make(m, "blackman", "f32f32") as p:
        got = p.sdft_every(to_dev(x), every, 0)
        check(got, want, True, "configs[2]")


# ---------------------------------------------------------------------------------------------
# a plain C host: the reference driver's kept rows in ONE call
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,combo", [([], "f32f64"), (["-DSDFT_FD_FLOAT"], "f32f32")])
def test_c_host_every(tmp_path, hip_library, flags, combo):
    td, fd, fdx = O.combo_types(combo)
    libdir = os.path.dirname(hip_library)
    rt = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    exe = tmp_path / "host_every"
    cmd = ["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), *flags,
           os.path.join(ROOT, "tests", "c", "host_every.c"), "-o", str(exe),
           "-L", libdir, "-lsdft_hip", "-L", rt, "-lamdhip64", "-lm", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{rt}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m, hop = 1000, 100
    x = (sine_sweep(48000) * 0.5).astype(td)
    x.tofile(tmp_path / "x.raw")
    r = subprocess.run([str(exe), str(m), str(hop), str(tmp_path / "x.raw"), str(tmp_path / "d.raw")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "C-HOST-EVERY ok" in r.stdout
    want = oracle_rows(O.best(m, "hann", 1.0, combo), x, [(hop, 0)])[(hop, 0)]
    got = np.fromfile(tmp_path / "d.raw", dtype=fdx).reshape(-1, m)
    check(got, want, exact_combo(combo), "C host")
