"""Power-moments analysis (sdft_hip_sdft_power_moments_n, SDFT.power_moments) on a real MI355X against the oracle.

The call returns per window and bin the pair (s1, s2): s1 the pooled power call's sum of the powers p, s2 the sum of q = fl(p * p).
The reference for s1 is tests/test_gpu_power_sum.py's pooled(); the reference for s2 is the same summation of the oracle's powers
squared in the FD dtype (one rounded product), in the wide dtype: float64 sums for FD float; for FD double np.longdouble sums for
windows under 2048 samples, math.fsum for longer ones.

The bars are the header's promises.  With L the window's length, u = 2^-24 (float) or 2^-53 (double), gamma_L = L u / (1 - L u):
gamma_L * want on the bit-identical routes (FD float, FD double with carry = 1, calls of one time chunk) -- promise (4); the step
from gamma_(L-1) to gamma_L pays for the reference's own rounding, as in the pooled suite.  For FD double with default carries
promise (5) comes on top: L * delta for s1 and L * delta * (2 pmax + delta) for s2, delta = BAR * pmax, BAR the project's 2.1e-11
of tests/test_gpu_power.py and pmax the largest power compared.  The check is the pooled suite's check(); for s2 it is handed
pmax * (2 pmax + delta) in pmax's place, which makes its L * BAR * pmax term the bar of promise (5).

Before a GPU comparison every parity test asserts on the CPU that the reference q of the compared band is finite and that its
largest value is a normal number, so that no test passes on zeros or infinities.

Inputs are sine_sweep(n) + 0.25 noise(n), the signal of tests/test_gpu_power.py; shapes are the pooled suite's."""

import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import guarded as G
from oracle import oracle as O
from sdft_amd.sdft import every_next_first, power_sum_lengths, power_sum_rows, power_variance, spectral_kurtosis
from sdft_amd.signals import noise
from test_gpu_lag_sum import LENGTHS
from test_gpu_power import BAR, WINDOWS, bands_of, exact_combo, expected, make, oracle_power, signal, to_dev
from test_gpu_power_sum import GRIDS, check, pooled, wide, windows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = [("f32f32", {}), ("f32f64", {"carry": 1})]           # a bit-identical route of either FD type
KERNEL = 13


def numpy_of(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def squares(p):
    """q = fl(p * p) in the FD dtype"""
    q = p * p
    assert q.dtype == p.dtype
    return q


def sums_of(p, w):
    """(rows, bins) sums of the (n, bins) terms p over the windows w, in the wide dtype, as pooled() forms them"""
    hi = wide(p.dtype)
    out = np.empty((len(w), p.shape[1]), dtype=hi)
    for r, (b, e) in enumerate(w):
        if e - b == 1:
            out[r] = p[b]
        elif hi is np.float64 or e - b < 2048:
            out[r] = p[b:e].astype(hi).sum(axis=0)
        else:
            out[r] = [math.fsum(p[b:e, k]) for k in range(p.shape[1])]
    return out


@functools.lru_cache(maxsize=2)
def expected_q(combo, window, m, n):
    """the oracle's powers squared in the FD dtype; shared, never written"""
    q = squares(expected(combo, window, m, n)[1])
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=4)
def pooled2(combo, window, m, n, every, first):
    """(rows, m) reference sums of q of one shape and grid in the wide dtype; shared, never written"""
    out = sums_of(expected_q(combo, window, m, n), windows(n, every, first))
    out.setflags(write=False)
    return out


def usable(q, what):
    """the CPU precondition of a comparison: the reference q of the compared band is finite and not all zeros or subnormals"""
    assert q.size and np.isfinite(q).all(), what
    assert float(q.max()) > float(np.finfo(q.dtype).tiny), (what, float(q.max()))


def bar2(pmax, scale=1.0):
    """what check() takes for pmax so that its L * BAR * pmax is promise (5)'s L * delta * (2 pmax + delta), delta = BAR * scale *
    pmax (scale: what BAR is multiplied by on a route whose rows are held to another bar; it enters delta once)"""
    return scale * pmax * (2.0 * pmax + BAR * scale * pmax)


def check_pair(got, want1, want2, lens, exact, pmax, what, scale=1.0):
    got = numpy_of(got)
    assert got.ndim == 3 and got.shape[-1] == 2 and got.shape[:2] == want1.shape == want2.shape, (what, got.shape, want1.shape)
    check(np.ascontiguousarray(got[..., 0]), want1, lens, exact, scale * pmax, (what, "s1"))
    check(np.ascontiguousarray(got[..., 1]), want2, lens, exact, bar2(pmax, scale), (what, "s2"))


def check_band(got, combo, window, m, n, every, first, band, exact, what):
    sl = slice(band[0], band[0] + band[1])
    usable(expected_q(combo, window, m, n)[:, sl], what)
    want1, lens = pooled(combo, window, m, n, every, first)
    want2 = pooled2(combo, window, m, n, every, first)
    pmax = float(expected(combo, window, m, n)[1][:, sl].max())
    check_pair(got, want1[:, sl], want2[:, sl], lens, exact, pmax, what)


# ---------------------------------------------------------------------------------------------
# 1. parity: every type pair x window x dftsize x grid x band (promises 4 and 5)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("window", WINDOWS)
def test_power_moments_parity(combo, window):
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
                    got = p.power_moments(dx if call % 2 else x, every, first, bins=band)
                    assert p.get_option("last_kernel") == KERNEL, (m, every, first, band)
                    if m >= 1000:
                        assert p.get_option("last_chunks") > 1, (m, every, first, band)
                    assert got.shape == (power_sum_rows(n, every, first), band[1], 2)
                    check_band(got, combo, window, m, n, every, first, band, exact_combo(combo), (combo, window, m, every, first, band))
            # bins=None is the whole row
            p.reset()
            check_band(p.power_moments(x, 7, 6), combo, window, m, n, 7, 6, (0, m), exact_combo(combo), (combo, window, m, "bins=None"))


@pytest.mark.parametrize("combo", O.COMBOS)
def test_power_moments_parity_4096(combo):
    m, n = 4096, 10000
    x = expected(combo, "hann", m, n)[0]
    with make(m, "hann", combo) as p:
        for i, (every, first, band) in enumerate([(100, 37, (0, m)), (1024, 1023, (1, m - 2)), (10000, 0, (4000, 96)), (7, 6, (61, 3))]):
            p.reset()
            got = p.power_moments(to_dev(x) if i % 2 else x, every, first, bins=band)
            assert p.get_option("last_kernel") == KERNEL and p.get_option("last_chunks") > 1
            check_band(got, combo, "hann", m, n, every, first, band, exact_combo(combo), (combo, m, every, first, band))


# ---------------------------------------------------------------------------------------------
# 2. promise (2): [..., 0] is the pooled power call's output, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [{}, {"chunk": 256}], ids=["default-chunks", "chunk256"])
@pytest.mark.parametrize("combo", O.COMBOS)
def test_power_moments_first_component_is_power_sum_bit_for_bit(combo, opts):
    """promise (2): every type pair with its default carries, device pointers, every grid; both plans cut time alike because the
    call takes the pooled call's chunk choice"""
    n = 6000
    for m in (5, 125, 1024):
        x = expected(combo, "hann", m, n)[0]
        dx = to_dev(x)
        with make(m, "hann", combo, **opts) as p, make(m, "hann", combo, **opts) as q:
            bands = bands_of(m, p)
            for i, (every, first) in enumerate(GRIDS):
                band = bands[i % len(bands)]
                p.reset()
                q.reset()
                a = numpy_of(p.power_moments(dx, every, first, bins=band))
                b = numpy_of(q.power_sum(dx, every, first, bins=band))
                assert p.get_option("last_kernel") == KERNEL and q.get_option("last_kernel") == 6
                assert p.get_option("last_chunk_len") == q.get_option("last_chunk_len") and p.get_option("last_chunks") == q.get_option("last_chunks")
                assert p.get_option("last_segments") == q.get_option("last_segments")
                if opts and n > 256:
                    assert p.get_option("last_chunks") > 1
                assert a.shape == b.shape + (2,) and np.array_equal(a[..., 0], b), (combo, opts, m, every, first, band)
                assert (a[..., 1] >= 0).all() and (a[..., 1] > 0).any()


# ---------------------------------------------------------------------------------------------
# 3. promise (3): every = 1, first = 0 is the dense power call and its square, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
def test_power_moments_of_one_sample_windows_is_power_and_its_square_bit_for_bit(combo):
    """promise (3): both components against power() at every = 1 on a twin plan, which cuts time alike; on the bit-identical routes
    that is the reference's p and fl(p * p)"""
    n = 6000
    for m in (5, 125, 1024):
        x, ref = expected(combo, "hann", m, n)
        with make(m, "hann", combo) as p, make(m, "hann", combo) as q:
            for i, band in enumerate(bands_of(m, p)):
                p.reset()
                q.reset()
                xs = to_dev(x) if i % 2 else x
                a, b = numpy_of(p.power_moments(xs, 1, 0, bins=band)), numpy_of(q.power(xs, 1, 0, bins=band))
                assert p.get_option("last_kernel") == KERNEL and q.get_option("last_kernel") == 5
                assert a.shape == (n, band[1], 2) and b.shape == (n, band[1])
                assert np.array_equal(a[..., 0], b) and np.array_equal(a[..., 1], squares(b)), (combo, m, band)
                if exact_combo(combo):
                    want = ref[:, band[0]:band[0] + band[1]]
                    assert np.array_equal(a[..., 0], want) and np.array_equal(a[..., 1], squares(want)), (combo, m, band, "the reference's bits")


@pytest.mark.parametrize("combo", O.COMBOS)
def test_power_moments_of_one_sample_windows_along_a_cut_stream(combo):
    """promise (3) for a stream cut into calls (the lag suite's lengths: a call starts one sample after the roll-over): the twin
    plan's power() takes the same calls"""
    m, n, band = 1000, 6000, (10, 300)
    lengths = LENGTHS + [n - sum(LENGTHS)]
    x, ref = expected(combo, "hann", m, n)
    with make(m, "hann", combo) as p, make(m, "hann", combo) as q:
        got, terms, t = [], [], 0
        for i, k in enumerate(lengths):
            xs = x[t:t + k]
            xs = to_dev(xs) if i % 3 == 1 else xs
            got.append(numpy_of(p.power_moments(xs, 1, 0, bins=band)))
            terms.append(numpy_of(q.power(xs, 1, 0, bins=band)))
            assert got[-1].shape == (k, band[1], 2) and p.get_option("last_kernel") == KERNEL
            t += k
        got, terms = np.concatenate(got), np.concatenate(terms)
    assert np.array_equal(got[..., 0], terms) and np.array_equal(got[..., 1], squares(terms)), combo
    if exact_combo(combo):
        want = ref[:, band[0]:band[0] + band[1]]
        assert np.array_equal(got[..., 0], want) and np.array_equal(got[..., 1], squares(want))
        with make(m, "hann", combo) as r:
            assert np.array_equal(got, r.power_moments(x, 1, 0, bins=band))      # any cut of a stream: one call's bits


# ---------------------------------------------------------------------------------------------
# 4. FD double with exact carries: a bit-identical route, the bars are gamma_L alone (promise 4)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", ["f32f64", "f64f64"])
def test_power_moments_exact_carries(combo):
    n = 6000
    for m in (5, 1000):
        x, ref = expected(combo, "hann", m, n)
        band = (3, max(1, m - 5))
        with make(m, "hann", combo, carry=1) as p:
            for i, (every, first) in enumerate([(7, 6), (100, 37), (1024, 1023), (6000, 0)]):
                p.reset()
                got = p.power_moments(to_dev(x) if i % 2 else x, every, first, bins=band)
                assert p.get_option("last_chunks") > 1 and p.get_option("last_kernel") == KERNEL
                check_band(got, combo, "hann", m, n, every, first, band, True, (combo, m, every, first))
            p.reset()
            got = p.power_moments(x, 1, 0, bins=band)
            want = ref[:, band[0]:band[0] + band[1]]
            assert np.array_equal(got[..., 0], want) and np.array_equal(got[..., 1], squares(want)), (combo, m, "promise (3) with carry = 1")


# ---------------------------------------------------------------------------------------------
# 5. streaming: uneven calls, the head rows' two components added to the previous tails
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("every,first0", [(100, 37), (1024, 1023), (6000, 0), (1, 0)])
def test_power_moments_streaming(combo, every, first0):
    """the rows of a stream cut into calls (the pooled suite's lengths), head rows added on the host, hold the bars of promises (4)
    and (5) against the whole stream's windows -- the host's additions are part of the ordered sum --, and so lie within those bars
    of one long call's rows; at every = 1 on the bit-identical routes they are one call's bits"""
    m, n, band = 1000, 6000, (10, 300)
    lengths = [1, 99, 100, 511, 512, 513, 3000]
    lengths.append(n - sum(lengths))
    x = expected(combo, "hann", m, n)[0]
    bitwise = exact_combo(combo)
    with make(m, "hann", combo) as p:
        rows, t, first = [], 0, first0
        for i, k in enumerate(lengths):
            xs = x[t:t + k]
            d = numpy_of(p.power_moments(to_dev(xs) if i % 3 == 1 else xs, every, first, bins=band))
            assert d.shape == (power_sum_rows(k, every, first), band[1], 2)
            if first > 0 and t > 0:
                rows[-1] = rows[-1] + d[0]               # the head completes the previous call's last row: the host adds both components
                d = d[1:]
            rows += list(d)
            first = every_next_first(k, every, first)
            t += k
        rows = np.array(rows)
        check_band(rows, combo, "hann", m, n, every, first0, band, bitwise, (combo, every, first0, "streamed"))
    with make(m, "hann", combo) as q:
        one = q.power_moments(x, every, first0, bins=band)
        check_band(one, combo, "hann", m, n, every, first0, band, bitwise, (combo, every, first0, "one call"))
        if bitwise and every == 1:
            assert np.array_equal(rows, one)


# ---------------------------------------------------------------------------------------------
# 6. promise (6): the state afterwards is sdft's; what follows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo,opts", EXACT)
@pytest.mark.parametrize("channels", [1, 3])
def test_power_moments_leaves_the_state_of_sdft(combo, opts, channels):
    """promise (6), on the routes where sdft_sdft_n's state does not depend on how it cuts time; the band is 5 of 64 bins: the
    bins outside it stepped too"""
    td = O.combo_types(combo)[0]
    m, n, band = 64, 2000, (30, 5)
    x = np.stack([signal(n, td, 40 + c) for c in range(channels)])
    x = x[0] if channels == 1 else x
    for device, chunk in ((False, 256), (True, 200)):
        with make(m, "hann", combo, channels=channels, chunk=chunk, **opts) as p, make(m, "hann", combo, channels=channels, **opts) as q:
            p.power_moments(to_dev(x) if device else x, 100, 37, bins=band)
            assert p.get_option("last_kernel") == KERNEL and p.get_option("last_chunks") > 1
            q.sdft(x)
            sp, sq = p.state(), q.state()
            assert sp[3] == sq[3] == n % (2 * m)
            for a, b in zip(sp[:3], sq[:3]):
                assert np.array_equal(a, b), (combo, channels, device)
            hop = x[..., :100]
            assert np.array_equal(p.sdft(hop), q.sdft(hop))


@pytest.mark.parametrize("combo", O.COMBOS)
def test_power_moments_leaves_the_state_of_power_sum(combo):
    """every type pair with its default carries: the state, and a following hop, of the pooled call of the same samples, which
    cuts time alike"""
    td = O.combo_types(combo)[0]
    m, n = 1000, 6000
    x = expected(combo, "hann", m, n)[0]
    hop = noise(100, seed=12, dtype=td)
    with make(m, "hann", combo) as p, make(m, "hann", combo) as q:
        p.power_moments(to_dev(x), 100, 37, bins=(10, 300))
        q.power_sum(to_dev(x), 100, 37, bins=(10, 300))
        for a, b in zip(p.state()[:3], q.state()[:3]):
            assert np.array_equal(a, b)
        assert p.state()[3] == q.state()[3]
        assert np.array_equal(p.sdft(hop), q.sdft(hop))


# ---------------------------------------------------------------------------------------------
# 7. batched plans, chunk boundaries at 256 and at 200
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [256, 200])
@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_power_moments_batched_channels(combo, chunk):
    """every channel by itself: its single-channel bits when both plans cut time alike (chunk forced on both), and the bars against
    the oracle"""
    td = O.combo_types(combo)[0]
    ch, m, n, band = 3, 64, 2000, (17, 30)
    x = np.stack([signal(n, td, 100 + c) for c in range(ch)])
    terms = [oracle_power(O.best(m, "blackman", 1.0, combo), x[c])[:, band[0]:band[0] + band[1]] for c in range(ch)]
    for c in range(ch):
        usable(squares(terms[c]), (combo, c))
    for device in (False, True):
        for every, first in [(1, 0), (100, 37), (2000, 0)]:
            with make(m, "blackman", combo, channels=ch, chunk=chunk) as p:
                got = numpy_of(p.power_moments(to_dev(x) if device else x, every, first, bins=band))
                assert p.get_option("last_kernel") == KERNEL and p.get_option("last_chunks") > 1 and p.get_option("last_chunk_len") == chunk
                assert got.shape == (ch, power_sum_rows(n, every, first), band[1], 2)
            w = windows(n, every, first)
            for c in range(ch):
                with make(m, "blackman", combo, chunk=chunk) as q:
                    one = numpy_of(q.power_moments(to_dev(x[c]) if device else x[c], every, first, bins=band))
                assert np.array_equal(got[c], one), (combo, chunk, device, every, c)
                check_pair(got[c], sums_of(terms[c], w), sums_of(squares(terms[c]), w), [e - b for b, e in w], exact_combo(combo), float(terms[c].max()),
                           (combo, chunk, device, every, c))


# ---------------------------------------------------------------------------------------------
# 8. host staging in segments
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_power_moments_host_staging_in_segments(combo):
    """stage_bytes small enough for several segments: windows shorter than a segment, longer than one, and one over all of them;
    host samples with host and with device moments.  The segments cut windows elsewhere than the chunks of one device call, so the
    bars are promise (4)'s and (5)'s, not bits; the row count is the call's"""
    import torch
    fd = O.combo_types(combo)[1]
    m, n, band = 1000, 6000, (10, 300)
    x = expected(combo, "hann", m, n)[0]
    row = 2 * band[1] * np.dtype(fd).itemsize
    for stage, grids in [(7 * row, [(100, 37), (100, 0)]), (2 * row, [(1024, 1023), (6000, 0), (700, 0)])]:
        with make(m, "hann", combo, stage_bytes=stage) as p:
            for every, first in grids:
                rows = power_sum_rows(n, every, first)
                p.reset()
                got = p.power_moments(x, every, first, bins=band)
                assert got.shape == (rows, band[1], 2) and p.get_option("last_kernel") == KERNEL
                check_band(got, combo, "hann", m, n, every, first, band, exact_combo(combo), (combo, stage, every, first, "host"))
                p.reset()
                out = torch.zeros((rows, band[1], 2), dtype=getattr(torch, np.dtype(fd).name), device="cuda")
                ret = p.api.sdft_power_moments_n(p._p, n, C.c_void_p(x.ctypes.data), every, first, band[0], band[1], C.c_void_p(out.data_ptr()))
                p.synchronize()
                assert ret == rows, p.api.last_error()
                check_band(out, combo, "hann", m, n, every, first, band, exact_combo(combo), (combo, stage, every, first, "host samples, device moments"))


# ---------------------------------------------------------------------------------------------
# 9. async with device pointers; promise (1): the same bits on every run
# ---------------------------------------------------------------------------------------------
def test_power_moments_async_device_pointers():
    m, n = 1000, 6000
    x = expected("f32f64", "hann", m, n)[0]
    with make(m, "hann", "f32f64", **{"async": 1}) as p:
        a = p.power_moments(to_dev(x), 100, 37, bins=(0, 256))
        p.synchronize()
        assert p.get_option("last_kernel") == KERNEL
        check_band(a, "f32f64", "hann", m, n, 100, 37, (0, 256), False, "async")


@pytest.mark.parametrize("combo", ["f32f64", "f64f32"])
def test_power_moments_same_bits_on_every_run(combo):
    """promise (1)"""
    m, n = 1000, 6000
    x = expected(combo, "hann", m, n)[0]
    for device in (False, True):
        xs = to_dev(x) if device else x
        with make(m, "hann", combo) as p:
            for every, first in [(100, 37), (6000, 0)]:
                runs = []
                for _ in range(3):
                    p.reset()
                    d = p.power_moments(xs, every, first)
                    assert p.get_option("last_chunks") > 1
                    runs.append(numpy_of(d))
                assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2]), (combo, device, every, first)


def test_power_moments_statistics_from_a_call():
    """power_sum_lengths, power_variance and spectral_kurtosis on a call's output: the float64 expressions on the oracle's terms"""
    combo, m, n, every, first, band = "f32f32", 64, 6000, 100, 37, (2, 40)
    x, ref = expected(combo, "hann", m, n)
    with make(m, "hann", combo) as p:
        got = p.power_moments(to_dev(x), every, first, bins=band)
    lens = power_sum_lengths(n, every, first)
    assert lens.tolist() == [e - b for b, e in windows(n, every, first)]
    pw = ref[:, band[0]:band[0] + band[1]].astype(np.float64)
    var = np.array([pw[b:e].var(axis=0) for b, e in windows(n, every, first)])
    v = power_variance(got, lens)
    assert v.shape == var.shape and np.abs(v - var).max() <= 1e-4 * float((pw * pw).max())
    sk = spectral_kurtosis(got, lens)
    L = lens[:, None].astype(np.float64)
    s1 = np.array([pw[b:e].sum(axis=0) for b, e in windows(n, every, first)])
    s2 = np.array([(pw[b:e] ** 2).sum(axis=0) for b, e in windows(n, every, first)])
    # (s1 and s2 each within gamma_L <= 100 * 2^-24 of the exact sums, relatively; the ratio L s2 / s1^2 is at most L = 100 and
    # carries three such errors, the factor (L + 1) / (L - 1) is at most 38 / 36: 100 * 3 * 6e-6 * 1.06 < 2.5e-3)
    assert np.abs(sk - (L + 1) / (L - 1) * (L * s2 / s1 ** 2 - 1)).max() <= 2.5e-3


# ---------------------------------------------------------------------------------------------
# 10. errors leave the state alone
# ---------------------------------------------------------------------------------------------
def test_power_moments_errors():
    combo, m = "f32f32", 64
    x = signal(3000, np.float32, 5)
    top = C.c_size_t(-1).value
    with make(m, "hann", combo) as p:
        api = p.api
        p.power_moments(x[:300], 7, 3)                      # (errors against a plan that is mid-stream)
        out = np.zeros((12, m, 2), dtype=np.float32)
        before = p.state()
        refused = [(100, 0, 0, 0, m, out.ctypes.data, "every"),                 # every == 0
                   (100, 10, 0, 0, 0, out.ctypes.data, "nbins"),                # nbins == 0
                   (100, 10, 0, 1, m, out.ctypes.data, "band"),                 # bin0 + nbins > dftsize
                   (100, 10, 0, m, 1, out.ctypes.data, "band"),
                   (100, 10, 0, 2, top, out.ctypes.data, "band"),               # bin0 + nbins overflows to 1
                   (100, 10, 0, top, 2, out.ctypes.data, "band"),
                   (100, 10, 0, 0, m, None, "NULL"),                            # rows > 0, moments NULL
                   (100, 10, 5000, 0, m, None, "NULL")]                         # first >= n: the head row is a row
        for n, every, first, bin0, nb, ptr, word in refused:
            api.clear()
            assert api.sdft_power_moments_n(p._p, n, x.ctypes.data, every, first, bin0, nb, ptr) == -1, (every, bin0, nb)
            err = api.last_error()
            assert err and "sdft_hip_sdft_power_moments_n" in err and word in err, err
            api.clear()
            after = p.state()
            assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3], (every, bin0, nb)
        # the pooled call's cases in the pooled call's order and words, under the new name
        sums = np.zeros((12, m), dtype=np.float32)
        with make(m, "hann", combo) as q:
            for n, every, first, bin0, nb, ptr, _ in refused + [(100, 0, 0, 0, 0, None, ""), (100, 0, 0, m, 1, None, ""), (100, 10, 0, m, 1, None, "")]:
                api.clear()
                assert api.sdft_power_moments_n(p._p, n, x.ctypes.data, every, first, bin0, nb, ptr) == -1
                mine = api.last_error()
                api.clear()
                ptr_sum = None if ptr is None else sums.ctypes.data
                assert api.sdft_power_sum_n(q._p, n, x.ctypes.data, every, first, bin0, nb, ptr_sum) == -1
                theirs = api.last_error()
                api.clear()
                assert mine == theirs.replace("sdft_hip_sdft_power_sum_n", "sdft_hip_sdft_power_moments_n").replace("sums is NULL", "moments is NULL"), (mine, theirs)
        assert np.count_nonzero(out) == 0 and np.count_nonzero(sums) == 0
        # n == 0: no rows, nothing moves, moments may be NULL
        assert api.sdft_power_moments_n(p._p, 0, x.ctypes.data, 10, 3, 0, m, None) == 0 and api.last_error() is None
        assert p.state()[3] == before[3]
        for bad in ((0, 0), (m, 1), (1, m), (-1, 2)):
            with pytest.raises(ValueError):
                p.power_moments(x[:10], bins=bad)
        with pytest.raises(ValueError):
            p.power_moments(x[:10], every=0)
        with pytest.raises(ValueError):
            p.power_moments(x[:10], 1, 0, out=np.zeros((10, 2, m), dtype=np.float32))
        after = p.state()
        assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3]
        # out= is written in place
        mine = np.zeros((10, m, 2), dtype=np.float32)
        assert p.power_moments(x[:10], 1, 0, out=mine) is mine and (mine[..., 0] > 0).any()


# ---------------------------------------------------------------------------------------------
# 11. no overrun, no hole, at every alignment of the output an element size allows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("combo", ["f32f32", "f32f64"])
def test_power_moments_guarded_misaligned_output(combo, host):
    """moments carved from a guarded arena at every residue modulo 16 its element size allows -- an offset of one sdft_fd_t among
    them, where no pair is aligned and the vector stores' scalar fallback runs -- and at 16 mod 128; a band of 999 bins from bin 1
    (the band's edges cut lanes), windows of 7 samples after a head of 3, many of them cut by chunk boundaries"""
    td, fd, _ = O.combo_types(combo)
    m, n, every, first, band = 1000, 2000, 7, 3, (1, 999)
    x = expected(combo, "hann", m, n)[0]
    rows = power_sum_rows(n, every, first)
    size = np.dtype(fd).itemsize
    places = [(r, 16) for r in range(size, 16, size)] + [(16, 128)]
    assert (size, 16) in places
    with make(m, "hann", combo) as p:
        for r, mod in places:
            arena = (G.HostArena if host else G.DeviceArena)(G.room(((n,), td), ((rows, band[1], 2), fd)))
            xv = G.put(arena.carve((n,), td, np.dtype(td).itemsize, 16, name="x"), x)
            out = arena.carve((rows, band[1], 2), fd, r, mod, name="moments")
            assert G.ptr_of(out) % mod == r
            p.reset()
            p.api.clear()
            got = p.api.sdft_power_moments_n(p._p, n, C.c_void_p(G.ptr_of(xv)), every, first, band[0], band[1], C.c_void_p(G.ptr_of(out)))
            p.synchronize()
            assert got == rows, p.api.last_error()
            assert p.get_option("last_kernel") == KERNEL and p.get_option("last_chunks") > 1
            arena.check()
            assert G.view_unwritten(out) == 0
            assert np.array_equal(G.to_numpy(xv), x)
            check_band(G.to_numpy(out), combo, "hann", m, n, every, first, band, exact_combo(combo), (combo, host, r, mod))


# ---------------------------------------------------------------------------------------------
# 12. a plain C host and the C++ facade: a stream in blocks, head rows added to the previous tails; the Python call's bits
# ---------------------------------------------------------------------------------------------
def host_link(hip_library):
    libdir = os.path.dirname(hip_library)
    rt = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    return ["-L", libdir, "-lsdft_hip", "-L", rt, "-lamdhip64", "-lm", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{rt}"]


def python_stream(combo, m, x, every, block, band):
    """SDFT.power_moments over x in blocks, head rows added to the rows they complete"""
    n = x.size
    with make(m, "hann", combo) as p:
        rows, first = [], 0
        for t in range(0, n, block):
            k = min(block, n - t)
            d = p.power_moments(x[t:t + k], every, first, bins=band)
            if first > 0:
                rows[-1] = rows[-1] + d[0]
                d = d[1:]
            rows += list(d)
            first = every_next_first(k, every, first)
    return np.array(rows)


@pytest.mark.parametrize("flags,combo", [([], "f32f64"), (["-DSDFT_FD_FLOAT"], "f32f32")])
def test_c_host_power_moments(tmp_path, hip_library, flags, combo):
    td, fd, _ = O.combo_types(combo)
    exe = tmp_path / "host_power_moments"
    cmd = ["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), *flags,
           os.path.join(ROOT, "tests", "c", "host_power_moments.c"), "-o", str(exe), *host_link(hip_library)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    m, n, every, block, band = 1000, 6000, 100, 730, (0, 400)
    x = expected(combo, "hann", m, n)[0]
    x.tofile(tmp_path / "x.raw")
    r = subprocess.run([str(exe), str(m), str(every), str(block), str(band[0]), str(band[1]), str(tmp_path / "x.raw"), str(tmp_path / "m.raw")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "C-HOST-POWER-MOMENTS ok" in r.stdout
    got = np.fromfile(tmp_path / "m.raw", dtype=fd).reshape(-1, band[1], 2)
    check_band(got, combo, "hann", m, n, every, 0, band, exact_combo(combo), "C host")
    assert np.array_equal(got, python_stream(combo, m, x, every, block, band)), combo


def test_cpp_facade_power_moments(tmp_path, hip_library):
    """tests/cpp/host_power_moments.cpp: sdft::SDFT<T, F>::power_moments over the same blocks; the Python call's bits"""
    combo = "f32f64"
    exe = tmp_path / "host_power_moments_cpp"
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-DHOST_T=float", "-DHOST_F=double", "-I", os.path.join(ROOT, "include", "cpp"),
           os.path.join(ROOT, "tests", "cpp", "host_power_moments.cpp"), "-o", str(exe), *host_link(hip_library)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    m, n, every, block, band = 125, 1500, 100, 441, (3, 100)
    x = expected(combo, "hann", m, 6000)[0][:n]
    x.tofile(tmp_path / "x.raw")
    r = subprocess.run([str(exe), str(m), str(every), str(block), str(band[0]), str(band[1]), str(tmp_path / "x.raw"), str(tmp_path / "m.raw")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CPP-POWER-MOMENTS ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    got = np.fromfile(tmp_path / "m.raw", dtype=np.float64).reshape(-1, band[1], 2)
    assert got.shape[0] == power_sum_rows(n, every, 0)
    assert np.array_equal(got, python_stream(combo, m, np.array(x), every, block, band))
