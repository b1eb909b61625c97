"""Peak-hold analysis (sdft_hip_sdft_power_peak_n, SDFT.power_peak) on a real MI355X against the oracle.

The reference row is np.maximum.reduce (hold "max") or np.minimum.reduce (hold "min"), over the row's window, of the oracle's powers
in the FD dtype (re*re + im*im of its rows, as tests/test_gpu_power.py forms them).  The extreme of a window is one of its terms,
so on the bit-identical routes (FD float, FD double with carry = 1, calls of one time chunk) the comparison is np.array_equal,
whatever the grid, the band, the time chunks, the host staging and the cut of a stream into calls.  For FD double with default
carries the bar is sdft_hip_sdft_power_n's term deviation, 2.1e-11 of the largest power compared, with no factor for the window's
length (|max a - max b| <= max |a - b|); against sdft_hip_sdft_power_n at every = 1 on a twin plan that cuts time alike it is
np.array_equal again.

Inputs are sine_sweep(n) + 0.25 noise(n), the signal of tests/test_gpu_power.py; shapes are the pooled suite's."""

import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import guarded as G
from oracle import oracle as O
from sdft_amd.sdft import every_next_first, power_sum_rows
from sdft_amd.signals import noise
from test_gpu_power import BAR, WINDOWS, bands_of, exact_combo, expected, make, oracle_power, rel, signal, to_dev
from test_gpu_power_sum import GRIDS, windows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOLDS = ("max", "min")


def reduce_of(hold):
    return np.maximum.reduce if hold == "max" else np.minimum.reduce


def join_of(hold):
    return np.maximum if hold == "max" else np.minimum


def held_rows(p, n, every, first, hold):
    """(rows, bins) extremes of the (n, bins) powers p over the windows of a call"""
    if every == 1 and first == 0:
        return p[:n]
    red = reduce_of(hold)
    w = windows(n, every, first)
    return np.array([red(p[b:e], axis=0) for b, e in w], dtype=p.dtype).reshape(len(w), p.shape[1])


@functools.lru_cache(maxsize=8)
def held(combo, window, m, n, every, first, hold):
    """(rows, m) reference extremes of one shape and grid; shared, never written"""
    out = held_rows(expected(combo, window, m, n)[1], n, every, first, hold)
    out.setflags(write=False)
    return out


def check(got, want, exact, pmax, what):
    """bit for bit on the bit-identical routes, else |got - want| <= BAR * pmax, element by element"""
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    if want.size == 0:
        return
    if exact:
        assert np.array_equal(got, want), (what, int((got != want).sum()), float(np.abs(got - want).max()))
    else:
        err = float(np.abs(got - want).max())
        assert err <= BAR * pmax, (what, err / pmax)


def check_band(got, combo, window, m, n, every, first, band, hold, exact, what):
    want = held(combo, window, m, n, every, first, hold)
    pmax = float(expected(combo, window, m, n)[1][:, band[0]:band[0] + band[1]].max())
    check(got, want[:, band[0]:band[0] + band[1]], exact, pmax, what)


# ---------------------------------------------------------------------------------------------
# 1. parity: every type pair x window x dftsize x grid x band x hold
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("window", WINDOWS)
def test_power_peak_parity(combo, window, hold):
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
                    got = p.power_peak(dx if call % 2 else x, every, first, bins=band, hold=hold)
                    assert p.get_option("last_kernel") == 11, (m, every, first, band)
                    if m >= 1000:
                        assert p.get_option("last_chunks") > 1, (m, every, first, band)
                    assert got.shape == (power_sum_rows(n, every, first), band[1])
                    check_band(got, combo, window, m, n, every, first, band, hold, exact_combo(combo), (combo, window, m, every, first, band, hold))
            # bins=None is the whole row, and the enum's number is the name
            p.reset()
            check_band(p.power_peak(x, 7, 6, hold=HOLDS.index(hold)), combo, window, m, n, 7, 6, (0, m), hold, exact_combo(combo), (combo, window, m, "bins=None"))


@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("combo", O.COMBOS)
def test_power_peak_parity_4096(combo, hold):
    m, n = 4096, 10000
    x = expected(combo, "hann", m, n)[0]
    with make(m, "hann", combo) as p:
        for i, (every, first, band) in enumerate([(100, 37, (0, m)), (1024, 1023, (1, m - 2)), (10000, 0, (4000, 96)), (7, 6, (61, 3))]):
            p.reset()
            got = p.power_peak(to_dev(x) if i % 2 else x, every, first, bins=band, hold=hold)
            assert p.get_option("last_kernel") == 11 and p.get_option("last_chunks") > 1
            check_band(got, combo, "hann", m, n, every, first, band, hold, exact_combo(combo), (combo, m, every, first, band, hold))


# ---------------------------------------------------------------------------------------------
# 2. FD double with exact carries: a bit-identical route
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("combo", ["f32f64", "f64f64"])
def test_power_peak_exact_carries(combo, hold):
    n = 6000
    for m in (5, 1000):
        x = expected(combo, "hann", m, n)[0]
        band = (3, max(1, m - 5))
        with make(m, "hann", combo, carry=1) as p:
            for i, (every, first) in enumerate([(7, 6), (100, 37), (1024, 1023), (6000, 0)]):
                p.reset()
                got = p.power_peak(to_dev(x) if i % 2 else x, every, first, bins=band, hold=hold)
                assert p.get_option("last_chunks") > 1 and p.get_option("last_kernel") == 11
                check_band(got, combo, "hann", m, n, every, first, band, hold, True, (combo, m, every, first, hold))


# ---------------------------------------------------------------------------------------------
# 3. windows of one sample are the dense power call, bit for bit; 4. FD double default carries against that call
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
def test_power_peak_of_one_sample_windows_is_power_bit_for_bit(combo):
    n = 6000
    for m in (5, 125, 1024):
        x = expected(combo, "hann", m, n)[0]
        with make(m, "hann", combo) as p, make(m, "hann", combo) as q:
            for i, band in enumerate(bands_of(m, p)):
                q.reset()
                xs = to_dev(x) if i % 2 else x
                b = q.power(xs, 1, 0, bins=band)
                b = b.cpu().numpy() if i % 2 else b
                assert q.get_option("last_kernel") == 5
                for hold in HOLDS:
                    p.reset()
                    a = p.power_peak(xs, 1, 0, bins=band, hold=hold)
                    a = a.cpu().numpy() if i % 2 else a
                    assert p.get_option("last_kernel") == 11
                    assert a.shape == b.shape == (n, band[1]) and np.array_equal(a, b), (combo, m, band, hold)


@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("combo", ["f32f64", "f64f64"])
def test_power_peak_default_carries_hold_the_dense_calls_terms(combo, hold):
    """FD double, fast carries: not the reference's bits, but exactly the extreme of what power() at every = 1 stores when both
    calls cut time into chunks of the same length"""
    m, n, band = 1000, 6000, (1, 998)
    x = expected(combo, "hann", m, n)[0]
    for device in (False, True):
        xs = to_dev(x) if device else x
        with make(m, "hann", combo) as p, make(m, "hann", combo) as q:
            terms = q.power(xs, 1, 0, bins=band)
            terms = terms.cpu().numpy() if device else terms
            for every, first in [(100, 0), (100, 37), (6000, 0)]:
                p.reset()
                got = p.power_peak(xs, every, first, bins=band, hold=hold)
                got = got.cpu().numpy() if device else got
                assert p.get_option("last_chunk_len") == q.get_option("last_chunk_len") and p.get_option("last_chunks") == q.get_option("last_chunks") > 1
                assert np.array_equal(got, held_rows(terms, n, every, first, hold)), (combo, device, every, first, hold)
                check_band(got, combo, "hann", m, n, every, first, band, hold, False, (combo, device, every, first, hold, "against the oracle"))


# ---------------------------------------------------------------------------------------------
# 5. the bits do not depend on how time is cut into chunks, nor on the carries' route; the same bits on every run
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("combo", ["f32f32", "f32f64"])
def test_power_peak_chunk_independence(combo, hold):
    m, n, band = 1000, 6000, (1, 998)
    x = expected(combo, "hann", m, n)[0]
    base = dict(carry=1) if combo == "f32f64" else {}
    routes = [dict(), dict(chunk=128), dict(chunk=1000), dict(segments=3), dict(chain=2), dict(chain=0)]
    for every, first in [(100, 37), (6000, 0)]:
        seen, lens = [], set()
        for opts in routes:
            with make(m, "hann", combo, **base, **opts) as p:
                got = p.power_peak(to_dev(x), every, first, bins=band, hold=hold)
                assert p.get_option("last_chunks") > 1 and p.get_option("last_kernel") == 11
                lens.add(p.get_option("last_chunk_len"))
                seen.append(got.cpu().numpy())
                check_band(seen[-1], combo, "hann", m, n, every, first, band, hold, True, (combo, opts, every, first, hold))
        assert len(lens) >= 2, lens                                 # (the chunks did differ)
        assert all(np.array_equal(seen[0], s) for s in seen[1:])


@pytest.mark.parametrize("combo", ["f32f64", "f64f32"])
def test_power_peak_same_bits_on_every_run(combo):
    m, n = 1000, 6000
    x = expected(combo, "hann", m, n)[0]
    for device in (False, True):
        xs = to_dev(x) if device else x
        with make(m, "hann", combo) as p:
            for every, first, hold in [(100, 37, "max"), (6000, 0, "min")]:
                runs = []
                for _ in range(3):
                    p.reset()
                    d = p.power_peak(xs, every, first, hold=hold)
                    assert p.get_option("last_chunks") > 1
                    runs.append(d.cpu().numpy() if device else d)
                assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2]), (combo, device, every, first)


# ---------------------------------------------------------------------------------------------
# 6. row counts
# ---------------------------------------------------------------------------------------------
def test_power_peak_row_counts():
    combo, m = "f32f32", 64
    x = signal(6000, np.float32, 3)
    with make(m, "hann", combo) as p:
        for i, (every, first) in enumerate(GRIDS):
            for n in (0, 1, 37, 38, 511, 6000):
                p.reset()
                got = p.power_peak(x[:n], every, first, bins=(3, 5), hold=HOLDS[i % 2])
                assert got.shape == (power_sum_rows(n, every, first), 5) == (len(windows(n, every, first)), 5), (n, every, first)
                assert (got.shape[0] == 0) == (n == 0)
        # the C call answers the same count
        out = np.zeros((70, m), dtype=np.float32)
        for i, (every, first) in enumerate(GRIDS):
            rows = power_sum_rows(3000, every, first)
            if rows <= out.shape[0]:
                p.reset()
                assert p.api.sdft_power_peak_n(p._p, 3000, x.ctypes.data, every, first, 0, m, i % 2, out.ctypes.data) == rows, (every, first)


# ---------------------------------------------------------------------------------------------
# 7. streaming: uneven calls, head rows joined to the previous tails by the rule; 8. state; what follows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("every,first0", [(100, 37), (1024, 1023), (6000, 0)])
def test_power_peak_streaming(combo, every, first0, hold):
    """the rows of a stream cut into calls are one long call's: bit for bit the reference's on the bit-identical routes (so equal
    to one long call's, which is checked too); with FD double's fast carries, whose rounding depends on the call lengths, within
    the bar of the reference like the long call itself"""
    m, n, band = 1000, 6000, (10, 300)
    lengths = [1, 99, 100, 511, 512, 513, 3000]
    lengths.append(n - sum(lengths))
    x = expected(combo, "hann", m, n)[0]
    ref = O.best(m, "hann", 1.0, combo)
    for t in range(0, n, 2048):
        ref.sdft(x[t:t + 2048])
    bitwise = exact_combo(combo)
    join = join_of(hold)
    with make(m, "hann", combo) as p:
        rows, t, first = [], 0, first0
        for i, k in enumerate(lengths):
            xs = x[t:t + k]
            d = p.power_peak(to_dev(xs) if i % 3 == 1 else xs, every, first, bins=band, hold=hold)
            d = d.cpu().numpy() if hasattr(d, "cpu") else d
            assert d.shape == (power_sum_rows(k, every, first), band[1])
            if first > 0 and t > 0:
                rows[-1] = join(rows[-1], d[0])          # the head completes the previous call's last row: the host joins the two
                d = d[1:]
            rows += list(d)
            first = every_next_first(k, every, first)
            t += k
        rows = np.array(rows)
        check_band(rows, combo, "hann", m, n, every, first0, band, hold, bitwise, (combo, every, first0, hold, "streamed"))
        acc, fid, hist, cur = p.state()
        ra, rf, rh, rc = [np.array(v) for v in ref.state()[:3]] + [ref.state()[3]]
        assert cur == rc and np.array_equal(hist, rh)
        if bitwise:
            assert np.array_equal(acc, ra) and np.array_equal(fid, rf)
        else:
            assert rel(acc, ra) <= 1e-10 and rel(fid, rf) <= 1e-10, (rel(acc, ra), rel(fid, rf))
    if bitwise:
        with make(m, "hann", combo) as q:
            assert np.array_equal(rows, q.power_peak(x, every, first0, bins=band, hold=hold))


@pytest.mark.parametrize("combo", O.COMBOS)
def test_power_peak_leaves_the_state_of_power(combo):
    """after a peak-hold call a following sdft_n or isdft_n continues as after power of the same samples"""
    td = O.combo_types(combo)[0]
    m, n = 1000, 6000
    x = expected(combo, "hann", m, n)[0]
    hop = noise(100, seed=12, dtype=td)
    for device, hold in ((False, "max"), (True, "min")):
        with make(m, "hann", combo) as p, make(m, "hann", combo) as q:
            xs = to_dev(x) if device else x
            p.power_peak(xs, 100, 37, bins=(10, 300), hold=hold)
            q.power(xs, 1, 0, bins=(10, 300))                # the twin forms the same terms and cuts time alike
            for a, b in zip(p.state()[:3], q.state()[:3]):
                assert np.array_equal(a, b)
            assert p.state()[3] == q.state()[3]
            dp, dq = p.sdft(hop), q.sdft(hop)
            assert np.array_equal(dp, dq)
            assert np.array_equal(p.isdft(dp), q.isdft(dq))


# ---------------------------------------------------------------------------------------------
# 9. batched plans, 10. host staging, 11. async
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_power_peak_batched_channels(combo, hold):
    td = O.combo_types(combo)[0]
    ch, m, n, band = 3, 64, 3000, (17, 30)
    x = np.stack([signal(n, td, 100 + c) for c in range(ch)])
    terms = [oracle_power(O.best(m, "blackman", 1.0, combo), x[c])[:, band[0]:band[0] + band[1]] for c in range(ch)]
    for device in (False, True):
        with make(m, "blackman", combo, channels=ch) as p:
            for every, first in [(100, 37), (3000, 0)]:
                p.reset()
                got = p.power_peak(to_dev(x) if device else x, every, first, bins=band, hold=hold)
                got = got.cpu().numpy() if device else got
                assert p.get_option("last_kernel") == 11 and p.get_option("last_chunks") > 1
                assert got.shape == (ch, power_sum_rows(n, every, first), band[1])
                for c in range(ch):
                    check(got[c], held_rows(terms[c], n, every, first, hold), exact_combo(combo), float(terms[c].max()), (combo, device, every, hold, c))


@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_power_peak_host_staging_in_segments(combo, hold):
    """stage_bytes small enough for several segments: windows shorter than a segment, longer than one, and one over all of them;
    host samples with host and with device peaks"""
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
                check_band(p.power_peak(x, every, first, bins=band, hold=hold), combo, "hann", m, n, every, first, band, hold, exact_combo(combo),
                           (combo, stage, every, first, hold, "host"))
                p.reset()
                out = torch.zeros((rows, band[1]), dtype=getattr(torch, np.dtype(fd).name), device="cuda")
                got = p.api.sdft_power_peak_n(p._p, n, C.c_void_p(x.ctypes.data), every, first, band[0], band[1], HOLDS.index(hold), C.c_void_p(out.data_ptr()))
                p.synchronize()
                assert got == rows, p.api.last_error()
                check_band(out, combo, "hann", m, n, every, first, band, hold, exact_combo(combo), (combo, stage, every, first, hold, "host samples, device peaks"))


@pytest.mark.parametrize("hold", HOLDS)
def test_power_peak_async_device_pointers(hold):
    m, n = 1000, 6000
    x = expected("f32f64", "hann", m, n)[0]
    with make(m, "hann", "f32f64", **{"async": 1}) as p:
        a = p.power_peak(to_dev(x), 100, 37, bins=(0, 256), hold=hold)
        p.synchronize()
        check_band(a, "f32f64", "hann", m, n, 100, 37, (0, 256), hold, False, "async")


# ---------------------------------------------------------------------------------------------
# 12. a NaN sample: the window that holds it and every later one is NaN, as the dense call's terms say; earlier rows are finite
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("m,n,at,opts", [(64, 500, 250, {}), (1000, 6000, 3000, dict(chain=0))], ids=["one-chunk", "serial-carries"])
def test_power_peak_nan_rule(m, n, at, opts, hold):
    """relative to power() on a twin plan, not to the oracle: the rule makes a window with a NaN term NaN, whatever the order"""
    combo, every, first = "f32f32", 100, 37
    x = np.array(expected(combo, "hann", m, n)[0])
    x[at] = np.nan
    with make(m, "hann", combo, **opts) as p, make(m, "hann", combo, **opts) as q:
        terms = q.power(x, 1, 0)
        got = p.power_peak(x, every, first, hold=hold)
        assert (p.get_option("last_chunks") > 1) == (n > 512) and p.get_option("last_kernel") == 11
        assert np.array_equal(got, held_rows(terms, n, every, first, hold), equal_nan=True)
        w = windows(n, every, first)
        before = [r for r, (b, e) in enumerate(w) if e <= at]
        assert before and np.isfinite(got[before]).all()
        assert np.isnan(got).all(axis=1).any()


# ---------------------------------------------------------------------------------------------
# 13. errors leave the state alone
# ---------------------------------------------------------------------------------------------
def test_power_peak_errors():
    combo, m = "f32f32", 64
    x = signal(3000, np.float32, 5)
    top = C.c_size_t(-1).value
    with make(m, "hann", combo) as p:
        api = p.api
        p.power_peak(x[:300], 7, 3)                         # (errors against a plan that is mid-stream)
        out = np.zeros((12, m), dtype=np.float32)
        before = p.state()
        refused = [(100, 0, 0, 0, m, 0, out.ctypes.data, "every"),              # every == 0
                   (100, 10, 0, 0, 0, 1, out.ctypes.data, "nbins"),             # nbins == 0
                   (100, 10, 0, 1, m, 0, out.ctypes.data, "band"),              # bin0 + nbins > dftsize
                   (100, 10, 0, m, 1, 1, out.ctypes.data, "band"),
                   (100, 10, 0, 2, top, 0, out.ctypes.data, "band"),            # bin0 + nbins overflows to 1
                   (100, 10, 0, top, 2, 1, out.ctypes.data, "band"),
                   (100, 10, 0, 0, m, 0, None, "NULL"),                         # rows > 0, peaks NULL
                   (100, 10, 5000, 0, m, 1, None, "NULL"),                      # first >= n: the head row is a row
                   (100, 10, 0, 0, m, 2, out.ctypes.data, "hold"),              # hold is neither 0 nor 1
                   (100, 10, 0, 0, m, -1, out.ctypes.data, "hold"),
                   (0, 10, 0, 0, m, 7, None, "hold")]                           # ... even for a call without samples
        for n, every, first, bin0, nb, hold, ptr, word in refused:
            api.clear()
            assert api.sdft_power_peak_n(p._p, n, x.ctypes.data, every, first, bin0, nb, hold, ptr) == -1, (every, bin0, nb, hold)
            err = api.last_error()
            assert err and "sdft_hip_sdft_power_peak_n" in err and word in err, err
            api.clear()
            after = p.state()
            assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3], (every, bin0, nb, hold)
        assert np.count_nonzero(out) == 0
        # n == 0: no rows, nothing moves, peaks may be NULL
        assert api.sdft_power_peak_n(p._p, 0, x.ctypes.data, 10, 3, 0, m, 1, None) == 0 and api.last_error() is None
        assert p.state()[3] == before[3]
        for bad in ((0, 0), (m, 1), (1, m), (-1, 2)):
            with pytest.raises(ValueError):
                p.power_peak(x[:10], bins=bad)
        with pytest.raises(ValueError):
            p.power_peak(x[:10], every=0)
        for bad in (2, -1, "peak", None):
            with pytest.raises(ValueError):
                p.power_peak(x[:10], hold=bad)
        after = p.state()
        assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3]


# ---------------------------------------------------------------------------------------------
# 14. no overrun, no hole, at every alignment of the output an element size allows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("combo", ["f32f32", "f32f64"])
def test_power_peak_guarded_misaligned_output(combo, host, hold):
    """peaks carved from a guarded arena at every residue modulo 16 its element size allows, and at 16 mod 128; a band of 999
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
            out = arena.carve((rows, band[1]), fd, r, mod, name="peaks")
            assert G.ptr_of(out) % mod == r
            p.reset()
            p.api.clear()
            got = p.api.sdft_power_peak_n(p._p, n, C.c_void_p(G.ptr_of(xv)), every, first, band[0], band[1], HOLDS.index(hold), C.c_void_p(G.ptr_of(out)))
            p.synchronize()
            assert got == rows, p.api.last_error()
            assert p.get_option("last_kernel") == 11 and p.get_option("last_chunks") > 1
            arena.check()
            assert G.view_unwritten(out) == 0
            assert np.array_equal(G.to_numpy(xv), x)
            check_band(G.to_numpy(out), combo, "hann", m, n, every, first, band, hold, exact_combo(combo), (combo, host, r, mod, hold))


# ---------------------------------------------------------------------------------------------
# 15. a plain C host: a stream in blocks, head rows joined to the previous tails by the rule
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,combo", [([], "f32f64"), (["-DSDFT_FD_FLOAT"], "f32f32")])
def test_c_host_power_peak(tmp_path, hip_library, flags, combo):
    td, fd, _ = O.combo_types(combo)
    libdir = os.path.dirname(hip_library)
    rt = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    exe = tmp_path / "host_power_peak"
    cmd = ["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), *flags,
           os.path.join(ROOT, "tests", "c", "host_power_peak.c"), "-o", str(exe),
           "-L", libdir, "-lsdft_hip", "-L", rt, "-lamdhip64", "-lm", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{rt}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m, n, every, block, band = 1000, 6000, 100, 730, (0, 400)
    x = expected(combo, "hann", m, n)[0]
    x.tofile(tmp_path / "x.raw")
    for hold in HOLDS:
        r = subprocess.run([str(exe), str(m), str(every), str(block), str(band[0]), str(band[1]), str(HOLDS.index(hold)), str(tmp_path / "x.raw"),
                            str(tmp_path / "p.raw")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        assert "C-HOST-POWER-PEAK ok" in r.stdout
        got = np.fromfile(tmp_path / "p.raw", dtype=fd).reshape(-1, band[1])
        check_band(got, combo, "hann", m, n, every, 0, band, hold, exact_combo(combo), ("C host", hold))
        # the Python call in the same blocks: the same bits
        with make(m, "hann", combo) as p:
            rows, first = [], 0
            for t in range(0, n, block):
                k = min(block, n - t)
                d = p.power_peak(x[t:t + k], every, first, bins=band, hold=hold)
                if first > 0:
                    rows[-1] = join_of(hold)(rows[-1], d[0])
                    d = d[1:]
                rows += list(d)
                first = every_next_first(k, every, first)
            assert np.array_equal(got, np.array(rows)), (combo, hold)
