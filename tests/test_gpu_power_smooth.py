"""Smoothed power analysis (sdft_hip_sdft_power_smooth_n, SDFT.power_smooth) on a real MI355X against the oracle.

The powers are the oracle's, re*re + im*im of its rows in the FD dtype (oracle_power / expected of tests/test_gpu_power.py).  The
recursion s = fl(fl(a * s) + fl(b * p)) is evaluated on them by numpy
  * in the FD dtype (loop) where bits are compared: calls of one time chunk, streams cut into such calls, decay 0;
  * in np.float64 (FD float) or np.longdouble (FD double) (wide) where the bound of calls of several chunks is asserted:
    |got - s| <= 8 u M / (1 - a), u = 2^-24 or 2^-53, M the largest of the incoming state and s up to that sample, element by
    element.  A wide recursion rounds 2^-29 (2^-11 for FD double) of u per step: far below the bound's slack.
On the route that is not bit-identical (FD double with default carries) the power call's term deviation, 2.1e-11 of the largest
power, comes on top.  Every comparison first asserts that its reference is finite and that its largest value is a normal number.

Inputs are sine_sweep(n) + 0.25 noise(n), the signal of tests/test_gpu_power.py, or that signal with a 40 dB burst in its middle."""

import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import guarded as G
from oracle import oracle as O
from sdft_amd.sdft import SDFT, every_next_first, every_rows, smooth_coefficients, smooth_decay
from sdft_amd.signals import noise
from test_gpu_power import BAR, WINDOWS, exact_combo, expected, make, oracle_power, signal, to_dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECAYS = (0.0, 0.5, 0.9, 1.0 - 2.0 ** -10)
BOUND = 8.0
LONGDOUBLE_OK = np.finfo(np.longdouble).nmant >= 63


def fd_of(combo):
    return O.combo_types(combo)[1]


def wide_of(fd):
    return np.float64 if np.dtype(fd) == np.float32 else np.longdouble


def need_wide(combo):
    if np.dtype(fd_of(combo)) == np.float64 and not LONGDOUBLE_OK:
        pytest.skip("np.longdouble has fewer than 63 mantissa bits here: no reference wider than FD double")


def loop(p, decay, state=None):
    """(n, bins) s after every sample and the end value, in p's dtype: one rounding per product, one per sum"""
    a, b = smooth_coefficients(decay, p.dtype)
    s = np.zeros(p.shape[1], dtype=p.dtype) if state is None else np.array(state, dtype=p.dtype)
    out = np.empty_like(p)
    for t in range(p.shape[0]):
        s = a * s + b * p[t]
        out[t] = s
    assert out.dtype == p.dtype
    return out, s


def wide(p, decay, state=None):
    """(n, bins) of the exact recursion on the FD terms and the rounded coefficients, in the wide type; M, the running largest of
    the incoming state and s; and u / (1 - a)"""
    fd, w = p.dtype, wide_of(p.dtype)
    a, b = (w(v) for v in smooth_coefficients(decay, fd))
    s = np.zeros(p.shape[1], dtype=w) if state is None else np.array(state, dtype=w)
    out, big = np.empty(p.shape, dtype=w), np.empty(p.shape, dtype=w)
    m = s.copy()
    for t in range(p.shape[0]):
        s = a * s + b * p[t].astype(w)
        m = np.maximum(m, s)
        out[t], big[t] = s, m
    u = w(2.0) ** (-24 if np.dtype(fd) == np.float32 else -53)
    return out, big, u / (w(1) - a)


def sane(ref):
    """the reference is finite and its largest value is a normal number"""
    ref = np.asarray(ref)
    assert ref.size and np.isfinite(ref).all()
    assert float(ref.max()) >= float(np.finfo(np.float32 if ref.dtype == np.float32 else np.float64).tiny)


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def same_bits(got, want, what):
    got = host(got)
    sane(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    assert np.array_equal(got, want), (what, int((got != want).sum()), float(np.abs(got - want).max()))


WORST = {}


def within_bound(got, ref, big, scale, what, extra=0.0):
    """|got - ref| <= BOUND * u M / (1 - a) (+ extra), element by element; -> the largest ratio err / (u M / (1 - a))"""
    got = host(got)
    sane(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    err = np.maximum(np.abs(got.astype(ref.dtype) - ref) - extra, 0)
    unit = scale * big
    assert not err[unit == 0].any(), what                   # (nothing has come in yet: s is exactly 0)
    ratio = float(np.divide(err, unit, out=np.zeros_like(err), where=unit > 0).max())
    key = np.dtype(got.dtype).name
    if ratio > WORST.get(key, 0.0):
        WORST[key] = ratio
        print(f"largest err / (u M / (1 - a)) so far, {key}: {ratio:.3f} at {what}")
    assert ratio <= BOUND, (what, f"largest err / (u M / (1 - a)) = {ratio:.3f}; so far, per FD type: {WORST}")
    return ratio


def burst(combo, n, seed):
    """the signal with a 40 dB burst over its middle fifth"""
    td = O.combo_types(combo)[0]
    x = signal(n, td, seed)
    x[2 * n // 5:3 * n // 5] *= td(100)
    return x


@functools.lru_cache(maxsize=4)
def burst_expected(combo, window, m, n):
    x = burst(combo, n, m + 1)
    p = oracle_power(O.best(m, window, 1.0, combo), x)
    x.setflags(write=False)
    p.setflags(write=False)
    return x, p


def some_state(fd, shape, seed):
    """an incoming state: positive, of the size of the powers"""
    rng = np.random.default_rng(seed)
    return (rng.random(shape) * 50 + 0.125).astype(fd)


def bit_opts(combo):
    """options that put the type pair on a route where sdft_sdft_n is bit-identical to the reference"""
    return {} if exact_combo(combo) else {"carry": 1}


# ---------------------------------------------------------------------------------------------
# 1. one chunk: the sequential loop, bit for bit (promise 2)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("window", WINDOWS)
def test_power_smooth_one_chunk_is_the_loop_bit_for_bit(combo, window):
    fd = fd_of(combo)
    n, call = 300, 0
    for m in (1, 3, 64, 125):
        x, p = expected(combo, window, m, n)
        dx = to_dev(x)
        bands = [(0, m)] + ([(m // 3, m - m // 2)] if m > 1 else [])
        with make(m, window, combo) as plan:
            for band in bands:
                pb = np.ascontiguousarray(p[:, band[0]:band[0] + band[1]])
                for decay in DECAYS:
                    for given in (False, True):
                        s0 = some_state(fd, band[1], call) if given else None
                        want, end = loop(pb, decay, s0)
                        for every, first in [(1, 0), (7, 3), (n + 5, 0)]:
                            plan.reset()
                            call += 1
                            device = call % 2 == 1
                            state = None if s0 is None else (to_dev(s0) if (call // 2) % 2 else s0.copy())
                            got = plan.power_smooth(dx if device else x, decay, every, first, bins=band, state=state)
                            what = (combo, window, m, band, decay, given, every, first)
                            assert plan.get_option("last_kernel") == 15 and plan.get_option("last_chunks") == 1, what
                            assert got.shape == (every_rows(n, every, first), band[1]), what
                            same_bits(got, want[first::every], what)
                            if given:
                                same_bits(state, end, what + ("state",))
            # bins=None is the whole row
            plan.reset()
            same_bits(plan.power_smooth(x, 0.9, 7, 3), loop(p, 0.9)[0][3::7], (combo, window, m, "bins=None"))


# ---------------------------------------------------------------------------------------------
# 2. several chunks: the bound (promise 5), on the bit-identical routes and with FD double's default carries
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("m", [1000, 1024])
def test_power_smooth_several_chunks_within_the_bound(combo, m):
    """n = 6000: several chunks, a roll-over at 2N (at sample 2000 or 2048 and again later), a 40 dB burst"""
    need_wide(combo)
    fd = fd_of(combo)
    n = 6000
    x, p = burst_expected(combo, "hann", m, n)
    with make(m, "hann", combo, **bit_opts(combo)) as plan:
        for i, decay in enumerate(DECAYS[1:]):
            s0 = some_state(fd, m, i) if i % 2 else None
            ref, big, scale = wide(p, decay, s0)
            for every, first in [(1, 0), (7, 3), (100, 37)][i:i + 2]:
                plan.reset()
                state = None if s0 is None else (to_dev(s0) if first else s0.copy())
                got = plan.power_smooth(to_dev(x) if every > 1 else x, decay, every, first, state=state)
                what = (combo, m, decay, every, first)
                assert plan.get_option("last_kernel") == 15 and plan.get_option("last_chunks") > 1, what
                assert n > 2 * m and plan.get_option("last_chunk_len") < 2 * m          # (chunks begin on either side of a roll-over)
                within_bound(got, ref[first::every], big[first::every], scale, what)
                if s0 is not None:
                    within_bound(host(state)[None], ref[-1:], big[-1:], scale, what + ("state",))


@pytest.mark.parametrize("combo", O.COMBOS)
def test_power_smooth_forced_small_chunks_within_the_bound(combo):
    """n = 1500 at m = 64 with option "chunk" forced small: many chunks per bin, a partial band, the scan's batches of loads and
    its tail; the exact-carry routes' chunk shift when the plan is mid-stream"""
    need_wide(combo)
    fd = fd_of(combo)
    m, n, band = 64, 1500, (5, 40)
    x, p = burst_expected(combo, "blackman", m, n + 77)
    lead, x = x[:77], x[77:]                                # (77 samples first: the cursor is odd, exact carries shift their chunks)
    pb = np.ascontiguousarray(p[77:, band[0]:band[0] + band[1]])
    for chunk in (128, 40):
        with make(m, "blackman", combo, chunk=chunk, **bit_opts(combo)) as plan:
            for i, decay in enumerate(DECAYS[1:]):
                s0 = some_state(fd, band[1], 10 + i)
                ref, big, scale = wide(pb, decay, s0)
                plan.reset()
                plan.sdft(lead)
                state = s0.copy()
                every, first = [(1, 0), (3, 2), (250, 249)][i]
                got = plan.power_smooth(x, decay, every, first, bins=band, state=state)
                what = (combo, chunk, decay, every, first)
                assert plan.get_option("last_chunks") > 8, what
                within_bound(got, ref[first::every], big[first::every], scale, what)
                within_bound(state[None], ref[-1:], big[-1:], scale, what + ("state",))


@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_power_smooth_band_across_a_tile_boundary(combo):
    """the hooks library's option "interior" cuts a small plan into several tiles: a band of two bins that lies across the first
    boundary, and the full band, in a call of several chunks"""
    need_wide(combo)
    m, n = 125, 1500
    x, p = burst_expected(combo, "hann", m, n)
    with SDFT(m, "hann", 1.0, combo, hooks=True) as plan:
        assert plan.get_option("test_hooks") == 1
        for k, v in bit_opts(combo).items():
            plan.set_option(k, v)
        plan.set_option("interior", 31)
        per = plan.get_option("interior") * plan.get_option("bins_per_lane")
        assert plan.get_option("tiles") > 1 and per < m
        for band in [(per - 1, 2), (0, m)]:
            pb = np.ascontiguousarray(p[:, band[0]:band[0] + band[1]])
            ref, big, scale = wide(pb, 0.9)
            plan.reset()
            got = plan.power_smooth(to_dev(x), 0.9, 7, 3, bins=band)
            assert plan.get_option("last_chunks") > 1 and plan.get_option("last_kernel") == 15
            within_bound(got, ref[3::7], big[3::7], scale, (combo, band))
        # ... and one chunk there: the loop's bits
        plan.reset()
        band = (per - 1, 2)
        same_bits(plan.power_smooth(x[:300], 0.9, 1, 0, bins=band), loop(np.ascontiguousarray(p[:300, band[0]:band[0] + 2]), 0.9)[0], (combo, "one chunk"))


@pytest.mark.parametrize("combo", ["f32f64", "f64f64"])
def test_power_smooth_default_carries_within_the_bound_plus_the_term_deviation(combo):
    """FD double, fast carries: not the reference's powers bit for bit -- the power call's 2.1e-11 of the largest power on top"""
    need_wide(combo)
    m, n = 1000, 6000
    x, p = burst_expected(combo, "hann", m, n)
    ref, big, scale = wide(p, 0.9)
    with make(m, "hann", combo) as plan:
        got = plan.power_smooth(to_dev(x), 0.9, 7, 3)
        assert plan.get_option("last_chunks") > 1
        within_bound(got, ref[3::7], big[3::7], scale, (combo, "default carries"), extra=BAR * float(p.max()))


# ---------------------------------------------------------------------------------------------
# 3. decay 0 is the power call, bit for bit, on every route (promise 4)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
def test_power_smooth_decay_zero_is_power_bit_for_bit(combo):
    m, n, band = 1000, 6000, (1, 998)
    x = expected(combo, "hann", m, n)[0]
    for i, opts in enumerate([{}, dict(chunk=128), bit_opts(combo)]):
        with make(m, "hann", combo, **opts) as plan, make(m, "hann", combo, **opts) as twin:
            for every, first in [(1, 0), (7, 3)]:
                plan.reset(); twin.reset()
                xs = to_dev(x) if (i + every) % 2 else x
                state = some_state(fd_of(combo), band[1], i)          # (forgotten at once: a == 0)
                got = plan.power_smooth(xs, 0.0, every, first, bins=band, state=state)
                want = host(twin.power(xs, every, first, bins=band))
                assert plan.get_option("last_chunks") == twin.get_option("last_chunks") > 1
                same_bits(got, want, (combo, opts, every, first))
            # the state a decay of 0 leaves is the last sample's power
            plan.reset(); twin.reset()
            state = np.zeros(band[1], dtype=fd_of(combo))
            plan.power_smooth(x, 0.0, n, n - 1, bins=band, state=state)
            last = twin.power(x, 1, 0, bins=band)[-1]               # (the dense grid: the call that cuts time as the smoothed call does)
            assert plan.get_option("last_chunk_len") == twin.get_option("last_chunk_len")
            same_bits(state, last, (combo, opts, "state"))


# ---------------------------------------------------------------------------------------------
# 4. streaming (promise 3): one-chunk calls that pass state and first along have the loop's bits, wherever the cuts are
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
def test_power_smooth_streaming_in_one_chunk_calls_is_the_loop(combo):
    need_wide(combo)
    fd = fd_of(combo)
    m, n, band, decay = 64, 2000, (3, 50), smooth_decay(40.0)
    x, p = burst_expected(combo, "hamming", m, n)
    pb = np.ascontiguousarray(p[:, band[0]:band[0] + band[1]])
    want, end = loop(pb, decay)
    rng = np.random.default_rng(7)
    for every, first0 in [(1, 0), (7, 3), (450, 449)]:
        cuts, t = [], 0
        while t < n:
            k = min(int(rng.integers(1, 401)), n - t)
            cuts.append(k); t += k
        for device_state in (False, True):
            with make(m, "hamming", combo) as plan:
                state = to_dev(np.zeros(band[1], dtype=fd)) if device_state else np.zeros(band[1], dtype=fd)
                rows, t, first = [], 0, first0
                for i, k in enumerate(cuts):
                    xs = x[t:t + k]
                    d = plan.power_smooth(to_dev(xs) if i % 3 == 1 else xs, decay, every, first, bins=band, state=state)
                    assert plan.get_option("last_chunks") == 1
                    rows += list(host(d))
                    first = every_next_first(k, every, first)
                    t += k
                same_bits(np.array(rows, dtype=fd).reshape(-1, band[1]), want[first0::every], (combo, every, first0, device_state, len(cuts)))
                same_bits(state, end, (combo, every, first0, device_state, "state"))
    # the same signal as one long call of several chunks is within the bound of the loop's exact value
    ref, big, scale = wide(pb, decay)
    with make(m, "hamming", combo, **bit_opts(combo)) as plan:
        state = np.zeros(band[1], dtype=fd)
        got = plan.power_smooth(x, decay, 7, 3, bins=band, state=state)
        assert plan.get_option("last_chunks") > 1
        within_bound(got, ref[3::7], big[3::7], scale, (combo, "one long call"))
        within_bound(state[None], ref[-1:], big[-1:], scale, (combo, "one long call", "state"))


# ---------------------------------------------------------------------------------------------
# 5. the stream state (promise 6), batched plans, where state lives
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
def test_power_smooth_leaves_the_state_of_sdft(combo):
    """after the call the plan's state is a twin's after sdft_sdft_n of the same samples (which cuts time alike only by chance:
    one chunk here, where both are the reference's bits), and sdft_sdft_n goes on bit for bit; for a long call, power()'s twin"""
    td = O.combo_types(combo)[0]
    m = 125
    x = signal(6000, td, 9)
    hop = noise(100, seed=12, dtype=td)
    for n, device in ((300, False), (300, True), (6000, True)):
        with make(m, "hann", combo) as plan, make(m, "hann", combo) as twin:
            xs = to_dev(x[:n]) if device else x[:n]
            plan.power_smooth(xs, 0.9, 7, 3, bins=(60, 5))               # (bins outside the band step too)
            if n == 300:
                twin.sdft(xs)
            else:
                twin.power(xs, 1, 0, bins=(60, 5))                      # the twin that cuts time alike
                assert plan.get_option("last_chunks") == twin.get_option("last_chunks") > 1
            for a, b in zip(plan.state()[:3], twin.state()[:3]):
                assert np.array_equal(a, b), (combo, n, device)
            assert plan.state()[3] == twin.state()[3]
            dp, dq = plan.sdft(hop), twin.sdft(hop)
            assert np.array_equal(dp, dq)
            assert np.array_equal(plan.isdft(dp), twin.isdft(dq))


@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_power_smooth_batched_channels_keep_their_own_state(combo):
    need_wide(combo)
    td, fd = O.combo_types(combo)[:2]
    ch, m, band = 3, 64, (17, 30)
    for n, opts in ((300, {}), (3000, bit_opts(combo))):
        x = np.stack([signal(n, td, 100 + c) * td(1 + 3 * c) for c in range(ch)])
        terms = [np.ascontiguousarray(oracle_power(O.best(m, "blackman", 1.0, combo), x[c])[:, band[0]:band[0] + band[1]]) for c in range(ch)]
        s0 = some_state(fd, (ch, band[1]), 5)
        for device in (False, True):
            with make(m, "blackman", combo, channels=ch, **opts) as plan:
                state = to_dev(s0) if device else s0.copy()
                got = host(plan.power_smooth(to_dev(x) if device else x, 0.9, 7, 3, bins=band, state=state))
                assert got.shape == (ch, every_rows(n, 7, 3), band[1]) and plan.get_option("last_kernel") == 15
                assert (plan.get_option("last_chunks") > 1) == (n > 512)
                for c in range(ch):
                    if n == 300:
                        want, end = loop(terms[c], 0.9, s0[c])
                        same_bits(got[c], want[3::7], (combo, device, c))
                        same_bits(host(state)[c], end, (combo, device, c, "state"))
                    else:
                        ref, big, scale = wide(terms[c], 0.9, s0[c])
                        within_bound(got[c], ref[3::7], big[3::7], scale, (combo, device, c))
                        within_bound(host(state)[c][None], ref[-1:], big[-1:], scale, (combo, device, c, "state"))


def test_power_smooth_state_on_host_or_device_whatever_the_other_pointers_are():
    import torch
    combo, m, band, decay = "f32f32", 64, (3, 50), 0.9
    fd = fd_of(combo)
    for n in (300, 1500):
        x, p = expected(combo, "hann", m, n)
        pb = np.ascontiguousarray(p[:, band[0]:band[0] + band[1]])
        s0 = some_state(fd, band[1], 3)
        rows = every_rows(n, 7, 3)
        seen = []
        with make(m, "hann", combo) as plan:
            for xd in (False, True):
                for od in (False, True):
                    for sd in (False, True):
                        plan.reset()
                        xs = to_dev(x) if xd else x
                        out = torch.zeros((rows, band[1]), dtype=torch.float32, device="cuda") if od else np.zeros((rows, band[1]), dtype=fd)
                        state = to_dev(s0) if sd else s0.copy()
                        ptr = lambda a: C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)
                        got = plan.api.sdft_power_smooth_n(plan._p, n, ptr(xs), 7, 3, band[0], band[1], decay, ptr(state), ptr(out))
                        plan.synchronize()
                        assert got == rows, plan.api.last_error()
                        seen.append((host(out).copy(), host(state).copy()))
            if n == 300:
                want, end = loop(pb, decay, s0)
                same_bits(seen[0][0], want[3::7], "one chunk"); same_bits(seen[0][1], end, "one chunk, state")
            else:
                # (host samples go in segments: the bits may differ between placements, each is within the bound)
                ref, big, scale = wide(pb, decay, s0)
                for o, s in seen:
                    within_bound(o, ref[3::7], big[3::7], scale, "placements"); within_bound(s[None], ref[-1:], big[-1:], scale, "placements, state")
            if n == 300:
                assert all(np.array_equal(seen[0][0], o) and np.array_equal(seen[0][1], s) for o, s in seen[1:])


# ---------------------------------------------------------------------------------------------
# 6. host memory in segments
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_power_smooth_host_staging_in_segments(combo):
    """a small stage_bytes on host pointers: segments of one chunk each have the loop's bits (state travels between them on the
    device); longer segments are within the bound"""
    need_wide(combo)
    import torch
    fd = fd_of(combo)
    m, n, band, decay = 64, 2000, (3, 50), 0.9
    x, p = burst_expected(combo, "hann", m, n)
    pb = np.ascontiguousarray(p[:, band[0]:band[0] + band[1]])
    s0 = some_state(fd, band[1], 8)
    want, end = loop(pb, decay, s0)
    ref, big, scale = wide(pb, decay, s0)
    row = band[1] * np.dtype(fd).itemsize
    for every, first, stage, one_chunk in [(1, 0, 300 * row, True), (7, 3, 40 * row, True), (1, 0, 900 * row, False)]:
        with make(m, "hann", combo, stage_bytes=stage, **bit_opts(combo)) as plan:
            rows = every_rows(n, every, first)
            plan.reset()
            state = s0.copy()
            got = plan.power_smooth(x, decay, every, first, bins=band, state=state)
            what = (combo, stage, every, first)
            assert plan.get_option("last_segments") > 1, what
            if one_chunk:
                assert plan.get_option("last_chunks") == 1 and plan.get_option("last_chunk_len") < 512
                same_bits(got, want[first::every], what); same_bits(state, end, what + ("state",))
            within_bound(got, ref[first::every], big[first::every], scale, what)
            within_bound(state[None], ref[-1:], big[-1:], scale, what + ("state",))
            # host samples, device rows and state
            plan.reset()
            out = torch.zeros((rows, band[1]), dtype=getattr(torch, np.dtype(fd).name), device="cuda")
            dstate = to_dev(s0)
            r = plan.api.sdft_power_smooth_n(plan._p, n, C.c_void_p(x.ctypes.data), every, first, band[0], band[1], decay, C.c_void_p(dstate.data_ptr()),
                                             C.c_void_p(out.data_ptr()))
            plan.synchronize()
            assert r == rows, plan.api.last_error()
            within_bound(out, ref[first::every], big[first::every], scale, what + ("device rows",))
            within_bound(host(dstate)[None], ref[-1:], big[-1:], scale, what + ("device state",))


# ---------------------------------------------------------------------------------------------
# 7. no overrun, no hole, at every alignment an element size allows: smooth and state
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host_side", [False, True])
@pytest.mark.parametrize("combo", ["f32f32", "f32f64"])
def test_power_smooth_guarded_misaligned_buffers(combo, host_side):
    """smooth and state carved from a guarded arena at every residue modulo 16 their element size allows, and at 16 mod 128; a band
    of 999 bins (an odd row length: consecutive rows change alignment) in a call of several chunks, whose fix-up rewrites rows"""
    need_wide(combo)
    td, fd, _ = O.combo_types(combo)
    m, n, every, first, band = 1000, 2000, 7, 3, (1, 999)
    x, p = expected(combo, "hann", m, n)
    pb = np.ascontiguousarray(p[:, band[0]:band[0] + band[1]])
    s0 = some_state(fd, band[1], 4)
    ref, big, scale = wide(pb, 0.9, s0)
    rows = every_rows(n, every, first)
    size = np.dtype(fd).itemsize
    places = [(r, 16) for r in range(size, 16, size)] + [(16, 128)]
    with make(m, "hann", combo, **bit_opts(combo)) as plan:
        for r, mod in places:
            arena = (G.HostArena if host_side else G.DeviceArena)(G.room(((n,), td), ((rows, band[1]), fd), ((band[1],), fd)))
            xv = G.put(arena.carve((n,), td, np.dtype(td).itemsize, 16, name="x"), x)
            out = arena.carve((rows, band[1]), fd, r, mod, name="smooth")
            sv = G.put(arena.carve((band[1],), fd, r, mod, name="state"), s0)
            assert G.ptr_of(out) % mod == r and G.ptr_of(sv) % mod == r
            plan.reset()
            plan.api.clear()
            got = plan.api.sdft_power_smooth_n(plan._p, n, C.c_void_p(G.ptr_of(xv)), every, first, band[0], band[1], 0.9, C.c_void_p(G.ptr_of(sv)),
                                               C.c_void_p(G.ptr_of(out)))
            plan.synchronize()
            assert got == rows, plan.api.last_error()
            assert plan.get_option("last_kernel") == 15
            arena.check()
            assert G.view_unwritten(out) == 0
            assert np.array_equal(G.to_numpy(xv), x)
            within_bound(G.to_numpy(out), ref[first::every], big[first::every], scale, (combo, host_side, r, mod))
            within_bound(G.to_numpy(sv)[None], ref[-1:], big[-1:], scale, (combo, host_side, r, mod, "state"))


# ---------------------------------------------------------------------------------------------
# 8. errors leave the stream state and the caller's state alone
# ---------------------------------------------------------------------------------------------
def test_power_smooth_errors():
    combo, m = "f32f32", 64
    x = signal(3000, np.float32, 5)
    top = C.c_size_t(-1).value
    with make(m, "hann", combo) as plan:
        api = plan.api
        plan.power_smooth(x[:300], 0.5, 7, 3)                        # (errors against a plan that is mid-stream)
        out = np.zeros((12, m), dtype=np.float32)
        state = some_state(np.float32, m, 1)
        kept = state.copy()
        before = plan.state()
        o, s = out.ctypes.data, state.ctypes.data
        refused = [(100, 0, 0, 0, m, 0.5, s, o, "every"),                 # every == 0
                   (100, 10, 0, 0, 0, 0.5, s, o, "nbins"),                # nbins == 0
                   (100, 10, 0, 1, m, 0.5, s, o, "band"),                 # bin0 + nbins > dftsize
                   (100, 10, 0, m, 1, 0.5, s, o, "band"),
                   (100, 10, 0, 2, top, 0.5, s, o, "band"),               # bin0 + nbins overflows to 1
                   (100, 10, 0, 0, m, float("nan"), s, o, "decay"),
                   (100, 10, 0, 0, m, -0.25, s, o, "decay"),
                   (100, 10, 0, 0, m, 1.0, s, o, "decay"),
                   (100, 10, 0, 0, m, 1.0 - 2.0 ** -26, s, o, "decay"),   # rounds to 1 in FD float
                   (100, 10, 0, 0, m, float("inf"), s, o, "decay"),
                   (0, 10, 0, 0, m, 2.0, s, None, "decay"),               # ... even for a call without samples
                   (100, 10, 0, 0, m, 0.5, s, None, "NULL")]              # rows > 0, smooth NULL
        for n, every, first, bin0, nb, decay, sp, op, word in refused:
            api.clear()
            assert api.sdft_power_smooth_n(plan._p, n, x.ctypes.data, every, first, bin0, nb, decay, sp, op) == -1, (every, bin0, nb, decay)
            err = api.last_error()
            assert err and "sdft_hip_sdft_power_smooth_n" in err and word in err, err
            api.clear()
            after = plan.state()
            assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3], (every, bin0, nb, decay)
            assert np.array_equal(state, kept), (every, bin0, nb, decay)
        assert np.count_nonzero(out) == 0
        # n == 0: no rows, nothing moves, smooth may be NULL, state stays
        assert api.sdft_power_smooth_n(plan._p, 0, x.ctypes.data, 10, 3, 0, m, 0.5, s, None) == 0 and api.last_error() is None
        assert plan.state()[3] == before[3] and np.array_equal(state, kept)
        # no row kept: smooth may be NULL, the state advances all the same
        assert api.sdft_power_smooth_n(plan._p, 100, x.ctypes.data, 10, 500, 0, m, 0.5, s, None) == 0 and api.last_error() is None
        assert not np.array_equal(state, kept) and plan.state()[3] != before[3]
        with make(m, "hann", combo) as twin:
            twin.power_smooth(x[:300], 0.5, 7, 3)
            want = kept.copy()
            twin.power_smooth(x[:100], 0.5, 1, 0, state=want)
            assert np.array_equal(state, want)
        # the Python call refuses the same before it touches the plan
        for bad in (float("nan"), -0.25, 1.0):
            with pytest.raises(ValueError):
                plan.power_smooth(x[:10], bad)
        with pytest.raises(ValueError):
            plan.power_smooth(x[:10], 0.5, state=np.zeros(m - 1, dtype=np.float32))


# ---------------------------------------------------------------------------------------------
# 9. the same bits on every run (promise 1)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", ["f32f64", "f64f32"])
def test_power_smooth_same_bits_on_every_run(combo):
    m, n = 1000, 6000
    x = expected(combo, "hann", m, n)[0]
    s0 = some_state(fd_of(combo), m, 2)
    for device in (False, True):
        xs = to_dev(x) if device else x
        with make(m, "hann", combo) as plan:
            for every, first in [(1, 0), (100, 37)]:
                runs = []
                for _ in range(3):
                    plan.reset()
                    state = to_dev(s0) if device else s0.copy()
                    d = plan.power_smooth(xs, 0.9, every, first, state=state)
                    assert plan.get_option("last_chunks") > 1
                    runs.append((host(d), host(state)))
                assert all(np.array_equal(runs[0][0], r[0]) and np.array_equal(runs[0][1], r[1]) for r in runs[1:]), (combo, device, every, first)


def test_power_smooth_async_device_pointers():
    need_wide("f32f64")
    m, n = 1000, 6000
    x, p = burst_expected("f32f64", "hann", m, n)
    ref, big, scale = wide(p[:, :256], 0.9)
    with make(m, "hann", "f32f64", **{"async": 1}) as plan:
        state = to_dev(np.zeros(256))
        a = plan.power_smooth(to_dev(x), 0.9, 100, 37, bins=(0, 256), state=state)
        plan.synchronize()
        extra = BAR * float(p.max())
        within_bound(a, ref[37::100], big[37::100], scale, "async", extra=extra)
        within_bound(host(state)[None], ref[-1:], big[-1:], scale, "async, state", extra=extra)


# ---------------------------------------------------------------------------------------------
# 10. a plain C host and a C++ host: a stream in blocks, state passed from call to call
# ---------------------------------------------------------------------------------------------
def python_in_blocks(combo, m, x, every, block, band, decay):
    with make(m, "hann", combo) as plan:
        state = np.zeros(band[1], dtype=fd_of(combo))
        rows, first = [], 0
        for t in range(0, x.size, block):
            k = min(block, x.size - t)
            rows += list(plan.power_smooth(x[t:t + k], decay, every, first, bins=band, state=state))
            first = every_next_first(k, every, first)
        return np.array(rows), state


@pytest.mark.parametrize("flags,combo", [([], "f32f64"), (["-DSDFT_FD_FLOAT"], "f32f32")])
def test_c_host_power_smooth(tmp_path, hip_library, flags, combo):
    fd = fd_of(combo)
    libdir = os.path.dirname(hip_library)
    rt = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    exe = tmp_path / "host_power_smooth"
    cmd = ["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), *flags,
           os.path.join(ROOT, "tests", "c", "host_power_smooth.c"), "-o", str(exe),
           "-L", libdir, "-lsdft_hip", "-L", rt, "-lamdhip64", "-lm", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{rt}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m, n, every, block, band, decay = 64, 2000, 7, 330, (3, 50), 0.96875
    x, p = expected(combo, "hann", m, n)
    x.tofile(tmp_path / "x.raw")
    r = subprocess.run([str(exe), str(m), str(every), str(block), str(band[0]), str(band[1]), repr(decay), str(tmp_path / "x.raw"),
                        str(tmp_path / "s.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "C-HOST-POWER-SMOOTH ok" in r.stdout
    got = np.fromfile(tmp_path / "s.raw", dtype=fd).reshape(-1, band[1])
    # blocks of 330 samples are one chunk each: the loop's bits over the whole signal, and the state's behind the last row
    want, end = loop(np.ascontiguousarray(p[:, band[0]:band[0] + band[1]]), decay)
    same_bits(got[:-1], want[::every], ("C host", combo))
    same_bits(got[-1], end, ("C host", combo, "state"))
    rows, state = python_in_blocks(combo, m, x, every, block, band, decay)
    assert np.array_equal(got[:-1], rows) and np.array_equal(got[-1], state)


@pytest.mark.parametrize("t,f,combo", [("float", "double", "f32f64"), ("float", "float", "f32f32")])
def test_cpp_host_power_smooth(tmp_path, hip_library, t, f, combo):
    fd = fd_of(combo)
    libdir = os.path.dirname(hip_library)
    rt = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    exe = tmp_path / "host_power_smooth_cpp"
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", f"-DHOST_T={t}", f"-DHOST_F={f}", "-I", os.path.join(ROOT, "include", "cpp"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "host_power_smooth.cpp"), "-o", str(exe),
           "-L", libdir, "-lsdft_hip", "-L", rt, "-lamdhip64", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{rt}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m, n, every, block, band, decay = 64, 2000, 7, 330, (3, 50), 0.96875
    x, p = expected(combo, "hann", m, n)
    x.tofile(tmp_path / "x.raw")
    r = subprocess.run([str(exe), str(m), str(every), str(block), str(band[0]), str(band[1]), repr(decay), str(tmp_path / "x.raw"),
                        str(tmp_path / "s.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "CPP-POWER-SMOOTH ok" in r.stdout
    got = np.fromfile(tmp_path / "s.raw", dtype=fd).reshape(-1, band[1])
    want, end = loop(np.ascontiguousarray(p[:, band[0]:band[0] + band[1]]), decay)
    same_bits(got[:-1], want[::every], ("C++ host", combo))
    same_bits(got[-1], end, ("C++ host", combo, "state"))
