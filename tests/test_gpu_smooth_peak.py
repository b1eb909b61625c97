"""Smoothed peak-hold analysis (sdft_hip_sdft_smooth_peak_n, SDFT.smooth_peak) on a real MI355X against the oracle.

The powers are the oracle's (expected / oracle_power of tests/test_gpu_power.py); the recursion s = fl(fl(a * s) + fl(b * p)) on
them is loop() of tests/test_gpu_power_smooth.py (the FD dtype: where bits are compared) or wide() (np.float64 for FD float,
np.longdouble for FD double: where the bound is asserted); the rows are np.maximum.reduce / np.minimum.reduce of that sequence
over the windows of tests/test_gpu_power_sum.py (held_rows of tests/test_gpu_power_peak.py).

  * one chunk, and a stream cut into one-chunk calls: the loop's extremes bit for bit, and the loop's end value in state;
  * every = 1 on one chunk: sdft_hip_sdft_power_smooth_n's rows; decay 0: sdft_hip_sdft_power_peak_n's rows, on any route;
  * several chunks: the rows at (every, first) are bit for bit the window-wise extremes of the same call's rows at (1, 0), and
    state is the last of those -- no tolerance: the flush rule, the cut-window slots and the chunk starts are pinned;
  * several chunks against the exact recursion: |got - peak| <= 8 u M / (1 - a), M the running largest of the incoming state and
    s up to the window's last sample (|ext(x') - ext(x)| <= max |x' - x|, and M does not decrease), with the power call's term
    deviation, 2.1e-11 of the largest power, on top on the route that is not bit-identical."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import guarded as G
from oracle import oracle as O
from sdft_amd.sdft import SDFT, every_next_first, power_sum_rows, smooth_decay
from sdft_amd.signals import noise
from test_gpu_power import BAR, WINDOWS, expected, make, oracle_power, signal, to_dev
from test_gpu_power_peak import HOLDS, held_rows
from test_gpu_power_smooth import (BOUND, bit_opts, burst_expected, fd_of, host, loop, need_wide, same_bits, sane, some_state, wide,
                                   within_bound)
from test_gpu_power_sum import windows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = 17


def at_ends(big, n, every, first):
    """(rows, bins) of the (n, bins) running largest at each window's last sample"""
    return np.array([big[e - 1] for _, e in windows(n, every, first)], dtype=big.dtype).reshape(-1, big.shape[1])


def held_within_bound(got, ref, big, scale, n, every, first, hold, what, extra=0.0):
    return within_bound(got, held_rows(ref, n, every, first, hold), at_ends(big, n, every, first), scale, what, extra=extra)


def stream_join(pieces, firsts, hold, fd, nb):
    """the rows of a stream from its calls' rows: a call with first > 0 completes the last row begun by np.fmax / np.fmin"""
    join = np.fmax if hold == "max" else np.fmin
    rows = []
    for d, first in zip(pieces, firsts):
        d = list(host(d))
        if first > 0:
            rows[-1] = join(rows[-1], d.pop(0))
        rows += d
    return np.array(rows, dtype=fd).reshape(-1, nb)


# ---------------------------------------------------------------------------------------------
# 1. one chunk: the extremes of the sequential loop, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("window", WINDOWS)
def test_smooth_peak_one_chunk_is_the_loop_bit_for_bit(combo, window):
    fd = fd_of(combo)
    n, call = 300, 0
    for m in (1, 3, 64, 125):
        x, p = expected(combo, window, m, n)
        dx = to_dev(x)
        bands = [(0, m)] + ([(m // 3, m - m // 2)] if m > 1 else [])
        with make(m, window, combo) as plan:
            for band in bands:
                pb = np.ascontiguousarray(p[:, band[0]:band[0] + band[1]])
                for decay in (0.5, 1.0 - 2.0 ** -10):
                    for given in (False, True):
                        s0 = some_state(fd, band[1], call) if given else None
                        seq, end = loop(pb, decay, s0)
                        for every, first in [(1, 0), (7, 3), (n + 5, 0), (50, 60)]:
                            for hold in HOLDS:
                                plan.reset()
                                call += 1
                                device = call % 2 == 1
                                state = None if s0 is None else (to_dev(s0) if (call // 2) % 2 else s0.copy())
                                got = plan.smooth_peak(dx if device else x, decay, every, first, bins=band, hold=hold, state=state)
                                what = (combo, window, m, band, decay, given, every, first, hold)
                                assert plan.get_option("last_kernel") == KERNEL and plan.get_option("last_chunks") == 1, what
                                assert got.shape == (power_sum_rows(n, every, first), band[1]), what
                                same_bits(got, held_rows(seq, n, every, first, hold), what)
                                if given:
                                    same_bits(state, end, what + ("state",))
            # bins=None is the whole row
            plan.reset()
            same_bits(plan.smooth_peak(x, 0.9, 7, 3, hold="min"), held_rows(loop(p, 0.9)[0], n, 7, 3, "min"), (combo, window, m, "bins=None"))


# ---------------------------------------------------------------------------------------------
# 2. every = 1 on one chunk: the smoothed power call's rows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
def test_smooth_peak_of_one_sample_windows_is_power_smooth_bit_for_bit(combo):
    fd = fd_of(combo)
    m, n, band = 125, 400, (7, 100)
    x = expected(combo, "blackman", m, n)[0]
    s0 = some_state(fd, band[1], 3)
    with make(m, "blackman", combo) as plan, make(m, "blackman", combo) as twin:
        for hold in HOLDS:
            plan.reset(); twin.reset()
            sa, sb = s0.copy(), s0.copy()
            got = plan.smooth_peak(x, 0.9, 1, 0, bins=band, hold=hold, state=sa)
            want = twin.power_smooth(x, 0.9, 1, 0, bins=band, state=sb)
            assert plan.get_option("last_chunks") == twin.get_option("last_chunks") == 1
            same_bits(got, want, (combo, hold))
            same_bits(sa, sb, (combo, hold, "state"))


# ---------------------------------------------------------------------------------------------
# 3. decay 0 is the peak-hold call, bit for bit, on every route and any chunking
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
def test_smooth_peak_decay_zero_is_power_peak_bit_for_bit(combo):
    fd = fd_of(combo)
    cases = [(1000, 6000, (1, 998), {}), (1000, 6000, (1, 998), bit_opts(combo)), (64, 1500, (5, 40), dict(chunk=40)), (64, 300, (0, 64), {})]
    for i, (m, n, band, opts) in enumerate(cases):
        x = expected(combo, "hann", m, n)[0]
        with make(m, "hann", combo, **opts) as plan, make(m, "hann", combo, **opts) as twin:
            for every, first in [(1, 0), (7, 3), (250, 249)]:
                for hold in HOLDS:
                    plan.reset(); twin.reset()
                    xs = to_dev(x) if (i + every) % 2 else x
                    state = some_state(fd, band[1], i)                # (forgotten at once: a == 0)
                    got = plan.smooth_peak(xs, 0.0, every, first, bins=band, hold=hold, state=state)
                    want = host(twin.power_peak(xs, every, first, bins=band, hold=hold))
                    what = (combo, m, n, opts, every, first, hold)
                    assert plan.get_option("last_chunks") == twin.get_option("last_chunks") and (plan.get_option("last_chunks") > 1) == (n > 512), what
                    assert plan.get_option("last_chunk_len") == twin.get_option("last_chunk_len"), what
                    same_bits(got, want, what)
            # the state a decay of 0 leaves is the last sample's power
            plan.reset(); twin.reset()
            state = np.zeros(band[1], dtype=fd)
            plan.smooth_peak(x, 0.0, n, n - 1, bins=band, state=state)
            last = twin.power_peak(x, 1, 0, bins=band)[-1]
            assert plan.get_option("last_chunk_len") == twin.get_option("last_chunk_len")
            same_bits(state, last, (combo, m, opts, "state"))


# ---------------------------------------------------------------------------------------------
# 4. several chunks: the hold is exact on the call's own s
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True], ids=["default-carries", "exact-carries"])
@pytest.mark.parametrize("combo", O.COMBOS)
def test_smooth_peak_several_chunks_hold_their_own_sequence_exactly(combo, exact):
    """m = 64, n = 1500, option "chunk" forced: many chunks, windows inside a chunk, across one boundary and across all of them; 77
    samples first, so that the cursor is odd and the exact carries shift their chunks"""
    fd = fd_of(combo)
    m, n, band = 64, 1500, (5, 40)
    x = expected(combo, "blackman", m, n + 77)[0]
    lead, x = x[:77], x[77:]
    opts = bit_opts(combo) if exact else {}
    for chunk in (128, 40):
        with make(m, "blackman", combo, chunk=chunk, **opts) as plan:
            for i, decay in enumerate((0.5, 0.9, 1.0 - 2.0 ** -10)):
                s0 = some_state(fd, band[1], 10 + i)
                for hold in HOLDS:
                    plan.reset()
                    plan.sdft(lead)
                    dense_state = s0.copy()
                    dense = host(plan.smooth_peak(to_dev(x), decay, 1, 0, bins=band, hold=hold, state=dense_state))
                    cut = (plan.get_option("last_chunks"), plan.get_option("last_chunk_len"))
                    assert cut[0] > 8 and plan.get_option("last_kernel") == KERNEL
                    sane(dense)
                    same_bits(dense_state, dense[-1], (combo, chunk, decay, hold, "state of the dense call"))
                    for every, first in [(3, 2), (250, 249), (n + 1, 0)]:
                        plan.reset()
                        plan.sdft(lead)
                        state = to_dev(s0) if every == 3 else s0.copy()
                        got = plan.smooth_peak(x if every == 3 else to_dev(x), decay, every, first, bins=band, hold=hold, state=state)
                        what = (combo, exact, chunk, decay, hold, every, first)
                        assert (plan.get_option("last_chunks"), plan.get_option("last_chunk_len")) == cut, what
                        same_bits(got, held_rows(dense, n, every, first, hold), what)
                        same_bits(state, dense[-1], what + ("state",))


# ---------------------------------------------------------------------------------------------
# 5. several chunks against the exact recursion: the bound
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("m", [1000, 1024])
def test_smooth_peak_several_chunks_within_the_bound(combo, m):
    """n = 6000: several chunks, a roll-over at 2N, a 40 dB burst"""
    need_wide(combo)
    fd = fd_of(combo)
    n = 6000
    x, p = burst_expected(combo, "hann", m, n)
    with make(m, "hann", combo, **bit_opts(combo)) as plan:
        for i, decay in enumerate((0.5, 0.9, 1.0 - 2.0 ** -10)):
            s0 = some_state(fd, m, i) if i % 2 else None
            ref, big, scale = wide(p, decay, s0)
            for j, (every, first) in enumerate([(1, 0), (7, 3), (100, 37)][i:i + 2]):
                hold = HOLDS[(i + j) % 2]
                plan.reset()
                state = None if s0 is None else (to_dev(s0) if first else s0.copy())
                got = plan.smooth_peak(to_dev(x) if every > 1 else x, decay, every, first, hold=hold, state=state)
                what = (combo, m, decay, every, first, hold)
                assert plan.get_option("last_kernel") == KERNEL and plan.get_option("last_chunks") > 1, what
                assert n > 2 * m and plan.get_option("last_chunk_len") < 2 * m          # (chunks begin on either side of a roll-over)
                held_within_bound(got, ref, big, scale, n, every, first, hold, what)
                if s0 is not None:
                    within_bound(host(state)[None], ref[-1:], big[-1:], scale, what + ("state",))


@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_smooth_peak_band_across_a_tile_boundary(combo):
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
            for hold in HOLDS:
                plan.reset()
                got = plan.smooth_peak(to_dev(x), 0.9, 7, 3, bins=band, hold=hold)
                assert plan.get_option("last_chunks") > 1 and plan.get_option("last_kernel") == KERNEL
                held_within_bound(got, ref, big, scale, n, 7, 3, hold, (combo, band, hold))
        # ... and one chunk there: the loop's bits
        plan.reset()
        band = (per - 1, 2)
        seq = loop(np.ascontiguousarray(p[:300, band[0]:band[0] + 2]), 0.9)[0]
        same_bits(plan.smooth_peak(x[:300], 0.9, 7, 3, bins=band, hold="min"), held_rows(seq, 300, 7, 3, "min"), (combo, "one chunk"))


@pytest.mark.parametrize("combo", ["f32f64", "f64f64"])
def test_smooth_peak_default_carries_within_the_bound_plus_the_term_deviation(combo):
    """FD double, fast carries: not the reference's powers bit for bit -- the power call's 2.1e-11 of the largest power on top"""
    need_wide(combo)
    m, n = 1000, 6000
    x, p = burst_expected(combo, "hann", m, n)
    ref, big, scale = wide(p, 0.9)
    with make(m, "hann", combo) as plan:
        for hold in HOLDS:
            plan.reset()
            state = np.zeros(m, dtype=fd_of(combo))
            got = plan.smooth_peak(to_dev(x), 0.9, 7, 3, hold=hold, state=state)
            assert plan.get_option("last_chunks") > 1
            extra = BAR * float(p.max())
            held_within_bound(got, ref, big, scale, n, 7, 3, hold, (combo, "default carries", hold), extra=extra)
            within_bound(state[None], ref[-1:], big[-1:], scale, (combo, "default carries", "state"), extra=extra)


# ---------------------------------------------------------------------------------------------
# 6. streaming: one-chunk calls that pass state and first along and join head rows have the loop's bits, wherever the cuts are
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("combo", O.COMBOS)
def test_smooth_peak_streaming_in_one_chunk_calls_is_the_loop(combo, hold):
    fd = fd_of(combo)
    m, n, band, decay = 64, 2000, (3, 50), smooth_decay(40.0)
    x, p = burst_expected(combo, "hamming", m, n)
    pb = np.ascontiguousarray(p[:, band[0]:band[0] + band[1]])
    seq, end = loop(pb, decay)
    rng = np.random.default_rng(7)
    for every, first0 in [(1, 0), (7, 3), (450, 449)]:
        # cuts before a window's first sample, in a window's middle and on a grid point, then wherever
        must = {first0 + every, first0 + every + every // 2 + 1, first0 + 2 * every + 1}
        edges, t = set(must) | {n}, 0
        while t < n:
            t += int(rng.integers(1, 401))
            edges.add(min(t, n))
        edges = sorted(edges)
        cuts = [int(k) for k in np.diff([0] + edges)]
        assert sum(cuts) == n and 0 < min(cuts) and max(cuts) < 512 and must <= set(edges)
        for device_state in (False, True):
            with make(m, "hamming", combo) as plan:
                state = to_dev(np.zeros(band[1], dtype=fd)) if device_state else np.zeros(band[1], dtype=fd)
                pieces, firsts, t, first = [], [], 0, first0
                for i, k in enumerate(cuts):
                    xs = x[t:t + k]
                    pieces.append(plan.smooth_peak(to_dev(xs) if i % 3 == 1 else xs, decay, every, first, bins=band, hold=hold, state=state))
                    assert plan.get_option("last_chunks") == 1
                    firsts.append(first if t else 0)             # (the stream's own head window is a row of its own)
                    first = every_next_first(k, every, first)
                    t += k
                what = (combo, hold, every, first0, device_state, len(cuts))
                same_bits(stream_join(pieces, firsts, hold, fd, band[1]), held_rows(seq, n, every, first0, hold), what)
                same_bits(state, end, what + ("state",))


# ---------------------------------------------------------------------------------------------
# 7. the stream state
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
def test_smooth_peak_leaves_the_state_of_sdft(combo):
    """after the call the plan's state is a twin's after sdft_sdft_n of the same samples (one chunk: both are the reference's
    bits) or after the peak-hold call, which cuts time alike (several chunks); sdft_sdft_n goes on bit for bit"""
    td = O.combo_types(combo)[0]
    m = 125
    x = signal(6000, td, 9)
    hop = noise(100, seed=12, dtype=td)
    for n, device in ((300, False), (300, True), (6000, True)):
        with make(m, "hann", combo) as plan, make(m, "hann", combo) as twin:
            xs = to_dev(x[:n]) if device else x[:n]
            plan.smooth_peak(xs, 0.9, 7, 3, bins=(60, 5), hold="min")        # (bins outside the band step too)
            if n == 300:
                twin.sdft(xs)
            else:
                twin.power_peak(xs, 7, 3, bins=(60, 5))
                assert plan.get_option("last_chunks") == twin.get_option("last_chunks") > 1
            for a, b in zip(plan.state()[:3], twin.state()[:3]):
                assert np.array_equal(a, b), (combo, n, device)
            assert plan.state()[3] == twin.state()[3]
            dp, dq = plan.sdft(hop), twin.sdft(hop)
            assert np.array_equal(dp, dq)
            assert np.array_equal(plan.isdft(dp), twin.isdft(dq))


# ---------------------------------------------------------------------------------------------
# 8. pointer placement, staging, guarded buffers, async, repeatability, NaN, refusals, the C and C++ hosts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_smooth_peak_batched_channels_keep_their_own_state(combo):
    need_wide(combo)
    td, fd = O.combo_types(combo)[:2]
    ch, m, band = 3, 64, (17, 30)
    for n, opts in ((300, {}), (3000, bit_opts(combo))):
        x = np.stack([signal(n, td, 100 + c) * td(1 + 3 * c) for c in range(ch)])
        terms = [np.ascontiguousarray(oracle_power(O.best(m, "blackman", 1.0, combo), x[c])[:, band[0]:band[0] + band[1]]) for c in range(ch)]
        s0 = some_state(fd, (ch, band[1]), 5)
        for device in (False, True):
            hold = HOLDS[device]
            with make(m, "blackman", combo, channels=ch, **opts) as plan:
                state = to_dev(s0) if device else s0.copy()
                got = host(plan.smooth_peak(to_dev(x) if device else x, 0.9, 7, 3, bins=band, hold=hold, state=state))
                assert got.shape == (ch, power_sum_rows(n, 7, 3), band[1]) and plan.get_option("last_kernel") == KERNEL
                assert (plan.get_option("last_chunks") > 1) == (n > 512)
                for c in range(ch):
                    if n == 300:
                        seq, end = loop(terms[c], 0.9, s0[c])
                        same_bits(got[c], held_rows(seq, n, 7, 3, hold), (combo, device, c))
                        same_bits(host(state)[c], end, (combo, device, c, "state"))
                    else:
                        ref, big, scale = wide(terms[c], 0.9, s0[c])
                        held_within_bound(got[c], ref, big, scale, n, 7, 3, hold, (combo, device, c))
                        within_bound(host(state)[c][None], ref[-1:], big[-1:], scale, (combo, device, c, "state"))


def test_smooth_peak_state_on_host_or_device_whatever_the_other_pointers_are():
    import torch
    combo, m, band, decay = "f32f32", 64, (3, 50), 0.9
    fd = fd_of(combo)
    for n in (300, 1500):
        x, p = expected(combo, "hann", m, n)
        pb = np.ascontiguousarray(p[:, band[0]:band[0] + band[1]])
        s0 = some_state(fd, band[1], 3)
        rows = power_sum_rows(n, 7, 3)
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
                        got = plan.api.sdft_smooth_peak_n(plan._p, n, ptr(xs), 7, 3, band[0], band[1], decay, 1, ptr(state), ptr(out))
                        plan.synchronize()
                        assert got == rows, plan.api.last_error()
                        seen.append((host(out).copy(), host(state).copy()))
            if n == 300:
                seq, end = loop(pb, decay, s0)
                same_bits(seen[0][0], held_rows(seq, n, 7, 3, "min"), "one chunk"); same_bits(seen[0][1], end, "one chunk, state")
                assert all(np.array_equal(seen[0][0], o) and np.array_equal(seen[0][1], s) for o, s in seen[1:])
            else:
                # (host samples go in segments: the bits may differ between placements, each is within the bound)
                ref, big, scale = wide(pb, decay, s0)
                for o, s in seen:
                    held_within_bound(o, ref, big, scale, n, 7, 3, "min", "placements"); within_bound(s[None], ref[-1:], big[-1:], scale, "placements, state")


@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_smooth_peak_host_staging_in_segments(combo, hold):
    """a small stage_bytes on host pointers: segments of one chunk each have the loop's bits (state travels between them on the
    device, head rows are joined by the rule); longer segments are within the bound, and of the device-pointer call; decay 0 is
    exact"""
    need_wide(combo)
    fd = fd_of(combo)
    m, n, band, decay = 64, 2000, (3, 50), 0.9
    x, p = burst_expected(combo, "hann", m, n)
    pb = np.ascontiguousarray(p[:, band[0]:band[0] + band[1]])
    s0 = some_state(fd, band[1], 8)
    seq, end = loop(pb, decay, s0)
    ref, big, scale = wide(pb, decay, s0)
    row = band[1] * np.dtype(fd).itemsize
    for every, first, stage, one_chunk in [(1, 0, 300 * row, True), (7, 3, 40 * row, True), (35, 11, 20 * row, False), (1, 0, 700 * row, False)]:      # (segments of 700, 700 and 600 samples: several chunks each)
        with make(m, "hann", combo, stage_bytes=stage, **bit_opts(combo)) as plan:
            plan.reset()
            state = s0.copy()
            got = plan.smooth_peak(x, decay, every, first, bins=band, hold=hold, state=state)
            what = (combo, hold, stage, every, first)
            assert plan.get_option("last_segments") > 1, what
            assert (plan.get_option("last_chunks") == 1) == one_chunk, what
            if one_chunk:
                same_bits(got, held_rows(seq, n, every, first, hold), what); same_bits(state, end, what + ("state",))
            held_within_bound(got, ref, big, scale, n, every, first, hold, what)
            within_bound(state[None], ref[-1:], big[-1:], scale, what + ("state",))
            # the device-pointer call: one forward call of several chunks
            plan.reset()
            dstate = to_dev(s0)
            dev = host(plan.smooth_peak(to_dev(x), decay, every, first, bins=band, hold=hold, state=dstate))
            assert plan.get_option("last_chunks") > 1
            unit = scale * at_ends(big, n, every, first)
            assert (np.abs(got.astype(ref.dtype) - dev.astype(ref.dtype)) <= BOUND * unit).all(), what
            # decay 0: exact, however the call is cut
            plan.reset()
            zero_host = plan.smooth_peak(x, 0.0, every, first, bins=band, hold=hold)
            assert plan.get_option("last_segments") > 1
            plan.reset()
            same_bits(plan.smooth_peak(to_dev(x), 0.0, every, first, bins=band, hold=hold), zero_host, what + ("decay 0",))


@pytest.mark.parametrize("host_side", [False, True])
@pytest.mark.parametrize("combo", ["f32f32", "f32f64"])
def test_smooth_peak_guarded_misaligned_buffers(combo, host_side):
    """peaks and state carved from a guarded arena at every residue modulo 16 their element size allows, and at 16 mod 128; a band
    of 999 bins (an odd row length: consecutive rows change alignment), windows of 7 samples after a head of 3, many of them cut
    by chunk boundaries"""
    need_wide(combo)
    td, fd, _ = O.combo_types(combo)
    m, n, every, first, band = 1000, 2000, 7, 3, (1, 999)
    x, p = expected(combo, "hann", m, n)
    pb = np.ascontiguousarray(p[:, band[0]:band[0] + band[1]])
    s0 = some_state(fd, band[1], 4)
    ref, big, scale = wide(pb, 0.9, s0)
    rows = power_sum_rows(n, every, first)
    size = np.dtype(fd).itemsize
    places = [(r, 16) for r in range(size, 16, size)] + [(16, 128)]
    with make(m, "hann", combo, **bit_opts(combo)) as plan:
        for i, (r, mod) in enumerate(places):
            hold = HOLDS[i % 2]
            arena = (G.HostArena if host_side else G.DeviceArena)(G.room(((n,), td), ((rows, band[1]), fd), ((band[1],), fd)))
            xv = G.put(arena.carve((n,), td, np.dtype(td).itemsize, 16, name="x"), x)
            out = arena.carve((rows, band[1]), fd, r, mod, name="peaks")
            sv = G.put(arena.carve((band[1],), fd, r, mod, name="state"), s0)
            assert G.ptr_of(out) % mod == r and G.ptr_of(sv) % mod == r
            plan.reset()
            plan.api.clear()
            got = plan.api.sdft_smooth_peak_n(plan._p, n, C.c_void_p(G.ptr_of(xv)), every, first, band[0], band[1], 0.9, HOLDS.index(hold),
                                              C.c_void_p(G.ptr_of(sv)), C.c_void_p(G.ptr_of(out)))
            plan.synchronize()
            assert got == rows, plan.api.last_error()
            assert plan.get_option("last_kernel") == KERNEL
            arena.check()
            assert G.view_unwritten(out) == 0
            assert np.array_equal(G.to_numpy(xv), x)
            held_within_bound(G.to_numpy(out), ref, big, scale, n, every, first, hold, (combo, host_side, r, mod, hold))
            within_bound(G.to_numpy(sv)[None], ref[-1:], big[-1:], scale, (combo, host_side, r, mod, "state"))


def test_smooth_peak_async_device_pointers():
    need_wide("f32f64")
    m, n = 1000, 6000
    x, p = burst_expected("f32f64", "hann", m, n)
    ref, big, scale = wide(p[:, :256], 0.9)
    with make(m, "hann", "f32f64", **{"async": 1}) as plan:
        state = to_dev(np.zeros(256))
        a = plan.smooth_peak(to_dev(x), 0.9, 100, 37, bins=(0, 256), hold="min", state=state)
        plan.synchronize()
        extra = BAR * float(p.max())
        held_within_bound(a, ref, big, scale, n, 100, 37, "min", "async", extra=extra)
        within_bound(host(state)[None], ref[-1:], big[-1:], scale, "async, state", extra=extra)


@pytest.mark.parametrize("combo", ["f32f64", "f64f32"])
def test_smooth_peak_same_bits_on_every_run(combo):
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
                    d = plan.smooth_peak(xs, 0.9, every, first, hold=HOLDS[device], state=state)
                    assert plan.get_option("last_chunks") > 1
                    runs.append((host(d), host(state)))
                assert all(np.array_equal(runs[0][0], r[0]) and np.array_equal(runs[0][1], r[1]) for r in runs[1:]), (combo, device, every, first)


@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("m,n,at,opts", [(64, 500, 250, {}), (1000, 6000, 3000, dict(chain=0))], ids=["one-chunk", "serial-carries"])
def test_smooth_peak_nan_rule(m, n, at, opts, hold):
    """a NaN sample reaches every bin and stays in the recurrence: the window that holds it and every later one is NaN, every
    earlier one is what the call gives without it"""
    combo, every, first = "f32f32", 100, 37
    clean = expected(combo, "hann", m, n)[0]
    x = np.array(clean)
    x[at] = np.nan
    with make(m, "hann", combo, **opts) as plan:
        state = np.zeros(m, dtype=np.float32)
        got = plan.smooth_peak(x, 0.9, every, first, hold=hold, state=state)
        assert (plan.get_option("last_chunks") > 1) == (n > 512) and plan.get_option("last_kernel") == KERNEL
        plan.reset()
        want = plan.smooth_peak(clean, 0.9, every, first, hold=hold)
        w = windows(n, every, first)
        before = [r for r, (b, e) in enumerate(w) if e <= at]
        after = [r for r, (b, e) in enumerate(w) if e > at]
        assert before and after and len(before) + len(after) == got.shape[0]
        assert np.isfinite(got[before]).all() and np.array_equal(got[before], want[before])
        assert np.isnan(got[after]).all() and np.isnan(state).all()


def test_smooth_peak_errors():
    combo, m = "f32f32", 64
    x = signal(3000, np.float32, 5)
    top = C.c_size_t(-1).value
    with make(m, "hann", combo) as plan:
        api = plan.api
        plan.smooth_peak(x[:300], 0.5, 7, 3)                         # (errors against a plan that is mid-stream)
        out = np.zeros((12, m), dtype=np.float32)
        state = some_state(np.float32, m, 1)
        kept = state.copy()
        before = plan.state()
        o, s = out.ctypes.data, state.ctypes.data
        refused = [(100, 0, 0, 0, m, 0.5, 0, s, o, "every"),                 # every == 0
                   (100, 10, 0, 0, 0, 0.5, 1, s, o, "nbins"),                # nbins == 0
                   (100, 10, 0, 1, m, 0.5, 0, s, o, "band"),                 # bin0 + nbins > dftsize
                   (100, 10, 0, m, 1, 0.5, 1, s, o, "band"),
                   (100, 10, 0, 2, top, 0.5, 0, s, o, "band"),               # bin0 + nbins overflows to 1
                   (100, 10, 0, 0, m, 0.5, 2, s, o, "hold"),                 # hold is neither 0 nor 1
                   (100, 10, 0, 0, m, 0.5, -1, s, o, "hold"),
                   (0, 10, 0, 0, m, 0.5, 7, s, None, "hold"),                # ... even for a call without samples
                   (100, 10, 0, 0, m, float("nan"), 0, s, o, "decay"),
                   (100, 10, 0, 0, m, -0.25, 1, s, o, "decay"),
                   (100, 10, 0, 0, m, 1.0, 0, s, o, "decay"),
                   (100, 10, 0, 0, m, 1.0 - 2.0 ** -26, 1, s, o, "decay"),   # rounds to 1 in FD float
                   (100, 10, 0, 0, m, float("inf"), 0, s, o, "decay"),
                   (0, 10, 0, 0, m, 2.0, 0, s, None, "decay"),
                   (100, 10, 0, 0, m, 0.5, 0, s, None, "NULL"),              # rows > 0, peaks NULL
                   (100, 10, 5000, 0, m, 0.5, 1, s, None, "NULL")]           # first >= n: the head row is a row
        for n, every, first, bin0, nb, decay, hold, sp, op, word in refused:
            api.clear()
            assert api.sdft_smooth_peak_n(plan._p, n, x.ctypes.data, every, first, bin0, nb, decay, hold, sp, op) == -1, (every, bin0, nb, decay, hold)
            err = api.last_error()
            assert err and "sdft_hip_sdft_smooth_peak_n" in err and word in err, err
            api.clear()
            after = plan.state()
            assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3], (every, bin0, nb, decay, hold)
            assert np.array_equal(state, kept), (every, bin0, nb, decay, hold)
        assert np.count_nonzero(out) == 0
        # n == 0: no rows, nothing moves, peaks may be NULL, state stays
        assert api.sdft_smooth_peak_n(plan._p, 0, x.ctypes.data, 10, 3, 0, m, 0.5, 1, s, None) == 0 and api.last_error() is None
        assert plan.state()[3] == before[3] and np.array_equal(state, kept)
        # the Python call refuses the same before it touches the plan
        for bad in (float("nan"), -0.25, 1.0):
            with pytest.raises(ValueError):
                plan.smooth_peak(x[:10], bad)
        for bad in (2, -1, "peak", None):
            with pytest.raises(ValueError):
                plan.smooth_peak(x[:10], 0.5, hold=bad)
        with pytest.raises(ValueError):
            plan.smooth_peak(x[:10], 0.5, state=np.zeros(m - 1, dtype=np.float32))
        with pytest.raises(ValueError):
            plan.smooth_peak(x[:10], 0.5, every=0)
        after = plan.state()
        assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3]
        assert np.array_equal(state, kept)


def python_in_blocks(combo, m, x, every, block, band, decay, hold):
    with make(m, "hann", combo) as plan:
        state = np.zeros(band[1], dtype=fd_of(combo))
        pieces, firsts, first = [], [], 0
        for t in range(0, x.size, block):
            k = min(block, x.size - t)
            pieces.append(plan.smooth_peak(x[t:t + k], decay, every, first, bins=band, hold=hold, state=state))
            firsts.append(first)
            first = every_next_first(k, every, first)
        return stream_join(pieces, firsts, hold, fd_of(combo), band[1]), state


def run_host(tmp_path, exe, combo, hold, word):
    fd = fd_of(combo)
    m, n, every, block, band, decay = 64, 2000, 7, 330, (3, 50), 0.96875
    x, p = expected(combo, "hann", m, n)
    x.tofile(tmp_path / "x.raw")
    r = subprocess.run([str(exe), str(m), str(every), str(block), str(band[0]), str(band[1]), repr(decay), str(HOLDS.index(hold)),
                        str(tmp_path / "x.raw"), str(tmp_path / "s.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert word in r.stdout
    got = np.fromfile(tmp_path / "s.raw", dtype=fd).reshape(-1, band[1])
    # blocks of 330 samples are one chunk each: the loop's extremes over the whole signal, and the state's behind the last row
    seq, end = loop(np.ascontiguousarray(p[:, band[0]:band[0] + band[1]]), decay)
    same_bits(got[:-1], held_rows(seq, n, every, 0, hold), (word, combo, hold))
    same_bits(got[-1], end, (word, combo, hold, "state"))
    rows, state = python_in_blocks(combo, m, x, every, block, band, decay, hold)
    assert np.array_equal(got[:-1], rows) and np.array_equal(got[-1], state)


@pytest.mark.parametrize("flags,combo,hold", [([], "f32f64", "min"), (["-DSDFT_FD_FLOAT"], "f32f32", "max")])
def test_c_host_smooth_peak(tmp_path, hip_library, flags, combo, hold):
    libdir = os.path.dirname(hip_library)
    rt = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    exe = tmp_path / "host_smooth_peak"
    cmd = ["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), *flags,
           os.path.join(ROOT, "tests", "c", "host_smooth_peak.c"), "-o", str(exe),
           "-L", libdir, "-lsdft_hip", "-L", rt, "-lamdhip64", "-lm", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{rt}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run_host(tmp_path, exe, combo, hold, "C-HOST-SMOOTH-PEAK ok")


@pytest.mark.parametrize("t,f,combo,hold", [("float", "double", "f32f64", "max"), ("float", "float", "f32f32", "min")])
def test_cpp_host_smooth_peak(tmp_path, hip_library, t, f, combo, hold):
    libdir = os.path.dirname(hip_library)
    rt = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    exe = tmp_path / "host_smooth_peak_cpp"
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", f"-DHOST_T={t}", f"-DHOST_F={f}", "-I", os.path.join(ROOT, "include", "cpp"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "host_smooth_peak.cpp"), "-o", str(exe),
           "-L", libdir, "-lsdft_hip", "-L", rt, "-lamdhip64", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{rt}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run_host(tmp_path, exe, combo, hold, "CPP-SMOOTH-PEAK ok")
