"""Filterbank analysis (sdft_hip_set_filterbank, sdft_hip_sdft_filterbank_n, SDFT.filterbank) on a real MI355X against the oracle.

The expected powers are those of tests/test_gpu_power.py: the oracle fed in blocks, re*re + im*im of its rows kept in the FD
dtype, never a complex matrix.  With W the dense band matrix, the reference value is W @ p and T = |W| @ p, both in float64
(on the device: the products of a parity case are 10^12).  The bars are the contract's, element by element, L the band's bin
count, u = 2^-24 / 2^-53, gamma_n = n u / (1 - n u), eta the smallest positive subnormal of the FD type:
    FD float    gamma_(L+1) T + L eta      float64 products are exact and the float64 sum's own error is below 2^-28 T
    FD double   2 gamma_L T + L eta        the float64 evaluation itself errs by up to gamma_L T
and on the inexact route (FD double with the default carries) the power call's term deviation on top: BAR of
tests/test_gpu_power.py (2.1e-11) times the largest power on the call's grid times sum |w|.  Every element of every row is compared."""

import ctypes as C

import numpy as np
import pytest

import guarded as G
from oracle import oracle as O
from sdft_amd import filterbank as F
from test_gpu_power import BAR, WINDOWS, MS, exact_combo, expected, make, on_grid, rel, signal, to_dev

pytestmark = pytest.mark.gpu
GRIDS = [(1, 0), (7, 6), (100, 0), (1024, 1023)]


# ---------------------------------------------------------------------------------------------
# filterbanks
# ---------------------------------------------------------------------------------------------
def whole_row(m):
    return np.array([0], dtype=np.uint64), np.array([m], dtype=np.uint64), np.ones(m)


def one_bin_bands(m):
    return np.arange(m, dtype=np.uint64), np.ones(m, dtype=np.uint64), np.ones(m)


def random_bands(m, seed=None):
    """3 m bands (more bands than bins): starts over the whole row, lengths from 1 to m (band 0 is the whole row, band 1 one bin),
    bands that straddle the bins 61/62 and 123/124 (the first tile boundaries at 62 bins per tile and at 2 x 62), weights drawn from
    {0, 1, -0.5, uniform in [2^-10, 1]}"""
    rng = np.random.default_rng(1000 + m if seed is None else seed)
    nb = 3 * m
    start = rng.integers(0, m, nb)
    length = 1 + (rng.random(nb) * rng.random(nb) * (m - start)).astype(np.int64)      # short bands are the many, long ones the few
    length = np.minimum(length, m - start)
    start[0], length[0] = 0, m
    start[1], length[1] = m - 1, 1
    fixed = [b for b in ((61, 2), (60, 4), (123, 2), (120, 8), (61, 63)) if b[0] + b[1] <= m]
    for i, (s, k) in enumerate(fixed):
        start[2 + i], length[2 + i] = s, k
    assert (length >= 1).all() and (start + length <= m).all() and length.max() == m
    total = int(length.sum())
    kind = rng.integers(0, 4, total)
    w = np.choose(kind, [np.zeros(total), np.ones(total), np.full(total, -0.5), rng.uniform(2.0 ** -10, 1.0, total)])
    return start.astype(np.uint64), length.astype(np.uint64), w


def banks_of(m):
    banks = [("whole row", whole_row(m)), ("one-bin bands", one_bin_bands(m)), ("random", random_bands(m))]
    if m >= 64:
        banks.append(("mel", F.mel(m, 48000, min(40, m))))
    return banks


def in_fd(bank, fd):
    """the weights as the plan holds them (rounded to the FD type once, here)"""
    return bank[0], bank[1], np.asarray(bank[2]).astype(fd)


# ---------------------------------------------------------------------------------------------
# reference and bars
# ---------------------------------------------------------------------------------------------
def reference(bank, p64):
    """(W @ p, |W| @ p, L, sum |w|) for the rows of p64 (a float64 device tensor [rows][m]); W from the FD weights"""
    import torch
    W = torch.from_numpy(F.dense(p64.shape[1], *bank).astype(np.float64)).cuda()
    R = p64 @ W.T
    T = p64 @ W.abs().T
    L = torch.from_numpy(np.asarray(bank[1]).astype(np.float64)).cuda()
    return R, T, L, W.abs().sum(dim=1)


def bar_of(fd, T, L, sum_w, inexact_scale):
    single = np.dtype(fd) == np.float32
    u = 2.0 ** -24 if single else 2.0 ** -53
    eta = 2.0 ** -149 if single else 5e-324
    if single:
        gamma = (L + 1) * u / (1 - (L + 1) * u)
        bar = gamma * T + L * eta
    else:
        gamma = L * u / (1 - L * u)
        bar = 2 * gamma * T + L * eta
    if inexact_scale:
        bar = bar + BAR * inexact_scale * sum_w
    return bar


def check_rows(got, R, T, L, sum_w, fd, inexact_scale, what):
    import torch
    got = got if hasattr(got, "cpu") else torch.from_numpy(got).cuda()
    assert tuple(got.shape) == tuple(R.shape) and got.dtype == getattr(torch, np.dtype(fd).name), (what, got.shape, R.shape, got.dtype)
    err = (got.double() - R).abs()
    bar = bar_of(fd, T, L, sum_w, inexact_scale)
    bad = ~(err <= bar)                                       # (a NaN fails)
    worst = float((err / torch.clamp(bar, min=1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: largest error / bar = {worst:.3g}")
    assert not bool(bad.any()), (what, int(bad.sum()), worst)


# ---------------------------------------------------------------------------------------------
# parity: every type pair x window x dftsize x filterbank x grid
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("m", MS)
def test_filterbank_parity(m, window, combo):
    import torch
    fd = O.combo_types(combo)[1]
    n = 10000 if m == 4096 else 6000            # several chunks, and a roll-over at 2N
    x, want = expected(combo, window, m, n)
    dx = to_dev(x)
    p64 = torch.from_numpy(np.array(want)).cuda().double()
    with make(m, window, combo) as p:
        for b, (name, bank) in enumerate(banks_of(m)):
            bank = in_fd(bank, fd)
            p.set_filterbank(*bank)
            assert p.filterbank_bands == bank[0].size
            R, T, L, sum_w = reference(bank, p64)
            for g, (every, first) in enumerate(GRIDS):
                p.reset()
                got = p.filterbank(dx if (b + g) % 2 else x, every, first)          # host and device memory alternate
                assert p.get_option("last_kernel") == 7, (m, name, every, first)
                if m >= 1000:
                    assert p.get_option("last_chunks") > 1, (m, name, every, first)
                inexact = 0.0 if exact_combo(combo) else float(p64[first::every].max())
                check_rows(got, R[first::every], T[first::every], L, sum_w, fd, inexact, (combo, window, m, name, every, first))
                del got
            del R, T


# ---------------------------------------------------------------------------------------------
# bit-exact cases
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
def test_one_bin_bands_are_the_power_call(combo):
    """dftsize one-bin bands of weight 1 against SDFT.power of the same call on a twin plan with the same options, bit for bit on
    every route: one chunk, chunk-parallel (default FD double: the inexact route, where both calls make the same chunks), exact
    carries, host and device memory"""
    td, fd, _ = O.combo_types(combo)
    call = 0
    for m, n, opts in ((64, 500, {}), (125, 6000, {}), (1000, 6000, {}), (1024, 6000, {"carry": 1})):
        x = signal(n, td, m)
        with make(m, "hann", combo, **opts) as p, make(m, "hann", combo, **opts) as q:
            p.set_filterbank(*in_fd(one_bin_bands(m), fd))
            for every, first in GRIDS[:3]:
                p.reset(); q.reset()
                call += 1
                xs = to_dev(x) if call % 2 else x
                got, want = p.filterbank(xs, every, first), q.power(xs, every, first)
                assert p.get_option("last_kernel") == 7 and q.get_option("last_kernel") == 5
                assert p.get_option("last_chunks") == q.get_option("last_chunks")
                got, want = (v.cpu().numpy() if hasattr(v, "cpu") else v for v in (got, want))
                assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want), (combo, m, every, first)


@pytest.mark.parametrize("combo,opts", [("f32f32", {}), ("f64f32", {}), ("f32f64", {"carry": 1}), ("f64f64", {"carry": 1})])
def test_two_bin_bands_are_two_rounded_products_and_their_sum(combo, opts):
    """bands (k, 2) for every k, tile boundaries included, on the routes that are bit-identical to the reference: exactly numpy's
    w0 * p0 + w1 * p1 in the FD dtype"""
    td, fd, _ = O.combo_types(combo)
    for m in (2, 125, 1000):
        n = 6000
        x, pw = expected(combo, "hann", m, n)
        rng = np.random.default_rng(m)
        w = rng.uniform(-1.0, 1.0, (m - 1, 2)).astype(fd)
        with make(m, "hann", combo, **opts) as p:
            p.set_filterbank(np.arange(m - 1), np.full(m - 1, 2), w.ravel())
            for i, (every, first) in enumerate(((1, 0), (100, 37))):
                p.reset()
                got = p.filterbank(to_dev(x) if i else x, every, first)
                got = got.cpu().numpy() if hasattr(got, "cpu") else got
                rows = on_grid(pw, every, first)
                want = w[:, 0] * rows[:, :-1] + w[:, 1] * rows[:, 1:]
                assert want.dtype == fd and np.array_equal(got, want), (combo, m, every, first)


# ---------------------------------------------------------------------------------------------
# streaming, chunking, state, determinism
# ---------------------------------------------------------------------------------------------
EXACT = [("f32f32", {}), ("f64f32", {}), ("f32f64", {"carry": 1}), ("f64f64", {"carry": 1})]


@pytest.mark.parametrize("combo,opts", EXACT)
def test_filterbank_streaming_and_chunking_bit_identical(combo, opts):
    """one call of n samples against calls of ragged lengths chained by the documented next first: the same rows and the same final
    state, bit for bit; and the one call with option chunk forced to two other values: the same rows (a row's bits do not depend
    on the time chunking)"""
    from sdft_amd.sdft import every_next_first
    td, fd, _ = O.combo_types(combo)
    m, n = 1000, 6000
    lengths = [1, 511, 512, 513, 3000]
    lengths.append(n - sum(lengths))
    x = signal(n, td, 21)
    bank = in_fd(random_bands(m), fd)
    for every in (1, 100):
        with make(m, "hann", combo, **opts) as p, make(m, "hann", combo, **opts) as q:
            p.set_filterbank(*bank); q.set_filterbank(*bank)
            whole = p.filterbank(to_dev(x), every, 0).cpu().numpy()
            chunks = p.get_option("last_chunks")
            assert chunks > 1
            got, t, first = [], 0, 0
            for i, k in enumerate(lengths):
                xs = x[t:t + k]
                d = q.filterbank(to_dev(xs) if i % 2 else xs, every, first)
                got.append(d.cpu().numpy() if hasattr(d, "cpu") else d)
                first = every_next_first(k, every, first)
                t += k
            assert np.array_equal(np.concatenate(got), whole), (combo, every)
            for a, b in zip(p.state()[:3], q.state()[:3]):
                assert np.array_equal(a, b), (combo, every)
            assert p.state()[3] == q.state()[3]
            for forced in (256, 1024):
                p.reset()
                p.set_option("chunk", forced)
                again = p.filterbank(to_dev(x), every, 0).cpu().numpy()
                assert p.get_option("last_chunks") not in (1, chunks), (forced, chunks)
                assert np.array_equal(again, whole), (combo, every, forced)
            p.set_option("chunk", 0)


@pytest.mark.parametrize("combo", O.COMBOS)
def test_state_after_a_filterbank_call_is_sdft_n_s(combo):
    """sdft_sdft_n of further samples gives, after a filterbank call, the rows it gives after sdft_sdft_n of the same prefix"""
    td, fd, _ = O.combo_types(combo)
    m, n, more = 1000, 6000, 700
    x = signal(n + more, td, 31)
    with make(m, "hann", combo) as p, make(m, "hann", combo) as q:
        p.set_filterbank(*in_fd(F.mel(m, 48000, 40), fd))
        p.filterbank(to_dev(x[:n]), 100, 5)
        q.sdft(to_dev(x[:n]))
        a, b = p.sdft(x[n:]), q.sdft(x[n:])
        if exact_combo(combo):
            assert np.array_equal(a, b)
        else:
            assert rel(a, b) <= 1e-11, rel(a, b)
        assert p.state()[3] == q.state()[3]


@pytest.mark.parametrize("combo", O.COMBOS)
def test_filterbank_is_deterministic(combo):
    td, fd, _ = O.combo_types(combo)
    m, n = 1024, 6000
    x = signal(n, td, 41)
    bank = in_fd(random_bands(m), fd)
    outs = []
    for _ in range(2):
        with make(m, "blackman", combo) as p:
            p.set_filterbank(*bank)
            outs.append(p.filterbank(to_dev(x), 3, 1).cpu().numpy())
            assert p.get_option("last_chunks") > 1
    assert outs[0].tobytes() == outs[1].tobytes()


@pytest.mark.parametrize("combo,opts", [("f32f32", {}), ("f32f64", {"carry": 1})])
def test_filterbank_batched_channels(combo, opts):
    """a 3-channel plan, out [3][rows][nbands], against three single-channel plans, bit for bit (on the routes whose values do not
    depend on the time chunks, which the channel count changes)"""
    td, fd, _ = O.combo_types(combo)
    ch, m, n = 3, 256, 6000
    x = np.stack([signal(n, td, 200 + c) for c in range(ch)])
    bank = in_fd(random_bands(m), fd)
    for device in (False, True):
        for every, first in ((100, 50), (3, 1)):
            with make(m, "blackman", combo, channels=ch, **opts) as p:
                p.set_filterbank(*bank)
                got = p.filterbank(to_dev(x) if device else x, every, first)
                got = got.cpu().numpy() if device else got
                assert p.get_option("last_kernel") == 7
            assert got.shape[0] == ch and got.shape[2] == bank[0].size
            for c in range(ch):
                with make(m, "blackman", combo, **opts) as q:
                    q.set_filterbank(*bank)
                    assert np.array_equal(got[c], q.filterbank(x[c], every, first)), (combo, device, every, c)


# ---------------------------------------------------------------------------------------------
# no overrun, no hole, at the least alignment an element allows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("combo", ["f32f32", "f32f64"])
def test_filterbank_guarded_misaligned_output(combo, host):
    """out carved from a guarded arena at residue sizeof(fd) of a 16-byte address, an odd number of bands (consecutive rows change
    alignment), split bands among them"""
    import torch
    td, fd, _ = O.combo_types(combo)
    m, n, every, first = 1000, 2000, 3, 1
    x, p_all = expected(combo, "hann", m, n)
    bank = in_fd(random_bands(m), fd)
    bank = (bank[0][:-1], bank[1][:-1], bank[2][:int(bank[1][:-1].sum())])
    nbands = bank[0].size
    assert nbands % 2 == 1
    rows = on_grid(p_all, every, first).shape[0]
    size = np.dtype(fd).itemsize
    R, T, L, sum_w = reference(bank, torch.from_numpy(np.array(on_grid(p_all, every, first))).cuda().double())
    with make(m, "hann", combo) as p:
        p.set_filterbank(*bank)
        arena = (G.HostArena if host else G.DeviceArena)(G.room(((n,), td), ((rows, nbands), fd)))
        xv = G.put(arena.carve((n,), td, np.dtype(td).itemsize, 16, name="x"), x)
        out = arena.carve((rows, nbands), fd, size, 16, name="out")
        assert G.ptr_of(out) % 16 == size
        p.api.clear()
        got = p.api.sdft_filterbank_n(p._p, n, C.c_void_p(G.ptr_of(xv)), every, first, C.c_void_p(G.ptr_of(out)))
        p.synchronize()
        assert got == rows, p.api.last_error()
        assert p.get_option("last_kernel") == 7 and p.get_option("last_chunks") > 1
        arena.check()
        assert G.view_unwritten(out) == 0
        assert np.array_equal(G.to_numpy(xv), x)
        inexact = 0.0 if exact_combo(combo) else float(on_grid(p_all, every, first).max())
        check_rows(np.ascontiguousarray(G.to_numpy(out)), R, T, L, sum_w, fd, inexact, (combo, host))


# ---------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------
def test_filterbank_errors_leave_state_and_filterbank_untouched():
    combo, m = "f32f32", 64
    x = signal(3000, np.float32, 5)
    sz = np.uint64
    with make(m, "hann", combo) as p:
        api = p.api
        out = np.zeros((10, m), dtype=np.float32)
        # no filterbank installed
        api.clear()
        assert p.filterbank_bands == 0
        assert api.sdft_filterbank_n(p._p, 100, x.ctypes.data, 10, 0, out.ctypes.data) == -1
        err = api.last_error()
        assert err and "sdft_hip_sdft_filterbank_n" in err and "filterbank" in err, err
        api.clear()
        with pytest.raises(ValueError):
            p.filterbank(x[:10])
        bank = in_fd(random_bands(m), np.float32)
        p.set_filterbank(*bank)
        nbands = bank[0].size
        assert p.filterbank_bands == nbands
        p.filterbank(x[:300])                                 # (errors against a plan that is mid-stream)
        before = p.state()
        with make(m, "hann", combo) as q:                     # what the installed filterbank gives from here on
            q.set_filterbank(*bank)
            q.filterbank(x[:300])
            want = q.filterbank(x[300:900], 7, 2)

        def untouched(what):
            after = p.state()
            assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3], what
            assert p.filterbank_bands == nbands, what

        big = np.zeros((10, nbands), dtype=np.float32)
        for n, every, ptr, word in [(100, 0, big.ctypes.data, "every"), (100, 10, None, "NULL")]:
            api.clear()
            assert api.sdft_filterbank_n(p._p, n, x.ctypes.data, every, 0, ptr) == -1, word
            err = api.last_error()
            assert err and "sdft_hip_sdft_filterbank_n" in err and word in err, err
            api.clear()
            untouched(word)
        w = np.ones(8, dtype=np.float32)
        refused = [(np.array([0, m - 3], dtype=sz), np.array([4, 4], dtype=sz), w.ctypes.data, "dftsize"),      # a band past dftsize
                   (np.array([0, m], dtype=sz), np.array([4, 1], dtype=sz), w.ctypes.data, "dftsize"),
                   (np.array([0, 2], dtype=sz), np.array([4, C.c_size_t(-1).value], dtype=sz), w.ctypes.data, "dftsize"),
                   (np.array([0, 9], dtype=sz), np.array([4, 0], dtype=sz), w.ctypes.data, "no bins"),          # a band of zero bins
                   (np.array([0, 9], dtype=sz), np.array([4, 4], dtype=sz), None, "NULL")]
        for b0, nb, wp, word in refused:
            api.clear()
            assert api.set_filterbank(p._p, 2, b0.ctypes.data, nb.ctypes.data, wp) == -1, word
            err = api.last_error()
            assert err and "sdft_hip_set_filterbank" in err and word in err, err
            api.clear()
            untouched(word)
        # n == 0: no rows, nothing moves
        assert api.sdft_filterbank_n(p._p, 0, x.ctypes.data, 10, 0, None) == 0 and api.last_error() is None
        untouched("n == 0")
        # the installed filterbank still answers as before
        assert np.array_equal(p.filterbank(x[300:900], 7, 2), want)
        # first >= n: no rows, out may be NULL, the state advances
        assert p.filterbank(x[900:1300], 10, 400).shape == (0, nbands)
        # no bands: the filterbank is removed
        p.set_filterbank([], [], [])
        assert p.filterbank_bands == 0
        api.clear()
        assert api.sdft_filterbank_n(p._p, 100, x.ctypes.data, 10, 0, big.ctypes.data) == -1
        api.clear()
