"""Array covariance analysis (sdft_hip_set_array, sdft_hip_sdft_covariance_n, SDFT.covariance) on a real MI355X against the oracle
and against the pooled cross-spectrum call, whose bits it promises.

Signals, the oracle's rows, the numpy term expression, the compensated prefix sums with their math.fsum spot checks and the bar are
those of tests/test_gpu_cross_sum.py (rows_of, check_pairs: gamma_L sum |term| on the bit-identical routes, L BAR max|X_a| max|X_b|
on top for FD double's default carries); the grids are GRIDS of tests/test_gpu_power_sum.py.  Nothing is tolerated here that is not
tolerated there.

Plans have 9 channels at m in {5, 64, 125} and 5 at m in {1000, 1024}.  The arrays are one below, at and one above every group
size the kernel can be built for (1, 2, 4, 8), in plan order and permuted, and subsets that leave channels to advance-only items:
element p(i, j) of an array `chan` is the pair (chan[i], chan[j]) of check_pairs.  n = 6000: several chunks, and a roll-over of the
cursor at 2 x dftsize."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import guarded as G
from oracle import oracle as O
from sdft_amd.sdft import SdftHipError, covariance_matrix, covariance_pairs, every_next_first, power_sum_rows
from sdft_amd.signals import noise
from test_gpu_cross_sum import check_pairs, check_state, fnv1a, host_link, plan, rows_of, same_bits, signals
from test_gpu_power import bands_of, exact_combo, make, rel, signal, to_dev
from test_gpu_power_sum import GRIDS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 6000
ARRAYS9 = [[0], [0, 1], [2, 0, 1], [0, 1, 2, 3], [4, 0, 5, 2, 1], list(range(8)), list(range(9)), [8, 3]]
ARRAYS5 = [list(range(5)), [3, 1]]
MIXED = [4, 0, 5, 2, 1]                                      # two groups of 4; the channels 3, 6, 7, 8 only advance


def pairs_of(chan):
    """the channel pairs of the upper triangle, in the output's order"""
    a, b = covariance_pairs(len(chan))
    return [(chan[i], chan[j]) for i, j in zip(a.tolist(), b.tolist())]


def array_plan(m, window, combo, chan, channels, **opts):
    p = make(m, window, combo, channels=channels, **opts)
    p.set_array(chan)
    assert p.array_channels == len(chan)
    return p


def numpy_of(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def shape_of(m):
    return (9, ARRAYS9) if m < 1000 else (5, ARRAYS5)


def two_bands(m, p):
    """as test_cross_sum_parity chooses them: one across the first tile boundaries with an odd start, one inside the last tile"""
    bs = bands_of(m, p)
    return list(dict.fromkeys([(50, 100) if (50, 100) in bs else bs[3] if len(bs) > 3 else bs[0], bs[-1]]))


# ---------------------------------------------------------------------------------------------
# parity: every type pair x window x dftsize x array x band, the grids in turn
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [5, 64, 125, 1000, 1024])
@pytest.mark.parametrize("window", ["hann", "blackman"])
@pytest.mark.parametrize("combo", O.COMBOS)
def test_covariance_parity(combo, window, m):
    channels, arrays = shape_of(m)
    x, X = rows_of(combo, window, m, N, None, channels)
    dx = to_dev(x)
    call = 0
    with make(m, window, combo, channels=channels) as p:
        bands = two_bands(m, p)
        caches = {band: {} for band in bands}            # (the reference's terms and prefix sums of a band, shared by arrays and grids)
        for ai, chan in enumerate(arrays):
            p.set_array(chan)
            pairs = pairs_of(chan)
            for bi, band in enumerate(bands):
                # three of the nine grids per (array, band), all nine over any three consecutive ones
                for every, first in GRIDS[(2 * ai + bi) % 3::3]:
                    p.reset()
                    call += 1
                    got = p.covariance(dx if call % 2 else x, every, first, bins=band)
                    what = (combo, window, m, chan, every, first, band)
                    assert p.get_option("last_kernel") == 9, what
                    if m >= 1000:
                        assert p.get_option("last_chunks") > 1, what
                    check_pairs(got, X, pairs, N, every, first, band, exact_combo(combo), what, cache=caches[band])
        # bins=None is the whole row
        p.reset()
        check_pairs(p.covariance(x, 7, 6), X, pairs, N, 7, 6, (0, m), exact_combo(combo), (combo, window, m, "bins=None"))


# ---------------------------------------------------------------------------------------------
# promise (2): every element has the cross-spectrum call's bits; the diagonal is the power call's value
# ---------------------------------------------------------------------------------------------
BITS_CASES = [("f32f32", {}, N), ("f64f32", {}, N), ("f32f64", dict(carry=1), N), ("f64f64", dict(carry=1), N),
              ("f32f64", dict(chunk=1000), N), ("f32f64", dict(chunk=64), N), ("f32f64", {}, 500), ("f64f64", {}, 500), ("f32f32", {}, 500)]


@pytest.mark.parametrize("combo,opts,n", BITS_CASES, ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) or "default" if isinstance(v, dict) else str(v))
def test_covariance_has_the_cross_spectrum_calls_bits(combo, opts, n):
    """a twin plan with set_pairs(covariance_pairs) returns the same bits for every element: on FD float by default, on FD double
    with carry = 1, on FD double's default carries when both plans cut time alike (option "chunk"), and for a call of one chunk.
    The two calls cut time into chunks of the same length in every case (asserted, never assumed)."""
    td = O.combo_types(combo)[0]
    for m in (125, 1000):
        channels, arrays = shape_of(m)
        x = np.ascontiguousarray(signals(td, N, m, channels)[:, :n])
        for k, chan in enumerate(arrays if m >= 1000 else [MIXED, list(range(9)), [8, 3], [2, 0, 1]]):
            pairs = pairs_of(chan)
            with array_plan(m, "hann", combo, chan, channels, **opts) as p, plan(m, "hann", combo, pairs=pairs, channels=channels, **opts) as q:
                bands = two_bands(m, p)
                for i, (every, first) in enumerate([(1, 0), (100, 37), (1024, 1023), (N, 0)]):
                    band = bands[(i + k) % 2]
                    xs = to_dev(x) if (i + k) % 2 else x
                    p.reset(); q.reset()
                    got, want = numpy_of(p.covariance(xs, every, first, bins=band)), numpy_of(q.cross_sum(xs, every, first, bins=band))
                    what = (combo, opts, n, m, chan, every, first, band)
                    assert p.get_option("last_kernel") == 9 and q.get_option("last_kernel") == 8, what
                    assert p.get_option("last_chunk_len") == q.get_option("last_chunk_len"), (what, p.get_option("last_chunk_len"), q.get_option("last_chunk_len"))
                    assert (p.get_option("last_chunks") > 1) == (n >= 512), what
                    if "chunk" in opts:
                        assert p.get_option("last_chunk_len") == opts["chunk"], what
                    assert same_bits(got, want), (what, int(np.count_nonzero(got.view(want.real.dtype) != want.view(want.real.dtype))))


@pytest.mark.parametrize("combo,opts", [("f32f32", {}), ("f64f32", {}), ("f32f64", dict(carry=1)), ("f32f64", dict(chunk=1000)), ("f64f64", dict(chunk=64))],
                         ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) or "default" if isinstance(v, dict) else str(v))
def test_covariance_diagonal_is_the_power_call(combo, opts):
    """at every = 1, first = 0, p(i, i).re is power() of a third plan bit for bit and im is all +0"""
    td = O.combo_types(combo)[0]
    for m, chan in [(125, MIXED), (125, list(range(9))), (1000, [3, 1]), (1000, list(range(5)))]:
        channels, _ = shape_of(m)
        x = signals(td, N, m, channels)
        with array_plan(m, "hann", combo, chan, channels, **opts) as p, make(m, "hann", combo, channels=channels, **opts) as q:
            band = two_bands(m, p)[0]
            cov = p.covariance(x, 1, 0, bins=band)
            pw = q.power(x, 1, 0, bins=band)
            what = (combo, opts, m, chan)
            assert p.get_option("last_chunks") > 1 and p.get_option("last_chunk_len") == q.get_option("last_chunk_len"), what
            nch = len(chan)
            for i in range(nch):
                d = cov[i * nch - i * (i - 1) // 2]
                assert same_bits(d.real.copy(), pw[chan[i]].copy()), (what, i)
                assert same_bits(d.imag.copy(), np.zeros_like(d.imag)), (what, i)
            # the host's mirror: Hermitian, the diagonal as returned
            mat = covariance_matrix(cov[:, :3], nch)
            assert mat.shape == (3, band[1], nch, nch) and np.array_equal(mat, np.conj(np.swapaxes(mat, -1, -2)))


@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_covariance_group_sizes_give_the_same_bits(combo):
    """the group size is a matter of speed alone: the candidates of the hooks build (option "array_group") return the bits of the
    product's choice, for arrays below, at and above each of them"""
    td = O.combo_types(combo)[0]
    m, band = 125, (1, 123)
    x = to_dev(signals(td, N, m, 9))
    opts = {} if exact_combo(combo) else dict(chunk=200)     # (FD double's default carries: the same chunks whatever the item count)
    for chan in ([0], [2, 0, 1], MIXED, list(range(9))):
        with array_plan(m, "blackman", combo, chan, 9, **opts) as p:
            default = p.get_option("array_group")
            want = numpy_of(p.covariance(x, 100, 37, bins=band))
            assert p.get_option("last_kernel") == 9 and p.get_option("last_chunks") > 1
            before = p.state()
            for group in (1, 2, 4):
                p.reset()
                p.set_option("array_group", group)
                assert p.get_option("array_group") == group and p.array_channels == len(chan)
                got = numpy_of(p.covariance(x, 100, 37, bins=band))
                assert same_bits(got, want), (combo, chan, group, default)
                after = p.state()
                assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3], (combo, chan, group)


# ---------------------------------------------------------------------------------------------
# state, streaming, determinism
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
def test_covariance_leaves_the_state_of_sdft(combo):
    """after the call the state of all nine channels -- members of a diagonal block, of several blocks, of a padded group, and the
    channels outside the array -- is the one sdft of the same samples leaves on a twin plan: bit for bit on the exact routes, within
    check_state's bar with FD double's default carries.  A following sdft and isdft continue."""
    td = O.combo_types(combo)[0]
    m = 125
    x = signals(td, N, m, 9)
    hop = np.stack([noise(100, seed=12 + c, dtype=td) for c in range(9)])
    eps = float(np.finfo(td).eps)
    k = 0
    for opts in ([{}, dict(carry=1)] if not exact_combo(combo) else [{}]):
        exact = exact_combo(combo) or "carry" in opts
        for chan in (MIXED, list(range(9)), [8, 3]):
            k += 1
            with array_plan(m, "hann", combo, chan, 9, **opts) as p, make(m, "hann", combo, channels=9, **opts) as q:
                p.covariance(to_dev(x) if k % 2 else x, 100, 37, bins=(10, 100))
                assert p.get_option("last_kernel") == 9 and p.get_option("last_chunks") > 1
                q.sdft(x)
                check_state(p, q, exact, (combo, opts, chan))
                dp, dq = p.sdft(hop), q.sdft(hop)
                yp, yq = p.isdft(dp), q.isdft(dq)
                if exact:
                    assert np.array_equal(dp, dq) and np.array_equal(yp, yq)
                else:
                    assert rel(dp, dq) <= 1e-10, rel(dp, dq)
                    assert float(np.abs(yp - yq).max()) <= 1e-10 * float(np.abs(dq).max()) + 2 * eps * float(np.abs(yq).max())


@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("every,first0", [(100, 37), (1024, 1023)])
def test_covariance_streaming(combo, every, first0):
    m, band = 125, (10, 100)
    lengths = [1, 99, 100, 511, 512, 513, 3000]
    lengths.append(N - sum(lengths))
    x, X = rows_of(combo, "hann", m, N, None, 9)
    with array_plan(m, "hann", combo, MIXED, 9) as p:
        rows, t, first = None, 0, first0
        for i, k in enumerate(lengths):
            xs = np.ascontiguousarray(x[:, t:t + k])
            d = numpy_of(p.covariance(to_dev(xs) if i % 3 == 1 else xs, every, first, bins=band))
            assert d.shape == (15, power_sum_rows(k, every, first), band[1]) and p.get_option("last_kernel") == 9
            if first > 0 and t > 0:
                rows[:, -1] += d[:, 0]                   # the head completes the previous call's last row: the host adds the two
                d = d[:, 1:]
            rows = d.copy() if rows is None else np.concatenate([rows, d], axis=1)
            first = every_next_first(k, every, first)
            t += k
        check_pairs(rows, X, pairs_of(MIXED), N, every, first0, band, exact_combo(combo), (combo, every, first0, "streamed"))


@pytest.mark.parametrize("combo", ["f32f64", "f64f32"])
def test_covariance_same_bits_on_every_run(combo):
    m = 1000
    x = signals(O.combo_types(combo)[0], N, m, 5)
    for device in (False, True):
        xs = to_dev(x) if device else x
        with array_plan(m, "hann", combo, list(range(5)), 5) as p:
            for every, first in [(100, 37), (N, 0)]:
                runs = []
                for _ in range(3):
                    p.reset()
                    runs.append(numpy_of(p.covariance(xs, every, first, bins=(1, 998))))
                    assert p.get_option("last_chunks") > 1
                assert same_bits(runs[0], runs[1]) and same_bits(runs[0], runs[2]), (combo, device, every, first)


# ---------------------------------------------------------------------------------------------
# forced routes (the hooks build where the key is a hook), host staging
# ---------------------------------------------------------------------------------------------
ROUTES = [dict(prefix_cells=2), dict(prefix_cells=0), dict(carry=1, chain=0), dict(carry=1, chain=2), dict(fft_carry=0), dict(xcd_map=0),
          dict(chunk=64), dict(chunk=1000)]


@pytest.mark.parametrize("opts", ROUTES, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
@pytest.mark.parametrize("m", [125, 1000])
def test_covariance_forced_routes(m, opts):
    combo, chan = "f32f64", MIXED if m == 125 else [3, 1]
    channels, _ = shape_of(m)
    x, X = rows_of(combo, "hann", m, N, None, channels)
    exact = "carry" in opts
    with array_plan(m, "hann", combo, chan, channels, **opts) as p, make(m, "hann", combo, channels=channels, **opts) as q:
        band = two_bands(m, p)[0]
        q.sdft(x)
        for i, (every, first) in enumerate([(1, 0), (100, 37), (N, 0)]):
            p.reset()
            got = p.covariance(to_dev(x) if i % 2 else x, every, first, bins=band)
            assert p.get_option("last_kernel") == 9 and p.get_option("last_chunks") > 1, (m, opts)
            if "chunk" in opts:
                assert p.get_option("last_chunk_len") == opts["chunk"]
            check_pairs(got, X, pairs_of(chan), N, every, first, band, exact, (m, opts, every, first))
            check_state(p, q, exact, (m, opts, every, first))


@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_covariance_host_staging_in_segments(combo):
    """stage_bytes small enough for several segments: windows shorter than a segment, longer than one, and one over all of them;
    host samples with host and with device sums (the joined head rows)"""
    import torch
    fd = O.combo_types(combo)[1]
    m, band, chan = 125, (10, 100), [2, 0, 1]
    x, X = rows_of(combo, "hann", m, N, None, 9)
    pairs = pairs_of(chan)
    row = len(pairs) * 2 * band[1] * np.dtype(fd).itemsize
    for stage, grids in [(7 * row, [(100, 37), (100, 0)]), (2 * row, [(1024, 1023), (N, 0), (700, 0)])]:
        with array_plan(m, "hann", combo, chan, 9, stage_bytes=stage) as p:
            for every, first in grids:
                rows = power_sum_rows(N, every, first)
                p.reset()
                check_pairs(p.covariance(x, every, first, bins=band), X, pairs, N, every, first, band, exact_combo(combo), (combo, stage, every, first, "host"))
                p.reset()
                out = torch.zeros((len(pairs), rows, band[1]), dtype=torch.complex64 if fd == np.float32 else torch.complex128, device="cuda")
                got = p.api.sdft_covariance_n(p._p, N, C.c_void_p(x.ctypes.data), every, first, band[0], band[1], C.c_void_p(out.data_ptr()))
                p.synchronize()
                assert got == rows, p.api.last_error()
                check_pairs(out, X, pairs, N, every, first, band, exact_combo(combo), (combo, stage, every, first, "host samples, device sums"))


# ---------------------------------------------------------------------------------------------
# no overrun, no hole, at every alignment of the buffers an element size allows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("combo", ["f32f32", "f32f64"])
def test_covariance_guarded_misaligned_buffers(combo, host):
    """cov carved from a guarded arena at every residue modulo 16 the element size of sdft_fd_t allows, and at 16 mod 128, the samples
    at an odd element; a band of 99 bins (an odd row length: consecutive rows change alignment), windows of 7 samples after a head
    of 3, many of them cut by chunk boundaries; an array with a padded group"""
    td, fd, _ = O.combo_types(combo)
    m, n, every, first, band, chan = 125, 2000, 7, 3, (1, 99), MIXED
    x, X = rows_of(combo, "hann", m, N, None, 9)
    x, X = np.ascontiguousarray(x[:, :n]), X[:, :n]
    pairs = pairs_of(chan)
    rows = power_sum_rows(n, every, first)
    size = np.dtype(fd).itemsize
    tsize = np.dtype(td).itemsize
    places = [(r, 16) for r in range(size, 16, size)] + [(16, 128)]
    with array_plan(m, "hann", combo, chan, 9) as p:
        for r, mod in places:
            arena = (G.HostArena if host else G.DeviceArena)(G.room(((9, n), td), ((len(pairs), rows, 2 * band[1]), fd)))
            xv = G.put(arena.carve((9, n), td, tsize, 16, name="x"), x)
            out = arena.carve((len(pairs), rows, 2 * band[1]), fd, r, mod, name="cov")
            assert G.ptr_of(out) % mod == r
            p.reset()
            p.api.clear()
            got = p.api.sdft_covariance_n(p._p, n, C.c_void_p(G.ptr_of(xv)), every, first, band[0], band[1], C.c_void_p(G.ptr_of(out)))
            p.synchronize()
            assert got == rows, p.api.last_error()
            assert p.get_option("last_kernel") == 9 and p.get_option("last_chunks") > 1
            arena.check()
            assert G.view_unwritten(out) == 0
            assert np.array_equal(G.to_numpy(xv), x)
            s = G.to_numpy(out).reshape(len(pairs), rows, band[1], 2)
            s = np.ascontiguousarray(s).view(X.dtype)[..., 0]
            check_pairs(s, X, pairs, n, every, first, band, exact_combo(combo), (combo, host, r, mod))


# ---------------------------------------------------------------------------------------------
# errors leave the state and the installed lists alone
# ---------------------------------------------------------------------------------------------
def test_covariance_errors():
    combo, m, channels = "f32f32", 64, 5
    x = signals(np.float32, 3000, 5, channels)
    top = C.c_size_t(-1).value
    chan = [3, 0, 4]
    T = 6
    with make(m, "hann", combo, channels=channels) as p:
        api = p.api
        out = np.zeros((T, 12, m), dtype=np.complex64)
        # no array installed
        api.clear()
        assert api.sdft_covariance_n(p._p, 100, x.ctypes.data, 10, 0, 0, m, out.ctypes.data) == -1
        assert "sdft_hip_sdft_covariance_n" in api.last_error() and "array" in api.last_error()
        api.clear()
        with pytest.raises(ValueError):
            p.covariance(x[:, :10])
        p.set_array(chan)
        p.covariance(np.ascontiguousarray(x[:, :300]), 7, 3)       # (errors against a plan that is mid-stream)
        before = p.state()
        # set_array refusals: the list stays
        for lst, count, word in [([0, 1, 5], 3, "channel"), ([top], 1, "channel"), ([1, 2, 1], 3, "twice"), ([0, 0], 2, "twice"),
                                 (None, channels + 1, "too long"), ([0, 1, 2, 3, 4, 0], 6, "too long")]:
            a = None if lst is None else np.array(lst, dtype=np.uint64)
            api.clear()
            assert api.set_array(p._p, count, None if a is None else a.ctypes.data) == -1, (lst, count)
            err = api.last_error()
            assert err and "sdft_hip_set_array" in err and word in err, err
            api.clear()
            assert p.array_channels == len(chan)
        refused = [(100, 0, 0, 0, m, out.ctypes.data, "every"),                 # every == 0
                   (100, 10, 0, 0, 0, out.ctypes.data, "nbins"),                # nbins == 0
                   (100, 10, 0, 1, m, out.ctypes.data, "band"),                 # bin0 + nbins > dftsize
                   (100, 10, 0, m, 1, out.ctypes.data, "band"),
                   (100, 10, 0, 2, top, out.ctypes.data, "band"),               # bin0 + nbins overflows to 1
                   (100, 10, 0, top, 2, out.ctypes.data, "band"),
                   (100, 10, 0, 0, m, None, "NULL"),                            # rows > 0, cov NULL
                   (100, 10, 5000, 0, m, None, "NULL")]                         # first >= n: the head row is a row
        for n, every, first, bin0, nb, ptr, word in refused:
            api.clear()
            assert api.sdft_covariance_n(p._p, n, x.ctypes.data, every, first, bin0, nb, ptr) == -1, (every, bin0, nb)
            err = api.last_error()
            assert err and "sdft_hip_sdft_covariance_n" in err and word in err, err
            api.clear()
            after = p.state()
            assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3], (every, bin0, nb)
            assert p.array_channels == len(chan)
        assert np.count_nonzero(out) == 0
        # n == 0: no rows, nothing moves, cov may be NULL
        assert api.sdft_covariance_n(p._p, 0, x.ctypes.data, 10, 3, 0, m, None) == 0 and api.last_error() is None
        assert p.state()[3] == before[3]
        for bad in ((0, 0), (m, 1), (1, m), (-1, 2)):
            with pytest.raises(ValueError):
                p.covariance(x[:, :10], bins=bad)
        with pytest.raises(ValueError):
            p.covariance(x[:, :10], every=0)
        # the array and the pair list are independent: each leaves the other installed and working
        xs = np.ascontiguousarray(x[:, :100])
        p.set_pairs([3, 3, 0], [3, 0, 4])
        assert p.pairs == 3 and p.array_channels == len(chan)
        with pytest.raises(SdftHipError, match="sdft_hip_set_array"):
            p.set_array([0, 7])
        with pytest.raises(SdftHipError, match="sdft_hip_set_pairs"):
            p.set_pairs([0], [7])
        assert p.pairs == 3 and p.array_channels == len(chan)
        p.reset()
        cov = p.covariance(xs, 10, 0)
        p.reset()
        cs = p.cross_sum(xs, 10, 0)
        assert cov.shape == (T, 10, m) and cs.shape == (3, 10, m)
        assert same_bits(cov[0], cs[0]) and same_bits(cov[1], cs[1]) and same_bits(cov[4], cs[2])     # (3, 3), (3, 0), (0, 4)
        p.set_array(channels)                                  # an int: the channels 0 ... 4
        assert p.array_channels == channels and p.pairs == 3
        p.set_array([])
        assert p.array_channels == 0 and p.pairs == 3
        p.reset()
        assert same_bits(p.cross_sum(xs, 10, 0), cs)
        p.set_array(chan)
        p.set_pairs([], [])
        assert p.pairs == 0 and p.array_channels == len(chan)
        p.reset()
        assert same_bits(p.covariance(xs, 10, 0), cov)


def test_covariance_single_channel_plan():
    combo, m, n, band = "f32f32", 64, 3000, (3, 40)
    x = signal(n, np.float32, 7)
    with make(m, "hann", combo) as p, make(m, "hann", combo) as q:
        p.set_array(1)
        assert p.array_channels == 1
        s = p.covariance(x, 1, 0, bins=band)
        assert s.shape == (1, n, band[1]) and p.get_option("last_kernel") == 9
        assert same_bits(s[0].real.copy(), q.power(x, 1, 0, bins=band)) and same_bits(s[0].imag.copy(), np.zeros((n, band[1]), np.float32))
        assert all(np.array_equal(a, b) for a, b in zip(p.state()[:3], q.state()[:3])) and p.state()[3] == q.state()[3]
        for bad in ([1], [0, 0], [0, 1]):
            with pytest.raises(SdftHipError, match="sdft_hip_set_array"):
                p.set_array(bad)
            assert p.array_channels == 1


# ---------------------------------------------------------------------------------------------
# a plain C host and the C++ facade
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,combo", [([], "f32f64"), (["-DSDFT_FD_FLOAT"], "f32f32")])
def test_c_host_covariance(tmp_path, hip_library, flags, combo):
    """tests/c/host_covariance.c: three channels, the array {2, 0, 1}, one call; its digest of the triangle's bytes is the digest of
    the Python call's result on a plan of the same kind"""
    td = O.combo_types(combo)[0]
    exe = tmp_path / "host_covariance"
    cmd = ["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), *flags,
           os.path.join(ROOT, "tests", "c", "host_covariance.c"), "-o", str(exe), *host_link(hip_library)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m, ch, n, every, first, band = 64, 3, 1500, 100, 37, (3, 20)
    x = np.ascontiguousarray(signals(td, n, 3)[:ch])
    x.tofile(tmp_path / "x.raw")
    r = subprocess.run([str(exe), str(m), str(ch), str(every), str(first), str(band[0]), str(band[1]), str(tmp_path / "x.raw")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "C-HOST-COVARIANCE ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    with array_plan(m, "hann", combo, [2, 0, 1], ch) as p:
        want = p.covariance(x, every, first, bins=band)
        assert p.get_option("last_chunks") > 1
    fields = dict(f.split("=") for f in r.stdout.split() if "=" in f)
    assert int(fields["rows"]) == want.shape[1] and int(fields["digest"], 16) == fnv1a(want.tobytes()), (r.stdout, hex(fnv1a(want.tobytes())))
    mat = covariance_matrix(want, 3)[-1, 0]
    assert float(fields["imagdiag"]) == 0.0 and abs(float(fields["trace"]) - float(np.trace(mat).real)) <= 1e-5 * float(np.trace(mat).real)


def test_cpp_facade_covariance(tmp_path, hip_library):
    """tests/cpp/host_covariance.cpp: sdft::SDFT<T, F>::set_array, array_channels and covariance, compiled once"""
    exe = tmp_path / "host_covariance_cpp"
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-DHOST_T=float", "-DHOST_F=double", "-I", os.path.join(ROOT, "include", "cpp"),
           os.path.join(ROOT, "tests", "cpp", "host_covariance.cpp"), "-o", str(exe), *host_link(hip_library)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m, n = 125, 1441
    signal(n, np.float32, 9).tofile(tmp_path / "x.raw")
    r = subprocess.run([str(exe), str(m), str(tmp_path / "x.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "CPP-COVARIANCE ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
