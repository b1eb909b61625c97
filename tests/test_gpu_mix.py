"""Channel-mix analysis (sdft_hip_set_mix, sdft_hip_sdft_mix_n, SDFT.mix) on a real MI355X against the oracle.

The reference is the header's expression evaluated with numpy on the oracle's rows, from separate real and imaginary arrays in
the FD dtype (numpy's complex product may fuse; four ufunc calls and two more do not):
    re = wr*yr - wi*yi        im = wr*yi + wi*yr
summed from -0 in ascending element order, each component by itself.  Bars: equal bits wherever sdft_sdft_n is bit-identical to
the reference (FD float, FD double with carry = 1, calls shorter than 512 samples); with FD double's default carries the header's
bar, promise (4): per component sum_i (|wr_i| + |wi_i|) 1e-11 max|X_chan[i]| over the call, plus gamma_(nch + 1) times
sum_i (|wr_i| + |wi_i|) (|yr_i| + |yi_i|) for the roundings.

Signals, the oracle's rows and the state check are those of tests/test_gpu_cross_sum.py; plans have 9 channels at m in
{5, 64, 125} and 5 at m in {1000, 1024}.  The mixes' channel lists are one below, at and one above every group size the kernel
is built for (2, 4, 8), in plan order and permuted, and subsets that leave channels to advance-only items; nout in {1, 2, 3, 5}
is one below, at and above the block sizes (1, 2, 4).  n = 6000: several chunks and a roll-over of the cursor at 2 x dftsize."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import guarded as G
from oracle import oracle as O
from sdft_amd.sdft import SdftHipError, covariance_matrix, every_next_first, every_rows, mvdr_weights
from sdft_amd.signals import noise
from test_gpu_cross_sum import check_state, host_link, rows_of, same_bits, signals
from test_gpu_power import bands_of, exact_combo, make, to_dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 6000
E_ROW = 1e-11                                                # the row deviation sdft_hip_sdft_every_n documents
GRIDS = [(1, 0), (1, 3), (7, 6), (100, 37), (1024, 1023)]
NOUTS = [1, 2, 3, 5]
ARRAYS9 = [[0], [0, 1], [2, 0, 1], [0, 1, 2, 3], [4, 0, 5, 2, 1], [6, 5, 4, 3, 2, 1, 0], list(range(8)), list(range(9)), [8, 3]]
ARRAYS5 = [list(range(5)), [3, 1], [4, 2, 0, 1]]
MIXED = [4, 0, 5, 2, 1]                                      # the channels 3, 6, 7, 8 only advance
GROUPS, BLOCKS = (2, 4, 8), (1, 2, 4)


def numpy_of(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def shape_of(m):
    return (9, ARRAYS9) if m < 1000 else (5, ARRAYS5)


def two_bands(m, p):
    """one across the first tile boundaries with an odd start, one inside the last tile"""
    bs = bands_of(m, p)
    return list(dict.fromkeys([(50, 100) if (50, 100) in bs else bs[3] if len(bs) > 3 else bs[0], bs[-1]]))


def weights_for(fdx, nout, nch, m, seed):
    """random complex weights; every seventh bin of element 0 is zero, the last element of output 0 is all zeros where there are
    two or more elements and outputs, and element 1 (where there is one) is a negative real column"""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((nout, nch, m)) + 1j * rng.standard_normal((nout, nch, m))).astype(fdx)
    w[:, 0, ::7] = 0
    if nch > 1:
        w[:, 1] = -np.abs(w[:, 1].real) - 0.25
        if nout > 1:
            w[0, nch - 1] = 0
    return w


def mix_ref(X, chan, w, every, first, band):
    """(re, im, bar_w, bar_r) of shape (nout, rows, nb): the header's expression on the rows X (channels, n, m), and the two sums
    the bar is made of: sum_i (|wr| + |wi|) max|X_chan[i]| and sum_i (|wr| + |wi|) (|yr| + |yi|)"""
    fd = X.real.dtype
    lo, nb = band
    rows = X[0, first::every].shape[0]
    nout = w.shape[0]
    re = np.full((nout, rows, nb), -0.0, dtype=fd)
    im = np.full((nout, rows, nb), -0.0, dtype=fd)
    bar_w = np.zeros((nout, 1, nb))
    bar_r = np.zeros((nout, rows, nb))
    for i, c in enumerate(chan):
        y = X[c, first::every, lo:lo + nb]
        yr, yi = np.ascontiguousarray(y.real), np.ascontiguousarray(y.imag)
        top = float(np.abs(X[c]).max()) if rows else 0.0
        for o in range(nout):
            wr = np.ascontiguousarray(w[o, i, lo:lo + nb].real)[None]
            wi = np.ascontiguousarray(w[o, i, lo:lo + nb].imag)[None]
            assert wr.dtype == fd and yr.dtype == fd
            rr, ii, ri, ir = wr * yr, wi * yi, wr * yi, wi * yr
            re[o] = re[o] + (rr - ii)
            im[o] = im[o] + (ri + ir)
            aw = np.abs(wr).astype(np.float64) + np.abs(wi)
            bar_w[o] += aw * top
            bar_r[o] += aw * (np.abs(yr).astype(np.float64) + np.abs(yi))
    return re, im, bar_w, bar_r


def check_mix(got, X, chan, w, every, first, band, exact, what, scale=1.0):
    """scale: what the row deviation E_ROW is multiplied by on a route whose rows are held to another bar"""
    got = numpy_of(got)
    re, im, bar_w, bar_r = mix_ref(X, chan, w, every, first, band)
    assert got.shape == re.shape and got.dtype == X.dtype, (what, got.shape, re.shape, got.dtype)
    if got.size == 0:
        return
    gr, gi = np.ascontiguousarray(got.real), np.ascontiguousarray(got.imag)
    if exact:
        assert same_bits(gr, re) and same_bits(gi, im), (what, float(np.abs(gr - re).max()), float(np.abs(gi - im).max()))
        return
    u = float(np.finfo(X.real.dtype).eps) / 2
    k = len(chan) + 1
    bar = E_ROW * scale * bar_w + (k * u / (1 - k * u)) * bar_r
    worst = max(float((np.abs(gr.astype(np.float64) - re) - bar).max()), float((np.abs(gi.astype(np.float64) - im) - bar).max()))
    print(what, "largest deviation over its bar:", float(np.maximum(np.abs(gr - re), np.abs(gi - im)).max()), "/", float(bar.min()))
    assert worst <= 0, (what, worst)


def mix_plan(m, window, combo, w, chan, channels, **opts):
    p = make(m, window, combo, channels=channels, **opts)
    p.set_mix(w, chan)
    assert p.mix_outputs == w.shape[0]
    return p


# ---------------------------------------------------------------------------------------------
# parity: every type pair x window x dftsize, the channel lists, output counts, grids and bands in turn
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [5, 64, 125, 1000, 1024])
@pytest.mark.parametrize("window", ["hann", "blackman"])
@pytest.mark.parametrize("combo", O.COMBOS)
def test_mix_parity(combo, window, m):
    channels, arrays = shape_of(m)
    x, X = rows_of(combo, window, m, N, None, channels)
    dx = to_dev(x)
    exact = exact_combo(combo)
    with make(m, window, combo, channels=channels) as p:
        bands = two_bands(m, p)
        call = 0
        for ai, chan in enumerate(arrays):
            nout = NOUTS[ai % len(NOUTS)]
            w = weights_for(p.fdx, nout, len(chan), m, 100 * m + ai)
            p.set_mix(w, chan)
            assert p.mix_outputs == nout
            for gi, (every, first) in enumerate(GRIDS):
                band = bands[(ai + gi) % len(bands)]
                call += 1
                p.reset()
                got = p.mix(dx if call % 2 else x, every, first, bins=band)
                assert p.get_option("last_kernel") == 10 and p.get_option("last_chunks") > 1
                check_mix(got, X, chan, w, every, first, band, exact, (combo, window, m, chan, nout, every, first, band))


@pytest.mark.parametrize("combo,opts,n", [("f32f64", dict(carry=1), N), ("f64f64", dict(carry=1), N), ("f32f64", {}, 500), ("f64f64", {}, 500),
                                          ("f32f32", {}, 500)], ids=str)
def test_mix_exact_routes(combo, opts, n):
    """FD double with the exact carries, and calls of one chunk (shorter than 512 samples): equal bits"""
    m, chan = 125, MIXED
    x, X = rows_of(combo, "hann", m, N, None, 9)
    x, X = np.ascontiguousarray(x[:, :n]), X[:, :n]
    w = weights_for(np.complex64 if combo.endswith("f32") else np.complex128, 3, len(chan), m, 5)
    with mix_plan(m, "hann", combo, w, chan, 9, **opts) as p:
        for band in two_bands(m, p):
            for i, (every, first) in enumerate(GRIDS):
                p.reset()
                got = p.mix(to_dev(x) if i % 2 else x, every, first, bins=band)
                assert p.get_option("last_kernel") == 10 and (p.get_option("last_chunks") > 1) == (n == N)
                check_mix(got, X, chan, w, every, first, band, True, (combo, opts, n, every, first, band))


@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("window", ["hann", "blackman"])
@pytest.mark.parametrize("combo", O.COMBOS)
def test_mix_tiny_sizes(combo, window, m):
    """m = 1: every halo cell is zero for ever; m = 2, 3: the halo reflects into the owned bins.  One chunk: exact bits"""
    n = 500
    x, X = rows_of(combo, window, m, n, None, 9)
    fdx = np.complex64 if combo.endswith("f32") else np.complex128
    for ai, chan in enumerate([[0], MIXED, list(range(9))]):
        w = weights_for(fdx, NOUTS[ai + 1], len(chan), m, 7 + ai)
        with mix_plan(m, window, combo, w, chan, 9) as p:
            for every, first in [(1, 0), (7, 6), (100, 37)]:
                for band in [(0, m), (m - 1, 1)]:
                    p.reset()
                    got = p.mix(x, every, first, bins=band)
                    assert p.get_option("last_kernel") == 10
                    check_mix(got, X, chan, w, every, first, band, True, (combo, window, m, chan, every, first, band))


@pytest.mark.parametrize("combo", O.COMBOS)
def test_mix_one_hot_is_every(combo):
    """weight 1 for one element, 0 for the others: the channel's rows of sdft_every(), as numbers"""
    m, chan = 125, MIXED
    td = O.combo_types(combo)[0]
    x = signals(td, N, m, 9)
    fdx = np.complex64 if combo.endswith("f32") else np.complex128
    w = np.zeros((len(chan), len(chan), m), dtype=fdx)
    for o in range(len(chan)):
        w[o, o] = 1
    for opts in ([{}] if exact_combo(combo) else [dict(chunk=1024), dict(carry=1)]):
        with mix_plan(m, "hann", combo, w, chan, 9, **opts) as p, make(m, "hann", combo, channels=9, **opts) as q:
            for every, first in [(1, 3), (100, 37)]:
                p.reset(); q.reset()
                got = p.mix(x, every, first)
                want = q.sdft_every(x, every, first)
                assert np.isfinite(want).all()
                for o, c in enumerate(chan):
                    assert np.array_equal(got[o], want[c]), (combo, opts, every, first, o, c)


# ---------------------------------------------------------------------------------------------
# the group and the block size are a matter of speed alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_mix_groups_and_blocks_give_the_same_bits(combo):
    """all nine (G, O) candidates of the hooks build (options "mix_group", "mix_block") return the bits of the product's choice; FD
    double runs at a fixed chunk length, so that every plan starts from the same carries"""
    m = 125
    td = O.combo_types(combo)[0]
    x = to_dev(signals(td, N, m, 9))
    fdx = np.complex64 if combo.endswith("f32") else np.complex128
    opts = {} if exact_combo(combo) else dict(chunk=1024)
    band = (1, 99)
    for ai, chan in enumerate(ARRAYS9):
        nout = NOUTS[ai % len(NOUTS)] if ai else 5
        w = weights_for(fdx, nout, len(chan), m, ai)
        with mix_plan(m, "hann", combo, w, chan, 9, **opts) as p:
            want = numpy_of(p.mix(x, 7, 6, bins=band))
            product = (p.get_option("mix_group"), p.get_option("mix_block"))
            assert product[0] in GROUPS and product[1] in BLOCKS
            for g in GROUPS:
                for o in BLOCKS:
                    p.set_option("mix_group", g)
                    p.set_option("mix_block", o)
                    assert (p.get_option("mix_group"), p.get_option("mix_block")) == (g, o) and p.mix_outputs == nout
                    p.reset()
                    got = numpy_of(p.mix(x, 7, 6, bins=band))
                    assert p.get_option("last_kernel") == 10 and p.get_option("last_chunks") > 1
                    assert same_bits(got, want), (combo, chan, nout, g, o)


# ---------------------------------------------------------------------------------------------
# state, streaming, determinism
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS)
def test_mix_leaves_the_state_of_sdft(combo):
    """after the call the state of all nine channels is the one sdft of the same samples leaves on a twin plan: with channels outside
    the mix, with a band that leaves tiles silent, with no row at all (out = None), and followed by sdft, isdft and covariance"""
    td = O.combo_types(combo)[0]
    fdx = np.complex64 if combo.endswith("f32") else np.complex128
    m = 125
    x = signals(td, N, m, 9)
    hop = np.stack([noise(100, seed=12 + c, dtype=td) for c in range(9)])
    eps = float(np.finfo(td).eps)
    k = 0
    for opts in ([{}, dict(carry=1)] if not exact_combo(combo) else [{}]):
        exact = exact_combo(combo) or "carry" in opts
        cases = [(MIXED, 3, (100, 37), (10, 100)),           # channels outside the mix
                 (list(range(9)), 5, (7, 6), (m - 2, 2)),    # a band inside the last tile: the other tiles only advance
                 ([8, 3], 1, (100, N + 5), (0, m)),          # first >= n: no row
                 (MIXED, 2, (1024, 1023), (1, 99))]          # followed by other calls
        for ci, (chan, nout, (every, first), band) in enumerate(cases):
            k += 1
            w = weights_for(fdx, nout, len(chan), m, ci)
            with mix_plan(m, "hann", combo, w, chan, 9, **opts) as p, make(m, "hann", combo, channels=9, **opts) as q:
                if ci == 2:
                    p.api.clear()
                    assert p.api.sdft_mix_n(p._p, N, C.c_void_p(x.ctypes.data), every, first, band[0], band[1], None) == 0 and p.api.last_error() is None
                else:
                    p.mix(to_dev(x) if k % 2 else x, every, first, bins=band)
                assert p.get_option("last_kernel") == 10 and p.get_option("last_chunks") > 1
                q.sdft(x)
                check_state(p, q, exact, (combo, opts, chan, every, first, band))
                if ci != 3:
                    continue
                dp, dq = p.sdft(hop), q.sdft(hop)
                yp, yq = p.isdft(dp), q.isdft(dq)
                p.set_array(chan); q.set_array(chan)
                cp, cq = p.covariance(hop, 10, 0), q.covariance(hop, 10, 0)
                if exact:
                    assert np.array_equal(dp, dq) and np.array_equal(yp, yq) and np.array_equal(cp, cq)
                else:
                    rel = lambda a, b: float(np.abs(a - b).max()) / float(np.abs(b).max())
                    assert rel(dp, dq) <= 1e-10 and rel(cp, cq) <= 1e-9, (rel(dp, dq), rel(cp, cq))
                    assert float(np.abs(yp - yq).max()) <= 1e-10 * float(np.abs(dq).max()) + 2 * eps * float(np.abs(yq).max())


@pytest.mark.parametrize("combo", ["f32f32", "f64f32", "f32f64"])
@pytest.mark.parametrize("every,first0", [(1, 0), (7, 6), (100, 37)])
def test_mix_streaming(combo, every, first0):
    """n cut into calls of 37, 500, 1 and the rest on one grid (every_next_first): the rows of the one call, bit for bit on the exact
    routes (FD double: carry = 1)"""
    m, band, chan = 125, (10, 100), MIXED
    opts = {} if exact_combo(combo) else dict(carry=1)
    x, X = rows_of(combo, "hann", m, N, None, 9)
    fdx = np.complex64 if combo.endswith("f32") else np.complex128
    w = weights_for(fdx, 3, len(chan), m, 3)
    with mix_plan(m, "hann", combo, w, chan, 9, **opts) as p:
        whole = numpy_of(p.mix(x, every, first0, bins=band))
        p.reset()
        parts, t, first = [], 0, first0
        for i, k in enumerate([37, 500, 1, N - 538]):
            xs = np.ascontiguousarray(x[:, t:t + k])
            d = numpy_of(p.mix(to_dev(xs) if i % 2 else xs, every, first, bins=band))
            assert d.shape == (3, every_rows(k, every, first), band[1]) and p.get_option("last_kernel") == 10
            parts.append(d)
            first = every_next_first(k, every, first)
            t += k
        got = np.concatenate(parts, axis=1)
        assert same_bits(got, whole), (combo, every, first0)
        check_mix(got, X, chan, w, every, first0, band, True, (combo, every, first0, "streamed"))


def test_mix_replaced_and_removed_between_calls():
    """a new mix takes effect with the next call, the stream goes on; a call with the mix removed returns -1 and moves nothing"""
    combo, m, band = "f32f32", 64, (3, 40)
    x, X = rows_of(combo, "hann", m, N, None, 9)
    w1 = weights_for(np.complex64, 2, 3, m, 1)
    w2 = weights_for(np.complex64, 5, 4, m, 2)
    with mix_plan(m, "hann", combo, w1, [2, 0, 1], 9) as p:
        a = p.mix(np.ascontiguousarray(x[:, :1000]), 7, 6, bins=band)
        check_mix(a, X[:, :1000], [2, 0, 1], w1, 7, 6, band, True, "first mix")
        f = every_next_first(1000, 7, 6)
        p.set_mix(w2, [8, 7, 0, 3])
        assert p.mix_outputs == 5
        b = p.mix(np.ascontiguousarray(x[:, 1000:3000]), 7, f, bins=band)
        check_mix(b, X[:, 1000:3000], [8, 7, 0, 3], w2, 7, f, band, True, "second mix")
        f = every_next_first(2000, 7, f)
        p.set_mix(None)
        assert p.mix_outputs == 0
        before = p.state()
        out = np.zeros((5, 500, band[1]), dtype=np.complex64)
        xs = np.ascontiguousarray(x[:, 3000:])
        p.api.clear()
        assert p.api.sdft_mix_n(p._p, 3000, C.c_void_p(xs.ctypes.data), 7, f, band[0], band[1], C.c_void_p(out.ctypes.data)) == -1
        assert "sdft_hip_sdft_mix_n" in p.api.last_error() and "mix" in p.api.last_error()
        p.api.clear()
        after = p.state()
        assert all(np.array_equal(u, v) for u, v in zip(before[:3], after[:3])) and before[3] == after[3] and np.count_nonzero(out) == 0
        p.set_mix(w1[0], [2, 0, 1])                          # (nch, dftsize): one output
        c = p.mix(xs, 7, f, bins=band)
        check_mix(c, X[:, 3000:], [2, 0, 1], w1[:1], 7, f, band, True, "third mix")


@pytest.mark.parametrize("combo", ["f32f64", "f64f32"])
def test_mix_same_bits_on_every_run(combo):
    m = 1000
    x = signals(O.combo_types(combo)[0], N, m, 5)
    fdx = np.complex64 if combo.endswith("f32") else np.complex128
    w = weights_for(fdx, 5, 5, m, 9)
    for device in (False, True):
        xs = to_dev(x) if device else x
        with mix_plan(m, "hann", combo, w, None, 5) as p:
            runs = []
            for _ in range(3):
                p.reset()
                runs.append(numpy_of(p.mix(xs, 7, 6, bins=(1, 998))))
                assert p.get_option("last_chunks") > 1
            assert same_bits(runs[0], runs[1]) and same_bits(runs[0], runs[2]), (combo, device)


# ---------------------------------------------------------------------------------------------
# pointers: host and device, misaligned, guarded; host memory in segments
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host_x", [False, True])
@pytest.mark.parametrize("host_out", [False, True])
@pytest.mark.parametrize("combo", ["f32f32", "f32f64"])
def test_mix_guarded_buffers(combo, host_x, host_out):
    """out carved from a guarded arena at 16-byte alignment and one sdft_fd_t off it, the samples at an odd element; a band of 99 bins
    (an odd row length: consecutive rows change alignment); a mix with a padded group and a short last block"""
    td, fd, _ = O.combo_types(combo)
    m, n, every, first, band, chan, nout = 125, 2000, 7, 3, (1, 99), MIXED, 5
    x, X = rows_of(combo, "hann", m, N, None, 9)
    x, X = np.ascontiguousarray(x[:, :n]), X[:, :n]
    w = weights_for(X.dtype, nout, len(chan), m, 11)
    rows = every_rows(n, every, first)
    size, tsize = np.dtype(fd).itemsize, np.dtype(td).itemsize
    with mix_plan(m, "hann", combo, w, chan, 9) as p:
        for r, mod in [(0, 16), (size, 16)]:
            ax = (G.HostArena if host_x else G.DeviceArena)(G.room(((9, n), td)))
            ao = (G.HostArena if host_out else G.DeviceArena)(G.room(((nout, rows, 2 * band[1]), fd)))
            xv = G.put(ax.carve((9, n), td, tsize, 16, name="x"), x)
            out = ao.carve((nout, rows, 2 * band[1]), fd, r, mod, name="out")
            assert G.ptr_of(out) % mod == r
            p.reset()
            p.api.clear()
            got = p.api.sdft_mix_n(p._p, n, C.c_void_p(G.ptr_of(xv)), every, first, band[0], band[1], C.c_void_p(G.ptr_of(out)))
            p.synchronize()
            assert got == rows, p.api.last_error()
            assert p.get_option("last_kernel") == 10 and p.get_option("last_chunks") > 1
            ax.check(); ao.check()
            assert G.view_unwritten(out) == 0
            assert np.array_equal(G.to_numpy(xv), x)
            s = np.ascontiguousarray(G.to_numpy(out).reshape(nout, rows, band[1], 2)).view(X.dtype)[..., 0]
            check_mix(s, X, chan, w, every, first, band, exact_combo(combo), (combo, host_x, host_out, r, mod))


@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_mix_host_staging_in_segments(combo):
    """stage_bytes small enough for several segments: host samples with host and with device rows"""
    import torch
    fd = O.combo_types(combo)[1]
    m, band, chan, nout = 125, (10, 100), [2, 0, 1, 7, 5], 3
    x, X = rows_of(combo, "hann", m, N, None, 9)
    w = weights_for(X.dtype, nout, len(chan), m, 13)
    row = nout * 2 * band[1] * np.dtype(fd).itemsize
    for stage, grids in [(7 * row, [(100, 37), (1, 0)]), (2 * row, [(1024, 1023), (7, 6)])]:
        with mix_plan(m, "hann", combo, w, chan, 9, stage_bytes=stage) as p:
            for every, first in grids:
                rows = every_rows(N, every, first)
                p.reset()
                check_mix(p.mix(x, every, first, bins=band), X, chan, w, every, first, band, exact_combo(combo), (combo, stage, every, first, "host"))
                p.reset()
                out = torch.zeros((nout, rows, band[1]), dtype=torch.complex64 if fd == np.float32 else torch.complex128, device="cuda")
                got = p.api.sdft_mix_n(p._p, N, C.c_void_p(x.ctypes.data), every, first, band[0], band[1], C.c_void_p(out.data_ptr()))
                p.synchronize()
                assert got == rows, p.api.last_error()
                check_mix(out, X, chan, w, every, first, band, exact_combo(combo), (combo, stage, every, first, "host samples, device rows"))


# ---------------------------------------------------------------------------------------------
# errors leave the state and the installed mix alone
# ---------------------------------------------------------------------------------------------
def test_mix_errors():
    combo, m, channels = "f32f32", 64, 5
    x = signals(np.float32, 3000, 5, channels)
    top = C.c_size_t(-1).value
    chan = [3, 0, 4]
    w = weights_for(np.complex64, 2, 3, m, 1)
    with make(m, "hann", combo, channels=channels) as p:
        api = p.api
        out = np.zeros((2, 12, m), dtype=np.complex64)
        api.clear()
        assert api.sdft_mix_n(p._p, 100, x.ctypes.data, 10, 0, 0, m, out.ctypes.data) == -1
        assert "sdft_hip_sdft_mix_n" in api.last_error() and "mix" in api.last_error()
        api.clear()
        with pytest.raises(ValueError):
            p.mix(x[:, :10])
        p.set_mix(w, chan)
        first_rows = p.mix(np.ascontiguousarray(x[:, :300]), 7, 3)      # (errors against a plan that is mid-stream)
        before = p.state()
        wide = np.zeros((2, 6, m), dtype=np.complex64)
        for lst, nout, count, wts, word in [([0, 1, 5], 2, 3, wide, "channel"), ([top], 2, 1, wide, "channel"), ([1, 2, 1], 2, 3, wide, "twice"),
                                            (None, 2, channels + 1, wide, "too long"), ([0, 1, 2, 3, 4, 0], 2, 6, wide, "too long"),
                                            ([0, 1], 2, 2, None, "NULL"), (None, 2, 0, wide, "at least one channel"), (None, 70000, 1, wide, "outputs")]:
            a = None if lst is None else np.array(lst, dtype=np.uint64)
            api.clear()
            assert api.set_mix(p._p, nout, count, None if a is None else a.ctypes.data, None if wts is None else wts.ctypes.data) == -1, (lst, count)
            err = api.last_error()
            assert err and "sdft_hip_set_mix" in err and word in err, err
            api.clear()
            assert p.mix_outputs == 2
        refused = [(100, 0, 0, 0, m, out.ctypes.data, "every"), (100, 10, 0, 0, 0, out.ctypes.data, "nbins"),
                   (100, 10, 0, 1, m, out.ctypes.data, "band"), (100, 10, 0, m, 1, out.ctypes.data, "band"),
                   (100, 10, 0, 2, top, out.ctypes.data, "band"), (100, 10, 0, top, 2, out.ctypes.data, "band"),
                   (100, 10, 0, 0, m, None, "NULL")]
        for n, every, first, bin0, nb, ptr, word in refused:
            api.clear()
            assert api.sdft_mix_n(p._p, n, x.ctypes.data, every, first, bin0, nb, ptr) == -1, (every, bin0, nb)
            err = api.last_error()
            assert err and "sdft_hip_sdft_mix_n" in err and word in err, err
            api.clear()
            after = p.state()
            assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3], (every, bin0, nb)
            assert p.mix_outputs == 2
        assert np.count_nonzero(out) == 0
        assert api.sdft_mix_n(p._p, 0, x.ctypes.data, 10, 3, 0, m, None) == 0 and api.last_error() is None
        assert api.sdft_mix_n(p._p, 100, x.ctypes.data, 10, 100, 0, m, None) == 0 and api.last_error() is None      # no row: out may be NULL
        for bad in ((0, 0), (m, 1), (1, m), (-1, 2)):
            with pytest.raises(ValueError):
                p.mix(x[:, :10], bins=bad)
        with pytest.raises(ValueError):
            p.mix(x[:, :10], every=0)
        with pytest.raises(ValueError):
            p.set_mix(np.zeros((2, 3, m + 1), dtype=np.complex64))
        with pytest.raises(ValueError):
            p.set_mix(w, [0, 1])
        with pytest.raises(SdftHipError, match="sdft_hip_set_mix"):
            p.set_mix(w, [0, 7, 1])
        # the refused mixes left the first one installed and working; pair list, array and mix are independent
        p.set_pairs([3], [0])
        p.set_array([0, 1])
        assert p.mix_outputs == 2 and p.pairs == 1 and p.array_channels == 2
        p.reset()
        assert same_bits(p.mix(np.ascontiguousarray(x[:, :300]), 7, 3), first_rows)
        p.set_mix(None)
        assert p.mix_outputs == 0 and p.pairs == 1 and p.array_channels == 2


# ---------------------------------------------------------------------------------------------
# the chain the call closes: covariance -> mvdr_weights -> mix
# ---------------------------------------------------------------------------------------------
def test_mix_mvdr_chain():
    """a plane wave in noise on four channels: the MVDR mix of the covariance call's matrix keeps w^H d = 1 per bin and returns
    the einsum of its own weights with the rows of sdft()"""
    combo, m, channels, n = "f32f64", 64, 4, 3000
    x = signals(np.float32, n, 3, channels)
    with make(m, "hann", combo, channels=channels, carry=1) as p, make(m, "hann", combo, channels=channels, carry=1) as q:
        p.set_array(channels)
        mat = covariance_matrix(p.covariance(x, n, 0), channels)
        d = np.exp(-2j * np.pi * np.outer(np.arange(m), np.arange(channels)) / 16)
        w = mvdr_weights(mat, d, loading=1e-3)
        assert w.shape == (1, channels, m)
        assert np.abs(np.einsum("ck,kc->k", w[0], d) - 1).max() <= 1e-12
        p.reset()
        p.set_mix(w)
        y = p.mix(x, 1, 0)
        rows = q.sdft(x)
        want = np.einsum("ck,ctk->tk", w[0], rows)
        assert float(np.abs(y[0] - want).max()) <= 1e-12 * float(np.abs(rows).max()) * float(np.abs(w).sum(axis=1).max())


# ---------------------------------------------------------------------------------------------
# a plain C host and the C++ facade
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,combo", [([], "f32f64"), (["-DSDFT_FD_FLOAT"], "f32f32")])
def test_c_host_mix(tmp_path, hip_library, flags, combo):
    """tests/c/host_mix.c: three channels, the mix {2, 0, 1} with two outputs whose weights it reads from a file, one call; it prints
    the rows it got, which are the Python call's on a plan of the same kind"""
    td = O.combo_types(combo)[0]
    fdx = np.complex64 if combo.endswith("f32") else np.complex128
    exe = tmp_path / "host_mix"
    cmd = ["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), *flags,
           os.path.join(ROOT, "tests", "c", "host_mix.c"), "-o", str(exe), *host_link(hip_library)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m, ch, n, every, first, band, nout = 64, 3, 1500, 100, 37, (3, 20), 2
    x = np.ascontiguousarray(signals(td, n, 3)[:ch])
    w = weights_for(fdx, nout, 3, m, 21)
    x.tofile(tmp_path / "x.raw")
    w.tofile(tmp_path / "w.raw")
    r = subprocess.run([str(exe), str(m), str(ch), str(every), str(first), str(band[0]), str(band[1]), str(tmp_path / "x.raw"), str(tmp_path / "w.raw"),
                        str(tmp_path / "y.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "C-HOST-MIX ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    with mix_plan(m, "hann", combo, w, [2, 0, 1], ch) as p:
        want = p.mix(x, every, first, bins=band)
        assert p.get_option("last_chunks") > 1
    got = np.fromfile(tmp_path / "y.raw", dtype=fdx).reshape(want.shape)
    assert same_bits(got, want)


def test_cpp_facade_mix(tmp_path, hip_library):
    """tests/cpp/host_mix.cpp: sdft::SDFT<T, F>::set_mix, mix_outputs and mix, compiled once; the one-channel plan's mix with weight
    (0, 1) is i times the rows of sdft_every()"""
    exe = tmp_path / "host_mix_cpp"
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-DHOST_T=float", "-DHOST_F=double", "-I", os.path.join(ROOT, "include", "cpp"),
           os.path.join(ROOT, "tests", "cpp", "host_mix.cpp"), "-o", str(exe), *host_link(hip_library)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m, n = 125, 1441
    from test_gpu_power import signal
    signal(n, np.float32, 9).tofile(tmp_path / "x.raw")
    r = subprocess.run([str(exe), str(m), str(tmp_path / "x.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "CPP-MIX ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
