"""The exact model (tests/exact_sdft.py) against the oracle, and the checker's sensitivity, on the CPU.

1. The model is the truth the inexact GPU routes are held to, so it is checked here first: against the oracle (port and, where
   it is built, the genuine reference) for every type pair, window, latency 1 / 0.5 / 0.3 and N from 1 to 1000, on streams that
   start from zero, cross several wraps and arrive in calls of uneven length; and a handful of bins against 40-digit mpmath.
   The reference must satisfy E[k] <= C B per bin (B the serial bound) and per sample |y - y_exact| <= C F_y(t).
2. Sensitivity: seeded mutations of the oracle's outputs that the old bars (max|a-b| / max|b| <= 1e-11 on rows, 1e-6 on the
   fused call's y at FD double) accept.  For each, the old figure is measured here and must pass, and the new check must fail.
"""

import math

import numpy as np
import pytest

import exact_sdft as X
from oracle import oracle as O
from sdft_amd.signals import noise, sine_sweep


def backends(combo):
    out = [("port", O.Port)]
    if O.have_reference(combo):
        out.append(("reference", O.Reference))
    return out


def rel_err(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return float(np.abs(a - b).max()) / float(np.abs(b).max())


def uneven_calls(ref, x):
    """The oracle over x in calls of uneven length (1, 2N-1, 7, the rest in thirds)."""
    cuts = sorted({0, 1, min(x.size, 1 + 2 * ref.dftsize - 1), min(x.size, 2 * ref.dftsize + 7), x.size // 3, 2 * x.size // 3, x.size})
    return np.concatenate([ref.sdft(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:]) if b > a])


@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 7, 64, 100, 1000])
def test_model_against_the_oracle(combo, N):
    td, fd, fdx = O.combo_types(combo)
    n = max(7 * N + 13, 2500)                                   # several wraps of the 2N-sample period
    x = (sine_sweep(n, dtype=td) * td(0.7) + noise(n, seed=N, dtype=td) * td(0.3)).astype(td)
    st = X.Stream(x, N, combo)
    rows = X.sample_rows(n, extra=range(0, min(n, 2 * N + 3)), count=48, seed=N)     # all start-up rows t < 2N
    A = st.A(rows)
    F = X.serial_bound(combo, N, A, L=n)
    for window in ("boxcar", "hann", "hamming", "blackman"):
        Zx = st.rows(rows, window)
        for kind, cls in backends(combo):
            for latency in (1.0, 0.5, 0.3):
                ref = cls(N, window, latency, combo)
                d = uneven_calls(ref, x)
                if latency == 1.0:
                    X.check_bins(X.bin_errors(d[rows], Zx), np.zeros(N), F, what=(kind, combo, N, window))
                y = ref.isdft(d[rows])
                yx, S = X.exact_synthesis(Zx, N, latency)
                Fy = X.pipeline_floor(combo, combo, N, latency, S, F)
                X.check_pipeline(y, yx, yx, Fy, what=(kind, combo, N, window, latency))
                if window == "hann":
                    # the state: acc after the last sample
                    acc = ref.state()[0]
                    assert np.abs(acc - st.acc(n - 1)).max() <= 4 * F * 2 * N, (kind, combo, N)


@pytest.mark.parametrize("combo", O.COMBOS)
@pytest.mark.parametrize("latency", [1.0, 0.5, 0.3])
def test_exact_synthesis_of_rounded_rows(combo, latency):
    """The oracle's synthesis of exact rows rounded to FD against the exact sum of those same rows: the in-order sum of N terms
    errs by at most (N - 1) eps_FD of sum|terms| (recursive summation, Higham 4.2), the products and the table 2 eps_FD more,
    the rounding to TD eps_TD: r(t) <= eps_TD + eps_FD (N + 2), a rigorous bound.  A wrong synthesis convention is O(1) off."""
    td, fd, fdx = O.combo_types(combo)
    for N, window in ((1, "hann"), (5, "blackman"), (64, "boxcar"), (1000, "hamming")):
        x = noise(3 * N + 500, seed=N + 1, dtype=td)
        rows = X.sample_rows(x.size, count=64, seed=2)
        Zr = X.exact_rows(x, N, window, rows, combo).astype(fdx)
        yx, S = X.exact_synthesis(Zr, N, latency)
        for kind, cls in backends(combo):
            y = cls(N, window, latency, combo).isdft(Zr)
            r = X.sample_errors(y, yx, S)
            assert r.max() <= X.EPS[combo[:3]] + X.EPS[combo[3:]] * (N + 2), (kind, combo, N, latency, r.max())


def test_model_against_mpmath():
    """A handful of bins at 40 digits straight from the definition X_t[k] = sum_{s<=t} delta_s e^{i pi k (t+1-s)/N} with the
    reference's rounded differences: the model's own error is far below the eps_FD * A scale it judges (< 1e-3 of it)."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    for combo, N, window in (("f32f64", 7, "blackman"), ("f64f64", 5, "hann"), ("f32f32", 64, "hamming"), ("f64f64", 2, "blackman")):
        td = O.combo_types(combo)[0]
        x = noise(6 * N + 41, seed=3, dtype=td)
        n = x.size
        old = np.zeros_like(x)
        old[2 * N:] = x[:-2 * N]
        delta = (x - old).astype(np.float64)                    # TD arithmetic, as the reference rounds it
        st = X.Stream(x, N, combo)
        t = n - 1
        taps = X.TAPS[window]

        def Xbin(k):
            flip = False
            if N == 1 and k != 0:
                return mp.mpc(0)
            while k < 0 or k > N - 1:
                k = -k if k < 0 else 2 * (N - 1) - k
                flip = not flip
            v = mp.fsum(mp.mpf(float(delta[s])) * mp.expjpi(mp.mpf(k * (t + 1 - s)) / N) for s in range(t + 1))
            return mp.conj(v) if flip else v

        Z = st.rows([t], window)[0]
        A = st.A([t])
        for k in sorted({0, 1, N // 2, N - 1}):
            z = mp.fsum(mp.mpf(taps[abs(j)]) * Xbin(k + j) for j in range(-(len(taps) - 1), len(taps))) / (2 * N)
            err = abs(mp.mpc(mp.mpf(str(Z[k].real)), mp.mpf(str(Z[k].imag))) - z)      # (str keeps every digit of the longdouble)
            assert float(err) <= 1e-3 * X.EPS["f64"] * A, (combo, N, k, float(err), A)


# ---------------------------------------------------------------------------------------------------------------------------
# sensitivity: what the old bars accept and the new checks reject
# ---------------------------------------------------------------------------------------------------------------------------
def _analysis_case(N=1024, n=6000, combo="f32f64"):
    td = O.combo_types(combo)[0]
    x = sine_sweep(n, dtype=td)
    ref = O.best(N, "hann", 1.0, combo)
    d = ref.sdft(x)
    st = X.Stream(x, N, combo)
    rows = X.sample_rows(n, extra=range(n - 64, n), count=160, seed=5)
    Zx = st.rows(rows, "hann")
    F = X.analysis_floor(combo, N, st.A(rows), J=n // 512, L=512)             # a route of 512-sample chunks
    E_ref = X.bin_errors(d[rows], Zx)
    return x, d, st, rows, Zx, F, E_ref


def _rejected(fn):
    with pytest.raises(AssertionError):
        fn()


def test_mutation_edge_bin_scaled():
    """Bin N-1 scaled by (1 + 1e-10) at FD double: about 4e-12 against the 1e-11 bar, rejected per bin."""
    x, d, st, rows, Zx, F, E_ref = _analysis_case()
    m = d.copy()
    m[:, -1] *= 1 + 1e-10
    old = rel_err(m, d)
    assert old <= 1e-11, old
    X.check_bins(E_ref, E_ref, F)                                # the unmutated reference passes its own check
    _rejected(lambda: X.check_bins(X.bin_errors(m[rows], Zx), E_ref, F))


def test_mutation_carry_in_of_one_chunk():
    """One time chunk's carry-in perturbed by 1e-9 relative in one low-energy bin: acc[k] of the chunk's first sample off by
    1e-9 |acc[k]|, which every later row carries (demodulated, then spread by the window's taps)."""
    N = 1024
    x, d, st, rows, Zx, F, E_ref = _analysis_case(N)
    t0 = 3072                                                     # a chunk start (chunk of 512 samples)
    X0 = np.abs(st.demod([t0 - 1])[0]).astype(np.float64)
    k = int(np.argmin(np.abs(np.log10(np.maximum(X0, 1e-300) / X0.max()) + 2.5)))   # a bin 10^-2.5 below the strongest one
    k = min(max(k, 2), N - 3)
    dacc = 1e-9 * float(X0[k])
    t = np.arange(d.shape[0])
    dX = np.where(t >= t0, dacc, 0.0) * np.exp(1j * np.pi * ((k * (t + 1)) % (2 * N)) / N)
    m = d.copy()
    for j, tap in ((-1, -0.25), (0, 0.5), (1, -0.25)):
        m[:, k + j] += (tap / (2 * N)) * dX
    old = rel_err(m, d)
    assert old <= 1e-11, old
    _rejected(lambda: X.check_bins(X.bin_errors(m[rows], Zx), E_ref, F))


def _fused_case(N, window, latency, n=5000, combo="f64f64"):
    """FD double with TD double: y is not rounded to float, so what the fused call adds to it stays visible."""
    td, fd, fdx = O.combo_types(combo)
    x = (sine_sweep(n, dtype=td) * 0.6 + noise(n, seed=9, dtype=td) * 0.4).astype(td)
    ref = O.best(N, window, latency, combo)
    d = ref.sdft(x)
    y = ref.isdft(d)
    st = X.Stream(x, N, combo)
    rows = X.sample_rows(n, count=256, seed=6)
    yx, S = X.exact_synthesis(st.rows(rows, window), N, latency)
    Fy = X.pipeline_floor(combo, combo, N, latency, S, X.serial_bound(combo, N, st.A(rows), L=n))
    X.check_pipeline(y[rows], y[rows], yx, Fy)
    return x, d, y, st, rows, yx, Fy


def test_mutation_synthesis_twiddles_in_float():
    """The fused call's synthesis with its twiddle table rounded to float, FD double.  (Latency 0.3: at latency 0.5 the table is
    2 e^{-i pi k / 2}, whose entries float holds exactly, and the rounding changes nothing -- checked first.)"""
    N = 1024
    _, syn, w = O.best(N, "hann", 0.5, "f64f64").tables()
    assert np.abs(syn.astype(np.complex64).astype(np.complex128) - syn).max() <= 1e-15
    latency = 0.3
    x, d, y, st, rows, yx, Fy = _fused_case(N, "hann", latency)
    _, syn, w = O.best(N, "hann", latency, "f64f64").tables()
    syn32 = syn.astype(np.complex64).astype(np.complex128)
    m = w[1] * (d * syn32[None, :]).real.sum(axis=1)
    old = rel_err(m, y)
    assert old <= 1e-6, old
    _rejected(lambda: X.check_pipeline(m[rows], y[rows], yx, Fy))


def test_mutation_hamming_neighbour_tap():
    """The fused call's Hamming neighbour tap off by 1e-7 (0.23 + 1e-7): Z[k] -= 1e-7 w (X[k-1] + X[k+1])."""
    N, latency = 256, 1.0
    x, d, y, st, rows, yx, Fy = _fused_case(N, "hamming", latency)
    Xd = st.demod(np.arange(x.size))
    Zn = X.window_rows(Xd, N, "boxcar") * 0                      # (shape)
    src, cj, zero = X._halo_map(N)
    for j in (-1, 1):
        cell = np.where(cj[j + 2][None, :], np.conj(Xd[:, src[j + 2]]), Xd[:, src[j + 2]])
        Zn = Zn + cell
    md = (d - (1e-7 / (2 * N)) * Zn.astype(np.complex128)).astype(d.dtype)
    m = O.best(N, "hamming", latency, "f64f64").isdft(md)
    old = rel_err(m, y)
    assert old <= 1e-6, old
    _rejected(lambda: X.check_pipeline(m[rows], y[rows], yx, Fy))


def test_mutation_one_fold_coefficient_in_float():
    """The folded form sums y_t = sum_m re(c_m X_t[m]) with c_m = (2 / 2N) sum_j tap_j syn_{m-j}; one bin's coefficient rounded
    to float (the bin that carries the most energy over the call).  Latency 0.3: at 0.5 the coefficients are w syn_m, exact in float."""
    N, latency = 256, 0.3
    x, d, y, st, rows, yx, Fy = _fused_case(N, "hann", latency)
    Xd = st.demod(np.arange(x.size)).astype(np.complex128)
    mbin = int(np.argmax(np.abs(Xd).sum(axis=0)[2:N - 2])) + 2
    syn = X.synthesis_twiddles(N, latency).astype(np.complex128)
    c = 2.0 / (2 * N) * sum(X.TAPS["hann"][abs(j)] * syn[mbin - j] for j in (-1, 0, 1))
    dc = complex(np.complex64(c)) - c
    m = y + (dc * Xd[:, mbin]).real
    old = rel_err(m, y)
    assert old <= 1e-6, old
    _rejected(lambda: X.check_pipeline(m[rows], y[rows], yx, Fy))
