"""Exact model of the sliding DFT, for judging the routes that are not bit-exact by design.  TEST HELPER (plain numpy).

The bit-exact routes are compared with the oracle bit for bit.  The others (chunk-parallel carries, the folded and tree-sum
forms of the fused call, exact_inverse = 0, float_carry_parallel) can only be held to a truth that does not share the
reference's rounding.  This module computes that truth in extended precision, and the error measures and bounds the tests
apply to it.

Analysis.  The reference steps, per sample t and bin k (oracle/sdft_oracle.c analyse_one),
    delta_t  = x[t] - x[t-2N]                              rounded to TD precision
    acc[k]  += delta_t * fid[k],  fid[k] = e^{-i pi k (t mod 2N) / N}
    X_t[k]   = acc[k] * conj(fid after the step)  = sum_{s <= t} delta_s e^{+i pi k (t+1-s) / N}
With exact differences the sum telescopes to a 2N-point DFT of the last 2N samples,
    X_t[k]   = sum_{d=0}^{2N-1} x[t-d] e^{+i pi k (d+1) / N},
and the rounding error e_s of each difference (the one place where the reference's arithmetic is part of the operation:
every implementation forms the same rounded differences) adds
    e^{+i pi k (t+1) / N} * sum_r C_r(t) e^{-2 pi i k r / (2N)},   C_r(t) = sum_{s <= t, s = r mod 2N} e_s,
one more DFT of the errors folded by residue.  e_s is found exactly with TwoSum (for TD double a plain float64 subtraction
cannot see its own error).  The halo is the reference's iterated reflection about bin 0 and bin N-1, each reflection
conjugating (N = 1: the halo cells stay zero, as halo_at does); the window is the reference's taps times 1/(2N).
Both DFTs run in np.longdouble (64-bit significand here), so the model's own error is about 2^-11 of float64's.

Synthesis.  y_t = 2 * sum_k re(Z_t[k] * syn_k), syn_k = g e^{i omega k N latency}, g = 2 / (1 - cos(omega N latency)),
omega = -pi / N; at latency 1 that is the sign-alternating sum 2 * sum_k (-1)^k re Z_t[k].  Summed in np.longdouble.

Error measures and the criterion (every bound below is a formula; none is read off a GPU run).
  eps_P      unit roundoff of precision P: 2^-24 (float), 2^-53 (double).
  A          l1 bound of one windowed bin over the window, (1/2N) * sum_{d<2N} |x[t-d]|, the maximum over the rows compared
             (the window taps have |taps| summing to 1, so |Z_t[k]| <= A_t).
  Analysis   per bin:  E[k] = max over the compared rows |Z[t,k] - Z_exact[t,k]|.
             Serial bound  B = eps_FD * A * 2 * (sqrt(L) + sqrt(2N) + log2(2N) + 2), L the number of samples stepped one by
             one (the whole stream for the reference).  Each term is the standard (random-walk) growth of one stage of the
             recurrence: the accumulator over L additions, the fiddle over <= 2N multiplications since its roll-over, and the
             demodulation and window; the factor 2 is real and imaginary part.  The reference is held to E_ref[k] <= C B.
             Floor of a route  F = eps_FD * A * 2 * (sqrt(L) + log2(2N) + sqrt(J) + 2), L the route's time chunk and J its
             number of chunks: the carry of a chunk is a sum of its L differences times twiddles (directly or folded and
             transformed: log2(2N)), the carries are scanned over J chunks, the fiddle is rebuilt from a table, then the
             demodulation and window.  The partial sums of a carry are of the l1 scale A whatever the bin, where the
             reference's running sum errs relative to the bin itself: on a quiet bin a route may be an order of magnitude
             less accurate than the serial reference and still right, which is what this floor admits.
  Synthesis  per sample, S_t = 2 * sum_k |Z_exact[t,k] * syn_k| is the sum of the magnitudes of the terms that any
             summation order adds.  f = eps_TD + eps_FD * (ceil(log2 N) + 3): a tree sum of N terms errs by at most
             ceil(log2 N) eps_FD of sum|terms| (Higham, Accuracy and Stability, 4.2), the products Z * syn and the synthesis
             table add 2 eps_FD, the final rounding to TD eps_TD.  (The reference's in-order sum, up to (N-1) eps_FD, is
             measured, not bounded.)  Rows fed in exactly (exact_inverse = 0 alone): r(t) = |y_t - y_exact,t| / S_t,
             E = max_t r(t), floor f.  Whole pipelines (the fused call): per sample |y_t - y_exact,t| against
             F_y(t) = f S_t + 2 max|syn| sqrt(N) B, the second term the rows' own errors (<= B per bin, N of them adding as a
             random walk) carried through the synthesis; a quiet sample (S_t small) sees mostly that term.
             Gate: discontinuous in the rows, so compared only on samples whose every bin lies farther from the threshold
             than the analysis error bound (gate_margin_ok).
  Criterion  a route is at least as accurate as the reference up to a small factor:
                 E_path <= C * max(E_ref, floor),   C = 4,
             with E_ref measured from the oracle (oracle.best) on the same rows / samples.  C = 4 allows for the route's
             different operation order: its rounding errors are not the reference's, only of the same size.
"""

from __future__ import annotations

import math

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
PI = np.arccos(LD(-1))
EPS = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
TAPS = {"boxcar": (1.0,), "hann": (0.5, -0.25), "hamming": (0.54, -0.23), "blackman": (0.42, -0.25, 0.04)}
WINDOW_NAMES = ("boxcar", "hann", "hamming", "blackman")
C_FACTOR = 4.0
TD_DTYPE = {"f32": np.float32, "f64": np.float64}


def _window_name(window) -> str:
    return window if isinstance(window, str) else WINDOW_NAMES[int(window)]


def _td(td) -> str:
    if isinstance(td, str):
        return td[:3]
    return "f32" if np.dtype(td) == np.float32 else "f64"


# ---- analysis ---------------------------------------------------------------------------------------------------------------
def delta_errors(x, N: int, td) -> np.ndarray:
    """e_s = delta_s as the reference rounds it (TD precision) minus the exact x[s] - x[s-2N], as float64 (exact)."""
    td = _td(td)
    xt = np.asarray(x, dtype=TD_DTYPE[td])
    L = 2 * N
    old = np.zeros_like(xt)
    old[L:] = xt[:-L] if xt.size > L else old[L:]
    a = xt.astype(np.float64)
    b = -old.astype(np.float64)
    s = a + b                                          # TwoSum: a + b = s + err exactly
    bb = s - a
    err = (a - (s - bb)) + (b - bb)
    if td == "f64":
        return -err                                    # rounded delta is s
    dr = (xt - old).astype(np.float64)                 # the float difference, widened (exact)
    return (dr - s) - err                              # (dr - s) is exact: both round the same real number


def _halo_map(N: int):
    """(src, conj) of the halo cell k + j for j in -2..2: the reference's iterated reflection (oracle halo_at)."""
    src = np.zeros((5, N), dtype=np.int64)
    cj = np.zeros((5, N), dtype=bool)
    zero = np.zeros((5, N), dtype=bool)
    for j in range(-2, 3):
        for k0 in range(N):
            k, flip = k0 + j, False
            if N == 1 and k != 0:
                zero[j + 2, k0] = True
                continue
            while k < 0 or k > N - 1:
                k = -k if k < 0 else 2 * (N - 1) - k
                flip = not flip
            src[j + 2, k0], cj[j + 2, k0] = k, flip
    return src, cj, zero


def _phase(k, m, N):
    """e^{+i pi k m / N} for integer arrays, the product reduced mod 2N exactly first."""
    a = (np.asarray(k, dtype=np.int64) * np.asarray(m, dtype=np.int64)) % (2 * N)
    ang = PI * a.astype(LD) / LD(N)
    return np.cos(ang) + 1j * np.sin(ang)


class Stream:
    """One channel's stream from a zero state: x in TD precision, the delta rounding errors and their per-residue running sums,
    so that any set of rows costs O(|rows| N log N) after O(n) set-up."""

    def __init__(self, x, N: int, td="f32"):
        self.td = _td(td)
        self.x = np.ascontiguousarray(x, dtype=TD_DTYPE[self.td])
        self.N = int(N)
        self.n = self.x.size
        L = 2 * self.N
        e = delta_errors(self.x, self.N, self.td)
        q = -(-self.n // L) if self.n else 0
        E = np.zeros(q * L)
        E[:self.n] = e
        self._P = np.cumsum(E.reshape(q, L), axis=0) if q else np.zeros((0, L))
        self._x64 = self.x.astype(np.float64)
        self._absx = np.abs(self._x64)

    def _windows(self, rows):
        L = 2 * self.N
        idx = rows[:, None] - np.arange(L)[None, :]
        v = np.where(idx >= 0, self._x64[np.maximum(idx, 0)], 0.0)
        return v

    def demod(self, rows) -> np.ndarray:
        """X_t[k] (unwindowed, demodulated) for the stream's samples `rows`: (R, N) clongdouble."""
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        assert rows.size == 0 or (rows.min() >= 0 and rows.max() < self.n)
        N, L = self.N, 2 * self.N
        k = np.arange(N)
        v = self._windows(rows).astype(LD)
        main = np.fft.ifft(v, axis=1)[:, :N] * L * _phase(k, 1, N)[None, :]       # sum_d v[d] e^{+2 pi i k (d+1) / 2N}
        q, r0 = rows // L, rows % L
        C = self._P[q].copy()
        prev = np.where(q[:, None] > 0, self._P[np.maximum(q - 1, 0)], 0.0)
        later = np.arange(L)[None, :] > r0[:, None]
        C[later] = prev[later]
        corr = np.fft.fft(C.astype(LD), axis=1)[:, :N] * _phase(k[None, :], (rows + 1)[:, None], N)
        return main + corr

    def acc(self, t: int) -> np.ndarray:
        """The accumulator after sample t (what get_state returns after a call that ended there): e^{-i pi k (t+1)/N} X_t."""
        k = np.arange(self.N)
        return self.demod([t])[0] * np.conj(_phase(k, t + 1, self.N))

    def rows(self, rows, window) -> np.ndarray:
        """Windowed rows Z_t[k], (R, N) clongdouble."""
        return window_rows(self.demod(rows), self.N, window)

    def A(self, rows) -> float:
        """max over rows of (1/2N) sum |x| over the row's window."""
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        cs = np.concatenate([[0.0], np.cumsum(self._absx)])
        lo = np.maximum(rows - 2 * self.N + 1, 0)
        return float(((cs[rows + 1] - cs[lo]) / (2 * self.N)).max()) if rows.size else 0.0


def window_rows(X, N: int, window) -> np.ndarray:
    taps = TAPS[_window_name(window)]
    src, cj, zero = _halo_map(N)
    Z = np.zeros(X.shape, dtype=CLD)
    for j in range(-(len(taps) - 1), len(taps)):
        cell = X[:, src[j + 2]]
        cell = np.where(cj[j + 2][None, :], np.conj(cell), cell)
        cell = np.where(zero[j + 2][None, :], 0, cell)
        Z += LD(taps[abs(j)]) * cell
    return Z / LD(2 * N)


def exact_rows(x, N: int, window, rows, td="f32") -> np.ndarray:
    """Windowed rows of the stream x (one channel, from a zero state) at the sample indices `rows`: (R, N) clongdouble."""
    return Stream(x, N, td).rows(rows, window)


# ---- synthesis ------------------------------------------------------------------------------------------------------------
def synthesis_twiddles(N: int, latency: float) -> np.ndarray:
    if latency == 1:
        return np.where(np.arange(N) % 2, LD(-1), LD(1)).astype(CLD)
    omega = -PI / LD(N)
    g = LD(2) / (LD(1) - np.cos(omega * LD(N) * LD(latency)))
    ang = omega * np.arange(N).astype(LD) * LD(N) * LD(latency)
    return g * (np.cos(ang) + 1j * np.sin(ang))


def exact_synthesis(Z, N: int, latency: float):
    """-> (y, S): y_t = 2 sum_k re(Z_t[k] syn_k), S_t = 2 sum_k |Z_t[k] syn_k|, both (R,) longdouble."""
    Z = np.asarray(Z).astype(CLD).reshape(-1, N)
    terms = Z * synthesis_twiddles(N, latency)[None, :]
    return 2 * terms.real.sum(axis=1), 2 * np.abs(terms).sum(axis=1)


# ---- operations -------------------------------------------------------------------------------------------------------------
FUZZ_EXPR = ("const sdft_fd_t g = p[0] + p[1] * (sdft_fd_t)k / (sdft_fd_t)nbins + p[2] * cos(p[3] * (sdft_fd_t)t) + p[4] * (sdft_fd_t)ch;"
             " re *= g; im *= g;")


def expr_gain(N, t_call, pv, ch=0):
    """FUZZ_EXPR's factor for the call's samples t_call (the tests' expression, tests/test_gpu_fuzz.py)."""
    k = np.arange(N, dtype=np.float64)[None, :]
    t = np.asarray(t_call, dtype=np.float64)[:, None]
    return pv[0] + pv[1] * k / N + pv[2] * np.cos(pv[3] * t) + pv[4] * ch


def apply_op(Z, op, t_call, gain=None, shift=0, hop=0, threshold=0.0, floor=0.0, exponent=1.0, scale=1.0, expr_params=(), ch=0,
             xp=np):
    """The operation on rows Z (R, N) at the call's sample indices t_call, in the precision of Z (numpy)."""
    N = Z.shape[1]
    t_call = np.asarray(t_call, dtype=np.int64)
    if op == "identity":
        return Z
    if op in ("gain", "cgain"):
        return Z * np.asarray(gain)[None, :]
    if op == "shift":
        out = np.zeros_like(Z)
        s = int(shift)
        if s >= 0:
            out[:, s:] = Z[:, :N - s] if s < N else 0
        else:
            out[:, :N + s] = Z[:, -s:]
        return out
    if op in ("gain_rows", "cgain_rows"):
        g = np.asarray(gain)
        r = np.minimum(t_call // int(hop), g.shape[0] - 1)
        return Z * g[r]
    if op == "power":
        mag = np.abs(Z)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = scale * np.power(mag, exponent - 1)
        return np.where(mag > 0, Z * f, 0)
    if op == "gate":
        return np.where(np.abs(Z) < threshold, Z * floor, Z)
    if op == "expr":
        return Z * expr_gain(N, t_call, expr_params, ch)
    raise ValueError(op)


def gate_margin_ok(Z, threshold, bound) -> np.ndarray:
    """Samples whose every bin lies farther than `bound` from the gate's threshold: only there is the gate's output a
    continuous function of the rows, so only there may a route be compared (a bin within the analysis error of the
    threshold may be gated by one route and kept by another, both correctly)."""
    return np.all(np.abs(np.abs(Z).astype(np.float64) - threshold) > bound, axis=1)


# ---- error measures ---------------------------------------------------------------------------------------------------------
def analysis_floor(fd, N: int, A: float, J: int = 1, L: int = 1) -> float:
    """F = eps_FD * A * 2 * (sqrt(L) + log2(2N) + sqrt(J) + 2); see the module docstring."""
    return EPS[fd[-3:]] * A * 2.0 * (math.sqrt(L) + math.log2(2 * N) + math.sqrt(J) + 2.0)


def serial_bound(fd, N: int, A: float, L: int) -> float:
    """B = eps_FD * A * 2 * (sqrt(L) + sqrt(2N) + log2(2N) + 2); see the module docstring."""
    return EPS[fd[-3:]] * A * 2.0 * (math.sqrt(L) + math.sqrt(2 * N) + math.log2(2 * N) + 2.0)


def synthesis_floor(td, fd, N: int) -> float:
    """f = eps_TD + eps_FD * (ceil(log2 N) + 3); see the module docstring."""
    return EPS[_td(td)] + EPS[fd[-3:]] * (math.ceil(math.log2(max(N, 1))) + 3)


def bin_errors(Z, Zx) -> np.ndarray:
    """E[k] = max over rows |Z[t,k] - Z_exact[t,k]| (float64)."""
    d = np.asarray(Z).astype(CLD) - np.asarray(Zx).astype(CLD)
    return np.abs(d).astype(np.float64).reshape(-1, d.shape[-1]).max(axis=0)


def sample_errors(y, yx, S) -> np.ndarray:
    """r(t) = |y_t - y_exact,t| / S_t (float64); a sample with S_t = 0 counts its absolute error."""
    d = np.abs(np.asarray(y).astype(LD) - np.asarray(yx).astype(LD)).astype(np.float64)
    S = np.asarray(S, dtype=np.float64)
    return np.where(S > 0, d / np.where(S > 0, S, 1.0), d)


def check_bins(E_path, E_ref, F, C=C_FACTOR, what=""):
    """Per bin E_path[k] <= C max(E_ref[k], F).  -> (worst E_path / bound, worst E_path / E_ref) for reporting."""
    bound = C * np.maximum(E_ref, F)
    ratio = E_path / bound
    k = int(np.argmax(ratio))
    assert ratio[k] <= 1.0, (what, "bin", k, float(E_path[k]), float(E_ref[k]), F, float(ratio[k]))
    return float(ratio.max()), float((E_path / np.maximum(E_ref, F)).max())


def check_samples(r_path, r_ref, f, C=C_FACTOR, what=""):
    """max_t r_path <= C max(max_t r_ref, f).  -> (E_path / bound, E_path / E_ref)."""
    e_path, e_ref = float(np.max(r_path)), float(np.max(r_ref))
    bound = C * max(e_ref, f)
    t = int(np.argmax(r_path))
    assert e_path <= bound, (what, "sample", t, e_path, e_ref, f)
    return e_path / bound, e_path / max(e_ref, f)


def oracle_rows(ref, x, rows, chunk=1 << 16):
    """The oracle's rows of the stream x at the sample indices `rows` (sorted), without keeping the whole matrix: the stream
    is run in pieces through `ref` (which must start from a zero state)."""
    rows = np.asarray(rows, dtype=np.int64)
    out = np.empty((rows.size, ref.dftsize), dtype=ref.fdx)
    for a in range(0, len(x), chunk):
        b = min(a + chunk, len(x))
        d = ref.sdft(x[a:b])
        sel = (rows >= a) & (rows < b)
        out[sel] = d[rows[sel] - a]
    return out


def sample_rows(n: int, extra=(), count: int = 48, seed: int = 0) -> np.ndarray:
    """A sorted set of row indices of an n-sample stream: the first and last rows, `extra`, and `count` seeded others."""
    rng = np.random.default_rng(seed)
    pick = set(int(v) for v in extra if 0 <= v < n) | {0, n - 1}
    pick |= set(int(v) for v in rng.integers(0, n, size=min(count, n)))
    return np.array(sorted(pick), dtype=np.int64)


def pipeline_floor(td, fd, N: int, latency: float, S, Fa: float):
    """Per-sample floor of a synthesised sample whose rows carry analysis errors up to Fa (the serial bound B) per bin:
        F_y(t) = f * S_t + 2 * max_k |syn_k| * sqrt(N) * Fa;  see the module docstring."""
    G = float(np.abs(synthesis_twiddles(N, latency)).max())
    return synthesis_floor(td, fd, N) * np.asarray(S, dtype=np.float64) + 2.0 * G * math.sqrt(N) * Fa


def check_pipeline(y_path, y_ref, yx, Fy, C=C_FACTOR, what=""):
    """Per sample |y_path - y_exact| <= C max(|y_ref - y_exact|, F_y(t)).  -> (worst E_path / bound, worst E_path / E_ref)."""
    yx = np.asarray(yx).astype(LD)
    e_path = np.abs(np.asarray(y_path).astype(LD) - yx).astype(np.float64)
    e_ref = np.abs(np.asarray(y_ref).astype(LD) - yx).astype(np.float64)
    bound = C * np.maximum(e_ref, Fy)
    ratio = e_path / bound
    t = int(np.argmax(ratio))
    assert ratio[t] <= 1.0, (what, "sample", t, float(e_path[t]), float(e_ref[t]), float(np.broadcast_to(Fy, e_path.shape)[t]))
    return float(ratio.max()), float((e_path / np.maximum(e_ref, Fy)).max())
