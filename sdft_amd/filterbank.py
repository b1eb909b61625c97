"""Filterbanks for :meth:`sdft_amd.SDFT.set_filterbank`, in pure numpy (built once per plan: nothing here is on the hot path).

A plan of ``dftsize`` bins at ``samplerate`` has its bin k at the frequency ``k * samplerate / (2 * dftsize)``.  Both builders
return ``(bin0, nbins, weights)``: band b covers the bins ``bin0[b] <= k < bin0[b] + nbins[b]`` with the weights
``weights[off_b + (k - bin0[b])]``, ``off_b = sum(nbins[:b])`` -- the arguments of ``set_filterbank``.  A band that would cover no
bin (narrower than the bin spacing and between two bins) is dropped, so fewer bands than asked for may come back."""

import numpy as np


def bin_frequencies(dftsize: int, samplerate: float) -> np.ndarray:
    """Centre frequency of every bin of the plan, in the unit of ``samplerate``."""
    return np.arange(int(dftsize), dtype=np.float64) * (float(samplerate) / (2.0 * int(dftsize)))


def hz_to_mel(f):
    """The HTK formula: ``2595 * log10(1 + f / 700)``."""
    return 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_to_hz(m):
    return 700.0 * (10.0 ** (np.asarray(m, dtype=np.float64) / 2595.0) - 1.0)


def _pack(bands):
    """[(first bin, weights of consecutive bins)] -> (bin0, nbins, weights); bands without bins are left out."""
    bands = [(k0, w) for k0, w in bands if len(w)]
    bin0 = np.array([k0 for k0, _ in bands], dtype=np.uint64)
    nbins = np.array([len(w) for _, w in bands], dtype=np.uint64)
    weights = np.concatenate([w for _, w in bands]) if bands else np.zeros(0, dtype=np.float64)
    return bin0, nbins, weights.astype(np.float64)


def mel(dftsize: int, samplerate: float, nbands: int, fmin: float = 0.0, fmax=None):
    """``nbands`` triangles whose corners are equally spaced on the HTK mel scale between ``fmin`` and ``fmax`` (``None``: the
    Nyquist frequency), evaluated at the plan's bin frequencies.  Triangle b rises from 0 at corner b to 1 at corner b + 1 (its
    centre) and falls to 0 at corner b + 2; the band is the bins strictly inside (corner b, corner b + 2), where the weight is
    positive.  Between the first and the last centre the weights of adjacent triangles sum to 1 at every bin."""
    dftsize, nbands = int(dftsize), int(nbands)
    if dftsize < 1 or nbands < 1:
        raise ValueError("dftsize and nbands must be at least 1")
    fmax = float(samplerate) / 2.0 if fmax is None else float(fmax)
    fmin = float(fmin)
    if not 0.0 <= fmin < fmax:
        raise ValueError(f"need 0 <= fmin < fmax, got {fmin}, {fmax}")
    f = bin_frequencies(dftsize, samplerate)
    corners = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), nbands + 2))
    bands = []
    for b in range(nbands):
        lo, mid, hi = corners[b], corners[b + 1], corners[b + 2]
        inside = np.nonzero((f > lo) & (f < hi))[0]
        if inside.size == 0:
            continue
        fk = f[inside]
        w = np.where(fk <= mid, (fk - lo) / (mid - lo), (hi - fk) / (hi - mid))
        bands.append((int(inside[0]), w))
    return _pack(bands)


def fractional_octave(dftsize: int, samplerate: float, fraction: int = 3, fmin: float = 20.0):
    """Rectangular bands (weight 1) of 1 / ``fraction`` octave: band j covers the bins whose frequency lies in
    ``[fmin * 2**(j / fraction), fmin * 2**((j + 1) / fraction))``, up to the last bin of the plan.  Disjoint and ascending."""
    dftsize, fraction = int(dftsize), int(fraction)
    if dftsize < 1 or fraction < 1 or not fmin > 0.0:
        raise ValueError("dftsize and fraction must be at least 1 and fmin positive")
    f = bin_frequencies(dftsize, samplerate)
    top = f[-1]
    bands = []
    j = 0
    while fmin * 2.0 ** (j / fraction) <= top:
        lo, hi = fmin * 2.0 ** (j / fraction), fmin * 2.0 ** ((j + 1) / fraction)
        inside = np.nonzero((f >= lo) & (f < hi))[0]
        if inside.size:
            bands.append((int(inside[0]), np.ones(inside.size, dtype=np.float64)))
        j += 1
    return _pack(bands)


def flat(bin0, nbins):
    """Bands of weight 1: band b covers the bins ``bin0[b] <= k < bin0[b] + nbins[b]`` -- what a peak search over bin ranges
    (:meth:`sdft_amd.SDFT.band_peak`) installs.  Scalars give one band.  Bands without bins are dropped, as by the other builders."""
    b0 = np.atleast_1d(np.asarray(bin0, dtype=np.int64))
    nb = np.atleast_1d(np.asarray(nbins, dtype=np.int64))
    if b0.shape != nb.shape or b0.ndim != 1:
        raise ValueError("bin0 and nbins must have one entry per band")
    if (b0 < 0).any() or (nb < 0).any():
        raise ValueError("bin0 and nbins must not be negative")
    return _pack([(int(k0), np.ones(int(n), dtype=np.float64)) for k0, n in zip(b0, nb)])


def peak_frequency(bins, dftsize: int, samplerate: float) -> np.ndarray:
    """The frequency of the bins :func:`sdft_amd.sdft.band_peak_split` returns, by the rule of :func:`bin_frequencies`:
    ``bins * samplerate / (2 * dftsize)``, in the unit of ``samplerate``."""
    return np.asarray(bins, dtype=np.float64) * (float(samplerate) / (2.0 * int(dftsize)))


def dense(dftsize: int, bin0, nbins, weights) -> np.ndarray:
    """The filterbank as a dense (nbands, dftsize) matrix W, so that ``W @ power_row`` is what the filterbank analysis computes
    (bands that repeat stay separate rows)."""
    bin0 = np.asarray(bin0, dtype=np.int64)
    nbins = np.asarray(nbins, dtype=np.int64)
    weights = np.asarray(weights)
    W = np.zeros((bin0.size, int(dftsize)), dtype=weights.dtype if weights.size else np.float64)
    off = 0
    for b in range(bin0.size):
        W[b, bin0[b]:bin0[b] + nbins[b]] = weights[off:off + nbins[b]]
        off += int(nbins[b])
    return W
