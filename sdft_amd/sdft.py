"""Host-side mirror of the reference's operator interface over the C-ABI.

``SDFT(dftsize, window, latency).sdft(x) / .isdft(dfts)`` has the shape of the reference's
Python class (/root/reference/python/src/sdft/sdft.py:30,76,122) and the call order of its C
test driver (/root/reference/test/test.c:49-93), but every call goes through
``libsdft_hip.so``: torch tensors on the GPU are passed as device pointers (nothing is copied),
numpy arrays take the library's staged host-pointer path.  torch is used for device memory
only.  There is no CPU implementation in this package.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from .capi import Api, OPS, STAGES, WINDOWS, SdftHipError

_NP_REAL = {"f32": np.float32, "f64": np.float64}
_NP_CPLX = {"f32": np.complex64, "f64": np.complex128}


def _torch():
    import torch
    return torch


def _is_tensor(a) -> bool:
    return type(a).__module__.startswith("torch")


def _grid_args(dftsize: int, every, first, bins=None, banded=True, word="bins"):
    """The arguments every grid analysis call of :class:`SDFT` takes, checked: (every, first, bin0, nbins)."""
    every, first = int(every), int(first)
    bin0, nb = (0, dftsize) if bins is None else (int(bins[0]), int(bins[1]))
    if every < 1 or first < 0:
        raise ValueError(f"every must be >= 1 and first >= 0, got every={every}, first={first}")
    if banded and (bin0 < 0 or nb < 1 or bin0 + nb > dftsize):
        raise ValueError(f"{word} = (bin0, nbins) must select at least one of the {dftsize} bins, got {(bin0, nb)}")
    return every, first, bin0, nb


class SDFT:
    """One analysis/synthesis plan = one stream (or a batch of independent channels).

    Parameters follow ``sdft_alloc_custom`` (reference sdft.h:413): ``dftsize`` bins, analysis
    ``window`` in {boxcar, hann, hamming, blackman}, synthesis ``latency`` in (0, 1].
    ``combo`` selects time/frequency domain scalar types (``SDFT_TD_*`` / ``SDFT_FD_*`` macros).
    ``channels`` > 1 allocates a batched plan (an addition over the reference).
    """

    def __init__(self, dftsize: int, window="hann", latency: float = 1.0, combo: str = "f32f64",
                 channels: int = 1, device=None, hooks: bool = False):
        # hooks: the plan lives in libsdft_hip_hooks.so (the same sources built with -DSDFT_HIP_TEST_HOOKS), whose set_option also knows
        # the keys that force every remaining fork of the host logic -- for the tests and the probes; see set_option below
        self.api = Api(combo, hooks=hooks)
        self._options = []                                   # (key, value) set so far, and the caller's stream: replayed when the plan moves
        self._stream = None
        self._pairs = None                                   # the pair list of set_pairs, likewise
        self._array = None                                   # the array of set_array, likewise
        self._mix = None                                     # the (weights, chan) of set_mix, likewise
        self.combo = combo
        self.td = _NP_REAL[combo[:3]]
        self.fd = _NP_REAL[combo[3:]]
        self.fdx = _NP_CPLX[combo[3:]]
        self.dftsize = int(dftsize)
        self.channels = int(channels)
        self.window = WINDOWS[window] if isinstance(window, str) else int(window)
        self.latency = float(latency)
        if device is not None:
            if self.api.lib.sdft_hip_set_device(int(device)) != 0:
                self.api.check()
        self._p = self.api.alloc_batch(self.dftsize, self.window, self.latency, self.channels)
        self.device = int(self.api.get_option(self._p, b"device")) if self._p else -1
        if not self._p:
            err = self.api.last_error()
            self.api.lib.sdft_hip_clear_error()
            raise SdftHipError(f"sdft_alloc failed: {err}")

    # ---- lifetime -----------------------------------------------------------------------
    def close(self):
        if getattr(self, "_p", None):
            self.api.free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def reset(self):
        self.api.clear()
        self.api.reset(self._p)
        self.api.check()

    def size(self) -> int:
        return int(self.api.size(self._p))

    # ---- options ------------------------------------------------------------------------
    def set_option(self, key: str, value: int):
        """sdft_hip_set_option.  A key the product library does not know may be a test hook (include/sdft/sdft_hip.h lists them): the plan
        then moves to libsdft_hip_hooks.so -- a new plan with the same parameters on the same device, the options set so far replayed
        and the stream state copied over (sdft_hip_get_state / set_state) -- so that the tests can force a route on any plan they make; a key
        neither build knows raises."""
        if self.api.set_option(self._p, key.encode(), int(value)) == 0:
            self._options.append((key, int(value)))
            return
        if not self.api.hooks:
            other = Api(self.combo, hooks=True)
            if self.device >= 0:
                other.lib.sdft_hip_set_device(self.device)
            q = other.alloc_batch(self.dftsize, self.window, self.latency, self.channels)
            if q and other.set_option(q, key.encode(), int(value)) == 0:
                for k, v in self._options:
                    other.set_option(q, k.encode(), v)
                acc, fid, hist, cursor = self.state()            # (synchronises; the plan may have been called already)
                self.api.free(self._p)
                self.api, self._p = other, q
                # (a plan nobody has called yet is not handed a state: an installed fid counts as the host's own, and the relay
                # form of the exact carries, which needs the canonical rotation, would never be taken)
                if cursor != 0 or np.any(acc) or np.any(hist):
                    self.set_state(acc, fid, hist, cursor)
                if self._stream is not None:
                    self.set_stream(self._stream)
                if self._pairs is not None:                      # (the installed pair list moves with the plan)
                    self.set_pairs(*self._pairs)
                if self._array is not None:                      # (and the installed array)
                    self.set_array(self._array)
                if self._mix is not None:                        # (and the installed mix)
                    self.set_mix(*self._mix)
                self._options.append((key, int(value)))
                return
            if q:
                other.free(q)
        raise SdftHipError(f"unknown option {key!r}")

    def get_option(self, key: str) -> int:
        return int(self.api.get_option(self._p, key.encode()))

    def set_stream(self, stream_handle: int):
        """Launch on a caller-owned HIP stream (e.g. ``torch.cuda.Stream().cuda_stream``)."""
        if self.api.set_stream(self._p, C.c_void_p(stream_handle)) != 0:
            self.api.check()
        self._stream = stream_handle

    def synchronize(self):
        if self.api.synchronize(self._p) != 0:
            self.api.check()

    def profile(self) -> dict:
        """-> {stage: (milliseconds, launches)} accumulated since the last call; needs option profile=1."""
        ms = (C.c_double * 4)()
        calls = (C.c_long * 4)()
        if self.api.get_profile(self._p, ms, calls) != 0:
            self.api.check()
        return {s: (ms[i], calls[i]) for i, s in enumerate(STAGES)}

    def state(self):
        """(acc, fid, hist, cursor) copied from the device; hist is in time order."""
        n, c = self.dftsize, self.channels
        acc = np.empty((c, n), dtype=self.fdx)
        fid = np.empty((c, n), dtype=self.fdx)
        hist = np.empty((c, 2 * n), dtype=self.td)
        cur = C.c_size_t(0)
        if self.api.get_state(self._p, acc.ctypes.data, fid.ctypes.data, hist.ctypes.data, C.byref(cur)) != 0:
            self.api.check()
        if c == 1:
            acc, fid, hist = acc[0], fid[0], hist[0]
        return acc, fid, hist, int(cur.value)

    def set_state(self, acc, fid, hist, cursor: int):
        """Checkpoint / resume: install a state obtained from :meth:`state` (of a plan with the same
        parameters, possibly on another GPU)."""
        acc = np.ascontiguousarray(acc, dtype=self.fdx); fid = np.ascontiguousarray(fid, dtype=self.fdx)
        hist = np.ascontiguousarray(hist, dtype=self.td)
        assert acc.size == self.channels * self.dftsize and hist.size == 2 * self.channels * self.dftsize
        if self.api.set_state(self._p, acc.ctypes.data, fid.ctypes.data, hist.ctypes.data, int(cursor)) != 0:
            self.api.check()
            raise SdftHipError("sdft_hip_set_state failed")

    # ---- analysis / synthesis ---------------------------------------------------------------
    def _check_tensor(self, t, what, dtype, shape=None):
        """Device tensors are handed to the library as raw pointers: they must live on the plan's GPU,
        be dense, and have exactly the element type and shape the C-ABI expects."""
        torch = _torch()
        if not t.is_cuda or t.device.index != self.device:
            raise ValueError(f"{what} must be a CUDA tensor on the plan's device cuda:{self.device}, got {t.device}")
        if not t.is_contiguous():
            raise ValueError(f"{what} must be contiguous")
        if t.dtype != getattr(torch, np.dtype(dtype).name):
            raise ValueError(f"{what} must have dtype {np.dtype(dtype).name}, got {t.dtype}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what} must have shape {tuple(shape)}, got {tuple(t.shape)}")

    def _shape_x(self, shape):
        if self.channels == 1 and len(shape) == 1:
            return shape[0]
        if len(shape) == 2 and shape[0] == self.channels:
            return shape[1]
        raise ValueError(f"samples must have shape (n,) or ({self.channels}, n), got {tuple(shape)}")

    def sdft(self, x, out=None):
        """Analyse samples ``x`` -> DFT matrix of shape (n, dftsize) [(channels, n, dftsize) if batched].

        State persists across calls exactly like the reference's plan (endless streaming).
        """
        self.api.clear()
        if _is_tensor(x):
            torch = _torch()
            n = self._shape_x(x.shape)
            self._check_tensor(x, "samples", self.td)
            shape = (n, self.dftsize) if x.dim() == 1 else (self.channels, n, self.dftsize)
            if out is None:
                out = torch.empty(shape, dtype=getattr(torch, np.dtype(self.fdx).name), device=x.device)
            self._check_tensor(out, "out", self.fdx, shape)
            self.api.sdft_n(self._p, n, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()))
        else:
            x = np.ascontiguousarray(x, dtype=self.td)
            n = self._shape_x(x.shape)
            shape = (n, self.dftsize) if x.ndim == 1 else (self.channels, n, self.dftsize)
            if out is None:
                out = np.empty(shape, dtype=self.fdx)
            assert out.flags.c_contiguous and out.shape == shape and out.dtype == self.fdx
            self.api.sdft_n(self._p, n, C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data))
        self.api.check()
        return out

    def _grid_call(self, name, x, rows_rule, every, first, extra, lead, trail, dtype, out):
        """One grid analysis call ``sdft_hip_<name>(plan, n, x, every, first, *extra, out)`` on checked arguments: a device tensor
        or a numpy array in, the same kind out, of shape (lead, rows, trail) -- ``lead=None``: (rows, trail) for 1-D samples,
        (channels, rows, trail) for batched ones --, ``rows = rows_rule(n, every, first)``, which the library must report too."""
        tensor = _is_tensor(x)
        if tensor:
            n = self._shape_x(x.shape)
            self._check_tensor(x, "samples", self.td)
        else:
            x = np.ascontiguousarray(x, dtype=self.td)
            n = self._shape_x(x.shape)
        rows = rows_rule(n, every, first)
        shape = (lead, rows, trail) if lead is not None else (rows, trail) if x.ndim == 1 else (self.channels, rows, trail)
        if tensor:
            torch = _torch()
            if out is None:
                out = torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device=x.device)
            self._check_tensor(out, "out", dtype, shape)
            xp, op = x.data_ptr(), (out.data_ptr() if rows else None)
        else:
            if out is None:
                out = np.empty(shape, dtype=dtype)
            assert out.flags.c_contiguous and out.shape == shape and out.dtype == dtype
            xp, op = x.ctypes.data, (out.ctypes.data if rows else None)
        got = getattr(self.api, name)(self._p, n, C.c_void_p(xp), every, first, *extra, C.c_void_p(op))
        if got < 0:
            self.api.check()
            raise SdftHipError(f"sdft_hip_{name} failed")
        self.api.check()
        assert got == rows, (got, rows)
        return out

    def sdft_every(self, x, every: int, first: int = 0, out=None):
        """Decimated analysis (``sdft_hip_sdft_every_n``): the rows :meth:`sdft` would return for the samples ``first``,
        ``first + every``, ... < n -> array of shape (rows, dftsize) [(channels, rows, dftsize) if batched], numpy for numpy
        input, a device tensor for a device tensor.  The plan's state advances over all n samples, as with :meth:`sdft`.
        The grid is local to the call: a streaming host passes :func:`every_next_first` as the next call's ``first``."""
        self.api.clear()
        every, first, _, _ = _grid_args(self.dftsize, every, first, banded=False)
        return self._grid_call("sdft_every_n", x, every_rows, every, first, (), None, self.dftsize, self.fdx, out)

    def power(self, x, every: int = 1, first: int = 0, bins=None, out=None):
        """Power-spectrogram analysis (``sdft_hip_sdft_power_n``): ``re*re + im*im`` of the bins ``bins = (bin0, nbins)`` (``None``:
        all) of the rows :meth:`sdft` would return for the samples ``first``, ``first + every``, ... < n -> real array of shape
        (rows, nbins) [(channels, rows, nbins) if batched], numpy for numpy input, a device tensor for a device tensor.  The
        complex rows are never stored.  The plan's state advances over all n samples and all bins, as with :meth:`sdft`; the grid is
        local to the call and streams with :func:`every_next_first`, as that of :meth:`sdft_every`."""
        self.api.clear()
        every, first, bin0, nb = _grid_args(self.dftsize, every, first, bins)
        return self._grid_call("sdft_power_n", x, every_rows, every, first, (bin0, nb), None, nb, self.fd, out)

    def set_filterbank(self, bin0, nbins, weights):
        """Installs a filterbank in the plan (``sdft_hip_set_filterbank``; the arrays are copied): band b covers the bins
        ``bin0[b] <= k < bin0[b] + nbins[b]`` with the weights ``weights[off_b + (k - bin0[b])]``, ``off_b = sum(nbins[:b])``.  Bands
        may overlap, repeat and come in any order.  No bands removes the filterbank.  :mod:`sdft_amd.filterbank` builds mel and
        fractional-octave filterbanks in this form."""
        self.api.clear()
        b0 = np.ascontiguousarray(bin0, dtype=np.uint64).ravel()
        nb = np.ascontiguousarray(nbins, dtype=np.uint64).ravel()
        w = np.ascontiguousarray(weights, dtype=self.fd).ravel()
        if b0.size != nb.size:
            raise ValueError(f"bin0 and nbins must have one entry per band, got {b0.size} and {nb.size}")
        if w.size != int(nb.sum()):
            raise ValueError(f"weights must hold sum(nbins) = {int(nb.sum())} numbers, got {w.size}")
        # (empty arrays still have an address: the library is never handed NULL for a filterbank that has bands)
        rc = self.api.set_filterbank(self._p, b0.size, C.c_void_p(b0.ctypes.data), C.c_void_p(nb.ctypes.data), C.c_void_p(w.ctypes.data))
        if rc != 0:
            self.api.check()
            raise SdftHipError("sdft_hip_set_filterbank failed")
        self.api.check()

    @property
    def filterbank_bands(self) -> int:
        """Bands of the installed filterbank (``sdft_hip_filterbank_bands``), 0 for none."""
        return int(self.api.filterbank_bands(self._p))

    def filterbank(self, x, every: int = 1, first: int = 0, out=None):
        """Filterbank analysis (``sdft_hip_sdft_filterbank_n``): per band of the installed filterbank (:meth:`set_filterbank`) the
        sum of ``weight * power`` over the band's bins, of the rows :meth:`power` would return for the samples ``first``,
        ``first + every``, ... < n -> real array of shape (rows, nbands) [(channels, rows, nbands) if batched], numpy for numpy
        input, a device tensor for a device tensor.  Neither the complex rows nor the powers are stored.  State and grid as with
        :meth:`power`."""
        self.api.clear()
        every, first, _, _ = _grid_args(self.dftsize, every, first, banded=False)
        nb = self.filterbank_bands
        if nb == 0:
            raise ValueError("no filterbank is installed: call set_filterbank first")
        return self._grid_call("sdft_filterbank_n", x, every_rows, every, first, (), None, nb, self.fd, out)

    def band_peak(self, x, every: int = 1, first: int = 0, out=None):
        """Band-peak analysis (``sdft_hip_sdft_band_peak_n``): per band of the installed filterbank (:meth:`set_filterbank`) the
        largest ``weight * power`` over the band's bins and the bin that attains it, of the rows :meth:`power` would return for the
        samples ``first``, ``first + every``, ... < n -> real array of shape (rows, nbands, 2) [(channels, rows, nbands, 2) if
        batched], numpy for numpy input, a device tensor for a device tensor: ``[..., 0]`` the value, ``[..., 1]`` the absolute bin
        as a number of the plan's real type (:func:`band_peak_split` gives integers).  With ``v`` the rounded products of a band in
        ascending bin order the pair is ``v[i], i = np.argmax(v)``: the lowest bin of the largest value, the lowest NaN bin if
        there is one.  Neither the complex rows nor the powers are stored.  State and grid as with :meth:`filterbank`."""
        self.api.clear()
        every, first, _, _ = _grid_args(self.dftsize, every, first, banded=False)
        nb = self.filterbank_bands
        if nb == 0:
            raise ValueError("no filterbank is installed: call set_filterbank first")
        flat = None
        if out is not None:
            if _is_tensor(out) != _is_tensor(x):
                raise ValueError("out must be of the samples' kind: a device tensor for a device tensor, a numpy array for numpy input")
            shape = tuple(out.shape)
            if len(shape) < 2 or shape[-2:] != (nb, 2):
                raise ValueError(f"out must end in (nbands, 2) = ({nb}, 2), got shape {shape}")
            if not (out.is_contiguous() if _is_tensor(out) else out.flags.c_contiguous):
                raise ValueError("out must be contiguous")       # (a reshape would copy, and the call would write the copy)
            flat = out.reshape(shape[:-2] + (2 * nb,))
        got = self._grid_call("sdft_band_peak_n", x, every_rows, every, first, (), None, 2 * nb, self.fd, flat)
        return out if out is not None else got.reshape(tuple(got.shape[:-1]) + (nb, 2))

    def set_pairs(self, a, b):
        """Installs a list of channel pairs in the plan (``sdft_hip_set_pairs``; the arrays are copied): pair p is the channels
        ``(a[p], b[p])``.  Pairs may repeat, come in any order and have ``a == b`` (the auto-spectrum).  No pairs removes the list."""
        self.api.clear()
        try:
            pa = np.ascontiguousarray(a, dtype=np.uint64).ravel()
            pb = np.ascontiguousarray(b, dtype=np.uint64).ravel()
        except OverflowError as e:
            raise ValueError(f"channel indices must not be negative: {e}") from None
        if pa.size != pb.size:
            raise ValueError(f"a and b must have one entry per pair, got {pa.size} and {pb.size}")
        rc = self.api.set_pairs(self._p, pa.size, C.c_void_p(pa.ctypes.data), C.c_void_p(pb.ctypes.data))
        if rc != 0:
            self.api.check()
            raise SdftHipError("sdft_hip_set_pairs failed")
        self.api.check()
        self._pairs = (pa, pb) if pa.size else None

    @property
    def pairs(self) -> int:
        """Pairs of the installed list (``sdft_hip_pairs``), 0 for none."""
        return int(self.api.pairs(self._p))

    def cross_sum(self, x, every: int = 1, first: int = 0, bins=None, out=None):
        """Pooled cross-spectrum analysis (``sdft_hip_sdft_cross_sum_n``): per pair ``(a, b)`` of the installed list
        (:meth:`set_pairs`) the sum of ``X_a * conj(X_b)`` over the windows :meth:`power_sum` cuts the n samples into, for the bins
        ``bins = (bin0, nbins)`` (``None``: all) -> complex array of shape (npairs, rows, nbins), ``rows = power_sum_rows(n, every,
        first)``, numpy for numpy input, a device tensor for a device tensor.  ``x`` is (channels, n) [(n,) for a single-channel
        plan].  Head row, streaming and sums-not-means as with :meth:`power_sum`.  The state of every channel of the plan advances
        over all n samples and all bins, as with :meth:`sdft`."""
        self.api.clear()
        every, first, bin0, nb = _grid_args(self.dftsize, every, first, bins)
        npairs = self.pairs
        if npairs == 0:
            raise ValueError("no pairs are installed: call set_pairs first")
        return self._grid_call("sdft_cross_sum_n", x, power_sum_rows, every, first, (bin0, nb), npairs, nb, self.fdx, out)

    def cross_smooth(self, x, decay: float, every: int = 1, first: int = 0, bins=None, state=None, out=None):
        """Smoothed cross-spectrum analysis (``sdft_hip_sdft_cross_smooth_n``): per pair ``(a, b)`` of the installed list
        (:meth:`set_pairs`) the one-pole average ``s = a * s + b * X_a * conj(X_b)`` of :meth:`cross_sum`'s ``every = 1`` term, each
        component on its own, ``(a, b) = smooth_coefficients(decay, dtype)``, advanced at every sample and kept on :meth:`power`'s
        grid -> complex array of shape (npairs, rows, nbins), numpy for numpy input, a device tensor for a device tensor: row r is
        the average after the sample ``first + r * every``.  ``x`` is (channels, n) [(n,) for a single-channel plan].  ``state`` is a
        numpy array or a device tensor (whatever ``x`` is) of shape (npairs, nbins) in the complex FD dtype, updated in place: the
        average before the first sample on entry, after the last on return; ``None`` starts from zero and drops the end value.  A
        stream passes ``state`` and :func:`every_next_first` from call to call; :func:`coherence` relates the pairs ``(a, b)``,
        ``(a, a)`` and ``(b, b)`` of one call.  The state of every channel of the plan advances over all n samples and all bins, as
        with :meth:`sdft`."""
        self.api.clear()
        every, first, bin0, nb = _grid_args(self.dftsize, every, first, bins)
        smooth_coefficients(decay, self.fd)                  # (raises for a decay the library would refuse)
        npairs = self.pairs
        if npairs == 0:
            raise ValueError("no pairs are installed: call set_pairs first")
        sp = None
        if state is not None:
            shape = (npairs, nb)
            if _is_tensor(state):
                self._check_tensor(state, "state", self.fdx, shape)
                sp = state.data_ptr()
            else:
                if not isinstance(state, np.ndarray) or state.dtype != self.fdx or not state.flags.c_contiguous or not state.flags.writeable:
                    raise ValueError(f"state must be a writable C-contiguous numpy array of dtype {np.dtype(self.fdx).name} (it is updated in place) or a device tensor")
                if state.shape != shape:
                    raise ValueError(f"state must have shape {shape}, got {state.shape}")
                sp = state.ctypes.data
        return self._grid_call("sdft_cross_smooth_n", x, every_rows, every, first, (bin0, nb, float(decay), C.c_void_p(sp)), npairs, nb, self.fdx, out)

    def set_array(self, chan):
        """Installs an array in the plan (``sdft_hip_set_array``; the list is copied): an ordered list of distinct channels, the
        elements of the array whose covariance :meth:`covariance` forms.  An int n means the channels ``0 ... n - 1``; an empty list
        (or 0) removes the array.  Independent of :meth:`set_pairs`: both may be installed."""
        self.api.clear()
        try:
            ch = np.arange(int(chan), dtype=np.uint64) if np.isscalar(chan) else np.ascontiguousarray(chan, dtype=np.uint64).ravel()
        except OverflowError as e:
            raise ValueError(f"channel indices must not be negative: {e}") from None
        rc = self.api.set_array(self._p, ch.size, C.c_void_p(ch.ctypes.data if ch.size else None))
        if rc != 0:
            self.api.check()
            raise SdftHipError("sdft_hip_set_array failed")
        self.api.check()
        self._array = ch if ch.size else None

    @property
    def array_channels(self) -> int:
        """Channels of the installed array (``sdft_hip_array_channels``), 0 for none."""
        return int(self.api.array_channels(self._p))

    def covariance(self, x, every: int = 1, first: int = 0, bins=None, out=None):
        """Array covariance analysis (``sdft_hip_sdft_covariance_n``): :meth:`cross_sum` for ALL pairs ``(i <= j)`` of the installed
        array (:meth:`set_array`), formed by register blocks of groups of channels -> complex array of shape (T, rows, nbins),
        ``T = nch (nch + 1) / 2``: the upper triangle in row-major order, the order of :func:`covariance_pairs`; element
        ``i * nch - i * (i - 1) / 2 + (j - i)`` holds the sums of ``X_chan[i] * conj(X_chan[j])`` and has :meth:`cross_sum`'s bits.
        Arguments, grid, head row, streaming and state as with :meth:`cross_sum`; :func:`covariance_matrix` expands the result to
        Hermitian matrices on the host."""
        self.api.clear()
        every, first, bin0, nb = _grid_args(self.dftsize, every, first, bins)
        nch = self.array_channels
        if nch == 0:
            raise ValueError("no array is installed: call set_array first")
        return self._grid_call("sdft_covariance_n", x, power_sum_rows, every, first, (bin0, nb), nch * (nch + 1) // 2, nb, self.fdx, out)

    def set_mix(self, weights, chan=None):
        """Installs a mix in the plan (``sdft_hip_set_mix``; list and weights are copied).  ``weights`` is a complex array of shape
        (nout, nch, dftsize) (or (nch, dftsize) for one output), applied as written: ``out[o] = sum_i weights[o, i] * X_chan[i]`` per
        bin, so a host that wants ``w^H x`` passes conjugates (:func:`mvdr_weights` does).  ``chan`` is an ordered list of ``nch``
        distinct channels, None for the channels ``0 ... nch - 1``.  ``weights=None`` removes the mix.  Independent of
        :meth:`set_pairs`, :meth:`set_array` and the filterbank."""
        self.api.clear()
        if weights is None:
            rc = self.api.set_mix(self._p, 0, 0, C.c_void_p(None), C.c_void_p(None))
            if rc != 0:
                self.api.check()
                raise SdftHipError("sdft_hip_set_mix failed")
            self.api.check()
            self._mix = None
            return
        w = weights.detach().cpu().numpy() if _is_tensor(weights) else np.asarray(weights)
        if w.ndim == 2:
            w = w[None]
        if w.ndim != 3 or w.shape[2] != self.dftsize or w.shape[0] == 0:
            raise ValueError(f"weights must be (nout, nch, {self.dftsize}) with nout >= 1, got {w.shape}")
        w = np.ascontiguousarray(w, dtype=self.fdx)
        nout, nch = int(w.shape[0]), int(w.shape[1])
        ch = None
        if chan is not None:
            try:
                ch = np.ascontiguousarray(chan, dtype=np.uint64).ravel()
            except OverflowError as e:
                raise ValueError(f"channel indices must not be negative: {e}") from None
            if ch.size != nch:
                raise ValueError(f"chan names {ch.size} channels but weights has {nch}")
        rc = self.api.set_mix(self._p, nout, nch, C.c_void_p(ch.ctypes.data if ch is not None and ch.size else None), C.c_void_p(w.ctypes.data if w.size else None))
        if rc != 0:
            self.api.check()
            raise SdftHipError("sdft_hip_set_mix failed")
        self.api.check()
        self._mix = (w, ch)

    @property
    def mix_outputs(self) -> int:
        """Outputs of the installed mix (``sdft_hip_mix_outputs``), 0 for none."""
        return int(self.api.mix_outputs(self._p))

    def mix(self, x, every: int = 1, first: int = 0, bins=None, out=None):
        """Channel-mix analysis (``sdft_hip_sdft_mix_n``): the per-bin weighted sums of the installed mix (:meth:`set_mix`) at the rows
        of :meth:`sdft_every`'s grid, for the bins ``bins = (bin0, nbins)`` (default: all) -> complex array of shape (nout, rows, nbins).
        Each value is the sequential sum over the mix's elements of ``w * X`` formed from four rounded products, in the FD type.  The
        stream state of every channel afterwards is the one :meth:`sdft` leaves; ``every_next_first`` gives the next call's
        ``first``."""
        self.api.clear()
        every, first, bin0, nb = _grid_args(self.dftsize, every, first, bins)
        nout = self.mix_outputs
        if nout == 0:
            raise ValueError("no mix is installed: call set_mix first")
        return self._grid_call("sdft_mix_n", x, every_rows, every, first, (bin0, nb), nout, nb, self.fdx, out)

    def power_sum(self, x, every: int = 1, first: int = 0, bins=None, out=None):
        """Pooled power analysis (``sdft_hip_sdft_power_sum_n``): the grid points ``first``, ``first + every``, ... cut the n samples
        into windows, and row r is the sum of :meth:`power`'s ``every = 1`` values over the r-th window, for the bins
        ``bins = (bin0, nbins)`` (``None``: all) -> real array of shape (rows, nbins) [(channels, rows, nbins) if batched],
        ``rows = power_sum_rows(n, every, first)``, numpy for numpy input, a device tensor for a device tensor.  With ``first > 0``
        row 0 is the head window ``[0, first)``: it completes the previous call's last row (add the two); the next call's
        ``first`` is :func:`every_next_first`.  Sums, not means: divide a row by its window's length for a mean.  The plan's state
        advances over all n samples and all bins, as with :meth:`sdft`."""
        self.api.clear()
        every, first, bin0, nb = _grid_args(self.dftsize, every, first, bins)
        return self._grid_call("sdft_power_sum_n", x, power_sum_rows, every, first, (bin0, nb), None, nb, self.fd, out)

    def power_peak(self, x, every: int = 1, first: int = 0, bins=None, hold="max", out=None):
        """Peak-hold analysis (``sdft_hip_sdft_power_peak_n``): :meth:`power_sum`'s grid, windows, head row, shapes and pointers,
        with the other statistic: row r is the largest (``hold="max"`` or 0) or the smallest (``hold="min"`` or 1) of
        :meth:`power`'s ``every = 1`` values over the r-th window, bit for bit one of them (NaN if the window holds a NaN).  With
        ``first > 0`` row 0 is the head window ``[0, first)``: it completes the previous call's last row (``np.maximum`` /
        ``np.minimum`` of the two); the next call's ``first`` is :func:`every_next_first`.  The plan's state advances over all n
        samples and all bins, as with :meth:`sdft`."""
        self.api.clear()
        every, first, bin0, nb = _grid_args(self.dftsize, every, first, bins)
        if hold not in HOLDS:
            raise ValueError(f"hold must be 'max' (0) or 'min' (1), got {hold!r}")
        return self._grid_call("sdft_power_peak_n", x, power_sum_rows, every, first, (bin0, nb, HOLDS[hold]), None, nb, self.fd, out)

    def power_smooth(self, x, decay: float, every: int = 1, first: int = 0, bins=None, state=None, out=None):
        """Smoothed power analysis (``sdft_hip_sdft_power_smooth_n``): the one-pole average ``s = a * s + b * p`` of :meth:`power`'s
        ``every = 1`` values ``p``, ``(a, b) = smooth_coefficients(decay, dtype)``, advanced at every sample and kept on
        :meth:`power`'s grid -> real array of shape (rows, nbins) [(channels, rows, nbins) if batched], numpy for numpy input, a
        device tensor for a device tensor: row r is the average after the sample ``first + r * every``.  ``state`` is a numpy array
        or a device tensor (whatever ``x`` is) of shape (nbins,) [(channels, nbins)] in the FD dtype, updated in place: the average
        before the first sample on entry, after the last on return; ``None`` starts from zero and drops the end value.  A stream
        passes ``state`` and :func:`every_next_first` from call to call.  :func:`smooth_decay` turns a time constant into
        ``decay``.  The plan's state advances over all n samples and all bins, as with :meth:`sdft`."""
        self.api.clear()
        every, first, bin0, nb = _grid_args(self.dftsize, every, first, bins)
        smooth_coefficients(decay, self.fd)                  # (raises for a decay the library would refuse)
        sp = None
        if state is not None:
            batched = (x.dim() if _is_tensor(x) else np.ndim(x)) == 2
            shape = (self.channels, nb) if batched else (nb,)
            if _is_tensor(state):
                self._check_tensor(state, "state", self.fd, shape)
                sp = state.data_ptr()
            else:
                if not isinstance(state, np.ndarray) or state.dtype != self.fd or not state.flags.c_contiguous or not state.flags.writeable:
                    raise ValueError(f"state must be a writable C-contiguous numpy array of dtype {np.dtype(self.fd).name} (it is updated in place) or a device tensor")
                if state.shape != shape:
                    raise ValueError(f"state must have shape {shape}, got {state.shape}")
                sp = state.ctypes.data
        return self._grid_call("sdft_power_smooth_n", x, every_rows, every, first, (bin0, nb, float(decay), C.c_void_p(sp)), None, nb, self.fd, out)

    def smooth_peak(self, x, decay: float, every: int = 1, first: int = 0, bins=None, hold="max", state=None, out=None):
        """Smoothed peak-hold analysis (``sdft_hip_sdft_smooth_peak_n``): :meth:`power_peak`'s grid, windows, head row, shapes and
        pointers with :meth:`power_smooth`'s sequence for the term: row r is the largest (``hold="max"`` or 0) or the smallest
        (``hold="min"`` or 1: the noise floor of minimum statistics) over the r-th window of ``s = a * s + b * p``,
        ``(a, b) = smooth_coefficients(decay, dtype)``, advanced at every sample and taken after the sample's update; ``s`` does not
        restart at a window.  ``state`` is :meth:`power_smooth`'s: a numpy array or a device tensor (whatever ``x`` is) of shape
        (nbins,) [(channels, nbins)] in the FD dtype, updated in place; ``None`` starts from zero and drops the end value.  A
        stream passes ``state`` and :func:`every_next_first` from call to call and, with ``first > 0``, joins row 0 with the
        previous call's last row by ``np.fmax`` / ``np.fmin``.  The plan's state advances over all n samples and all bins."""
        self.api.clear()
        every, first, bin0, nb = _grid_args(self.dftsize, every, first, bins)
        if hold not in HOLDS:
            raise ValueError(f"hold must be 'max' (0) or 'min' (1), got {hold!r}")
        smooth_coefficients(decay, self.fd)                  # (raises for a decay the library would refuse)
        sp = None
        if state is not None:
            batched = (x.dim() if _is_tensor(x) else np.ndim(x)) == 2
            shape = (self.channels, nb) if batched else (nb,)
            if _is_tensor(state):
                self._check_tensor(state, "state", self.fd, shape)
                sp = state.data_ptr()
            else:
                if not isinstance(state, np.ndarray) or state.dtype != self.fd or not state.flags.c_contiguous or not state.flags.writeable:
                    raise ValueError(f"state must be a writable C-contiguous numpy array of dtype {np.dtype(self.fd).name} (it is updated in place) or a device tensor")
                if state.shape != shape:
                    raise ValueError(f"state must have shape {shape}, got {state.shape}")
                sp = state.ctypes.data
        return self._grid_call("sdft_smooth_peak_n", x, power_sum_rows, every, first, (bin0, nb, float(decay), HOLDS[hold], C.c_void_p(sp)), None, nb, self.fd, out)

    def power_moments(self, x, every: int = 1, first: int = 0, bins=None, out=None):
        """Power-moments analysis (``sdft_hip_sdft_power_moments_n``): :meth:`power_sum`'s grid, windows, head row and pointers,
        with two sums per window and bin -> real array of shape (rows, nbins, 2) [(channels, rows, nbins, 2) if batched] in the FD
        dtype, numpy for numpy input, a device tensor for a device tensor.  ``[..., 0]`` is ``s1``, the sum of :meth:`power`'s
        ``every = 1`` values ``p`` over the window -- :meth:`power_sum`'s value bit for bit --, ``[..., 1]`` is ``s2``, the sum of
        ``p * p`` (rounded once, no fused multiply-add).  Sums, not means; with ``first > 0`` row 0 is the head window
        ``[0, first)`` and completes the previous call's last row (add both components); the next call's ``first`` is
        :func:`every_next_first`.  :func:`power_sum_lengths` gives the windows' lengths, :func:`power_variance` and
        :func:`spectral_kurtosis` turn the sums into statistics.  Consecutive sliding-DFT rows overlap in all but one sample: the
        kurtosis estimator keeps its unit mean for Gaussian noise, but not the variance a textbook derives for independent
        spectra, so detection thresholds have to be calibrated on the host's own noise.  The plan's state advances over all n
        samples and all bins, as with :meth:`sdft`."""
        self.api.clear()
        every, first, bin0, nb = _grid_args(self.dftsize, every, first, bins)
        flat = None
        if out is not None:
            if tuple(out.shape[-2:]) != (nb, 2):
                raise ValueError(f"out must end in the shape ({nb}, 2), got {tuple(out.shape)}")
            if not (out.is_contiguous() if _is_tensor(out) else out.flags.c_contiguous):
                raise ValueError("out must be contiguous")
            flat = out.reshape(tuple(out.shape[:-2]) + (2 * nb,))
        flat = self._grid_call("sdft_power_moments_n", x, power_sum_rows, every, first, (bin0, nb), None, 2 * nb, self.fd, flat)
        return out if out is not None else flat.reshape(tuple(flat.shape[:-1]) + (nb, 2))

    def lag_sum(self, samples, every: int, first: int = 0, band=None, out=None):
        """Lag-product analysis (``sdft_hip_sdft_lag_sum_n``): the sum of ``X[t] * conj(X[t - 1])`` over the windows
        :meth:`power_sum` cuts the n samples into, for the bins ``band = (bin0, nbins)`` (``None``: all) -> complex array of shape
        (rows, nbins) [(channels, rows, nbins)], ``rows = power_sum_rows(n, every, first)``, numpy for numpy input, a device
        tensor for a device tensor.  ``X[t]`` is the row :meth:`sdft` stores at sample t; the row before the first sample is the
        row of the plan's state: the last row of the call before (whichever entry point), the zero row of a fresh plan.
        :func:`lag_frequency` turns the sums into frequencies.  Head row, streaming and sums-not-means as with :meth:`power_sum`.
        The plan's state advances over all n samples and all bins, as with :meth:`sdft`."""
        self.api.clear()
        every, first, bin0, nb = _grid_args(self.dftsize, every, first, band, word="band")
        return self._grid_call("sdft_lag_sum_n", samples, power_sum_rows, every, first, (bin0, nb), None, nb, self.fdx, out)

    def isdft(self, dfts, out=None):
        """Synthesise samples from a DFT matrix (n, dftsize) [(channels, n, dftsize)]."""
        self.api.clear()
        batched = (len(dfts.shape) == 3)
        n = dfts.shape[-2]
        assert dfts.shape[-1] == self.dftsize and (not batched or dfts.shape[0] == self.channels)
        yshape = (self.channels, n) if batched else (n,)
        if _is_tensor(dfts):
            torch = _torch()
            self._check_tensor(dfts, "dfts", self.fdx)
            if out is None:
                out = torch.empty(yshape, dtype=getattr(torch, np.dtype(self.td).name), device=dfts.device)
            self._check_tensor(out, "out", self.td, yshape)
            self.api.isdft_n(self._p, n, C.c_void_p(dfts.data_ptr()), C.c_void_p(out.data_ptr()))
        else:
            dfts = np.ascontiguousarray(dfts, dtype=self.fdx)
            if out is None:
                out = np.empty(yshape, dtype=self.td)
            assert out.flags.c_contiguous and out.shape == yshape and out.dtype == self.td
            self.api.isdft_n(self._p, n, C.c_void_p(dfts.ctypes.data), C.c_void_p(out.ctypes.data))
        self.api.check()
        return out


    def process(self, x, op="identity", gain=None, shift=0, out=None, dfts=None, hop=0, threshold=0.0, floor=0.0,
                exponent=1.0, scale=1.0, expr=None, expr_params=()):
        """Fused analysis -> spectral operation -> synthesis (``sdft_hip_process_n``): returns the
        processed samples; the DFT matrix is not materialised unless ``dfts`` (a CUDA tensor of shape
        (n, dftsize) [(channels, n, dftsize)]) asks for a copy of the processed spectrum.

        ``op``: "identity", "gain" (``gain`` = real array of dftsize factors), "cgain" (``gain`` = complex array),
        "shift" (``shift`` bins), "gain_rows" / "cgain_rows" (``gain`` = (rows, dftsize) array, row r for the call's samples
        [r*hop, (r+1)*hop), the last row for the rest), "gate" (``threshold``, ``floor``), "power" (``exponent``, ``scale``) or
        "expr" (``expr`` = HIP C++ statements on ``re``, ``im`` of bin ``k`` at sample ``t`` of channel ``ch`` with the
        parameters ``p[i]`` = ``expr_params``; compiled into the kernel at run time, see sdft_hip.h).
        """
        self.api.clear()
        kind = OPS[op] if isinstance(op, str) else int(op)
        params = None
        keep = None
        if kind in (OPS["gain_rows"], OPS["cgain_rows"]):
            gdt = self.fd if kind == OPS["gain_rows"] else self.fdx
            if _is_tensor(gain):
                assert gain.dim() == 2 and gain.shape[1] == self.dftsize
                self._check_tensor(gain, "gain", gdt)
                gptr, rows = gain.data_ptr(), int(gain.shape[0])
                keep_rows = gain
            else:
                keep_rows = np.ascontiguousarray(gain, dtype=gdt)
                assert keep_rows.ndim == 2 and keep_rows.shape[1] == self.dftsize
                gptr, rows = keep_rows.ctypes.data, int(keep_rows.shape[0])

            class _Table(C.Structure):
                _fields_ = [("gains", C.c_void_p), ("rows", C.c_size_t), ("hop", C.c_size_t)]
            keep = (_Table(gptr, rows, int(hop)), keep_rows)
            params = C.cast(C.byref(keep[0]), C.c_void_p)
        elif kind == OPS["expr"]:
            pv = np.ascontiguousarray(expr_params, dtype=self.fd).reshape(-1)
            text = C.c_char_p(str(expr).encode())

            class _Expr(C.Structure):
                _fields_ = [("expr", C.c_char_p), ("params", C.c_void_p), ("nparams", C.c_size_t)]
            keep = (_Expr(text, pv.ctypes.data if pv.size else None, int(pv.size)), pv, text)
            params = C.cast(C.byref(keep[0]), C.c_void_p)
        elif kind in (OPS["gate"], OPS["power"]):
            vals = (threshold, floor) if kind == OPS["gate"] else (exponent, scale)
            keep = np.asarray(vals, dtype=self.fd)
            params = C.c_void_p(keep.ctypes.data)
        elif kind in (OPS["gain"], OPS["cgain"]):
            gdt = self.fd if kind == OPS["gain"] else self.fdx
            if _is_tensor(gain):
                self._check_tensor(gain, "gain", gdt, (self.dftsize,))
                params = C.c_void_p(gain.data_ptr())
            else:
                keep = np.ascontiguousarray(gain, dtype=gdt)
                assert keep.shape == (self.dftsize,)
                params = C.c_void_p(keep.ctypes.data)
        elif kind == OPS["shift"]:
            keep = C.c_long(int(shift))
            params = C.cast(C.byref(keep), C.c_void_p)
        dptr = None
        if _is_tensor(x):
            torch = _torch()
            n = self._shape_x(x.shape)
            self._check_tensor(x, "samples", self.td)
            if out is None:
                out = torch.empty_like(x)
            self._check_tensor(out, "out", self.td, tuple(x.shape))
            if dfts is not None:
                self._check_tensor(dfts, "dfts", self.fdx, (n, self.dftsize) if x.dim() == 1 else (self.channels, n, self.dftsize))
                dptr = C.c_void_p(dfts.data_ptr())
            rc = self.api.process_n(self._p, n, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), kind, params, dptr)
        else:
            x = np.ascontiguousarray(x, dtype=self.td)
            n = self._shape_x(x.shape)
            if out is None:
                out = np.empty_like(x)
            assert out.flags.c_contiguous and out.shape == x.shape and out.dtype == self.td
            if dfts is not None:
                self._check_tensor(dfts, "dfts", self.fdx)
                dptr = C.c_void_p(dfts.data_ptr())
            rc = self.api.process_n(self._p, n, C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data), kind, params, dptr)
        if rc != 0:
            self.api.check()
            raise SdftHipError("sdft_hip_process_n failed")
        self.api.check()
        return out


def every_rows(n: int, every: int, first: int) -> int:
    """Rows a decimated analysis call of n samples keeps (sdft_hip_sdft_every_n)."""
    return (n - first + every - 1) // every if first < n else 0


def power_sum_rows(n: int, every: int, first: int) -> int:
    """Rows a pooled power analysis call of n samples writes (sdft_hip_sdft_power_sum_n): the head window, if any, and one row per
    grid point."""
    return (1 if first > 0 and n > 0 else 0) + every_rows(n, every, first)


def power_sum_lengths(n: int, every: int, first: int):
    """The window lengths of the rows a pooled call of n samples writes (:meth:`SDFT.power_sum`, :meth:`SDFT.power_moments` and
    their siblings), as an int64 array of ``power_sum_rows(n, every, first)`` entries: the head window ``[0, first)`` if
    ``first > 0``, then one window of at most ``every`` samples per grid point, the last one ending with the call."""
    n, every, first = int(n), int(every), int(first)
    if every < 1 or first < 0 or n < 0:
        raise ValueError(f"every must be >= 1, first >= 0 and n >= 0, got n={n}, every={every}, first={first}")
    head = [min(first, n)] if first > 0 and n > 0 else []
    starts = np.arange(first, n, every, dtype=np.int64) if first < n else np.zeros(0, dtype=np.int64)
    return np.concatenate([np.asarray(head, dtype=np.int64), np.minimum(starts + every, n) - starts])


def _moments(moments, lengths):
    """(s1, s2, L) of :meth:`SDFT.power_moments`' output in float64, L shaped to broadcast against (..., rows, nbins)."""
    if _is_tensor(moments):
        moments = moments.detach().cpu().numpy()
    m = np.asarray(moments).astype(np.float64)
    if m.ndim < 3 or m.shape[-1] != 2:
        raise ValueError(f"moments must be (..., rows, nbins, 2), got {m.shape}")
    length = np.asarray(lengths, dtype=np.float64)
    if length.ndim <= 1:
        length = length.reshape(-1, 1)                       # one length per row (or one for all): over bins and channels
    return m[..., 0], m[..., 1], length


def power_variance(moments, lengths):
    """The variance of the power per window and bin from :meth:`SDFT.power_moments`' sums: ``s2 / L - (s1 / L)**2``, in float64
    (numpy; a device tensor is copied).  ``lengths`` holds one window length per row (:func:`power_sum_lengths`) and broadcasts
    over bins and channels; rows that a stream cut are added by the caller first."""
    s1, s2, length = _moments(moments, lengths)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = s1 / length
        return s2 / length - mean * mean


def spectral_kurtosis(moments, lengths):
    """The spectral kurtosis estimator per window and bin from :meth:`SDFT.power_moments`' sums:
    ``(L + 1) / (L - 1) * (L * s2 / s1**2 - 1)``, in float64 (numpy; a device tensor is copied); NaN where ``L < 2`` or
    ``s1 == 0``.  ``lengths`` holds one window length per row (:func:`power_sum_lengths`) and broadcasts over bins and channels;
    rows that a stream cut are added by the caller first.  Its mean is 1 for Gaussian noise.  Consecutive sliding-DFT rows
    overlap in all but one sample, so the estimator's textbook variance, which assumes independent spectra, does NOT hold:
    calibrate detection thresholds on the host's own noise."""
    s1, s2, length = _moments(moments, lengths)
    with np.errstate(divide="ignore", invalid="ignore"):
        sk = (length + 1.0) / (length - 1.0) * (length * s2 / (s1 * s1) - 1.0)
    return np.where((length < 2) | (s1 == 0), np.nan, sk)


def smooth_coefficients(decay: float, dtype):
    """``(a, b)`` of :meth:`SDFT.power_smooth` as numbers of ``dtype`` (the plan's real type): ``a = dtype(decay)`` and
    ``b = dtype(1) - a``.  Raises ValueError for a decay the library refuses: NaN, negative, or 1 or more after rounding."""
    t = np.dtype(dtype).type
    a = t(decay)
    if not (a >= t(0) and a < t(1)):
        raise ValueError(f"decay must be at least 0 and less than 1 after rounding to {np.dtype(dtype).name}, got {decay!r}")
    return a, t(1) - a


def smooth_decay(time_constant_samples: float) -> float:
    """The decay of a time constant of that many samples: ``exp(-1 / tau)`` (after tau samples a step has reached 1 - 1/e)."""
    tau = float(time_constant_samples)
    if not tau > 0:
        raise ValueError(f"the time constant must be positive, got {time_constant_samples!r}")
    return float(np.exp(-1.0 / tau))


def coherence(s_ab, s_aa, s_bb):
    """The magnitude-squared coherence of :meth:`SDFT.cross_smooth`'s averages: ``|s_ab|**2 / (s_aa * s_bb)`` with the real parts
    of the auto-spectra ``s_aa`` and ``s_bb`` (the rows of the pairs ``(a, a)`` and ``(b, b)``; real arrays are taken as they
    are), in float64; NaN where ``s_aa * s_bb`` is 0.  Takes numpy arrays or tensors (which are copied to the host).  Between 0
    and 1 up to rounding for averages of one call with one decay."""
    def host(v):
        return np.asarray(v.detach().cpu().numpy() if _is_tensor(v) else v)
    ab = host(s_ab).astype(np.complex128)
    aa, bb = (host(v).real.astype(np.float64) for v in (s_aa, s_bb))
    den = aa * bb
    with np.errstate(divide="ignore", invalid="ignore"):
        c = (ab.real * ab.real + ab.imag * ab.imag) / den
    return np.where(den == 0, np.nan, c)


HOLDS = {"max": 0, "min": 1, 0: 0, 1: 1}                     # SDFT.power_peak's hold -> enum sdft_hip_hold


def lag_frequency(sums, samplerate: float = 1.0):
    """The frequency estimate of :meth:`SDFT.lag_sum`'s sums: ``angle(sums) / (2 pi) * samplerate``, the power-weighted mean
    frequency of each bin over its window (the pulse-pair estimator; with one sample per row the angle needs no unwrapping), in
    ``(-samplerate / 2, samplerate / 2]``; ``nan`` where the sum is 0, whose angle says nothing.  Takes a numpy array or a
    tensor (which is copied to the host) and returns a float64 numpy array of the same shape."""
    if _is_tensor(sums):
        sums = sums.detach().cpu().numpy()
    z = np.asarray(sums).astype(np.complex128)
    f = np.angle(z) / (2.0 * np.pi) * float(samplerate)
    return np.where(z == 0, np.nan, f)


def covariance_pairs(nch: int):
    """The upper triangle of an array of ``nch`` elements as a pair list ``(a, b)`` of array INDICES in the order of
    :meth:`SDFT.covariance`'s output: ``(0, 0), (0, 1), ... (0, nch - 1), (1, 1), ...``.  With the array's channel list ``chan``,
    ``set_pairs(chan[a], chan[b])`` makes :meth:`SDFT.cross_sum` return the same elements."""
    nch = int(nch)
    a = np.array([i for i in range(nch) for _ in range(i, nch)], dtype=np.uint64)
    b = np.array([j for i in range(nch) for j in range(i, nch)], dtype=np.uint64)
    return a, b


def covariance_matrix(cov, nch: int):
    """Expands :meth:`SDFT.covariance`'s (T, rows, nbins) upper triangle to Hermitian matrices of shape (rows, nbins, nch, nch) on the
    host (numpy; a device tensor is copied): ``[r, k, i, j]`` is the sum of ``X_chan[i] * conj(X_chan[j])``, the lower triangle the
    conjugate of the upper.  Plumbing only."""
    nch = int(nch)
    c = cov.detach().cpu().numpy() if _is_tensor(cov) else np.asarray(cov)
    if c.ndim != 3 or c.shape[0] != nch * (nch + 1) // 2:
        raise ValueError(f"cov must be (nch (nch + 1) / 2, rows, nbins) for nch = {nch}, got {c.shape}")
    a, b = covariance_pairs(nch)
    a, b = a.astype(np.intp), b.astype(np.intp)
    m = np.empty(c.shape[1:] + (nch, nch), dtype=c.dtype)
    m[:, :, b, a] = np.conj(np.moveaxis(c, 0, -1))
    m[:, :, a, b] = np.moveaxis(c, 0, -1)                        # (the diagonal last: as returned, im == +0)
    return m


def mvdr_weights(mat, steering, loading: float = 0.0):
    """MVDR weights per bin from :func:`covariance_matrix`'s output, shaped for :meth:`SDFT.set_mix` (numpy, on the host).
    ``mat`` is (rows, nbins, nch, nch), or one row of it (nbins, nch, nch); a stack of rows is summed first.  ``steering`` is the
    steering vector d per bin, (nbins, nch) or (nch,) for all bins.  ``loading`` adds ``loading * trace(R) / nch`` to R's diagonal.
    Returns ``conj(R^-1 d / (d^H R^-1 d))`` of shape (1, nch, nbins), so that :meth:`SDFT.mix` yields ``w^H x`` with ``w^H d = 1``."""
    r = np.asarray(mat)
    if r.ndim == 4:
        r = r.sum(axis=0)
    if r.ndim != 3 or r.shape[1] != r.shape[2]:
        raise ValueError(f"mat must be (rows, nbins, nch, nch) or (nbins, nch, nch), got {np.asarray(mat).shape}")
    nbins, nch = r.shape[0], r.shape[1]
    d = np.asarray(steering)
    if d.ndim == 1:
        d = np.broadcast_to(d, (nbins, d.shape[0]))
    if d.shape != (nbins, nch):
        raise ValueError(f"steering must be ({nbins}, {nch}) or ({nch},), got {np.asarray(steering).shape}")
    cdtype = np.result_type(r.dtype, np.complex64)
    r = r.astype(cdtype)
    d = d.astype(cdtype)
    if loading:
        r = r + (float(loading) * np.trace(r, axis1=1, axis2=2).real / nch)[:, None, None] * np.eye(nch, dtype=cdtype)
    rid = np.linalg.solve(r, d[:, :, None])[:, :, 0]                     # R^-1 d per bin
    den = np.einsum("kc,kc->k", np.conj(d), rid)                          # d^H R^-1 d
    w = rid / den[:, None]
    return np.ascontiguousarray(np.conj(w).T[None])


def band_peak_split(peaks):
    """``(values, bins)`` of :meth:`SDFT.band_peak`'s array: ``peaks[..., 0]`` as it is and ``peaks[..., 1]`` as int64 (the bins are
    stored as exactly representable integers of the plan's real type).  numpy in, numpy out; device tensors likewise."""
    if _is_tensor(peaks):
        return peaks[..., 0], peaks[..., 1].to(_torch().int64)
    peaks = np.asarray(peaks)
    return peaks[..., 0], peaks[..., 1].astype(np.int64)


def every_next_first(n: int, every: int, first: int) -> int:
    """The ``first`` of the next call when a stream is analysed in calls of any length on one row grid."""
    rows = every_rows(n, every, first)
    return first + rows * every - n if rows else first - n


def plan_tables(dftsize: int, latency: float = 1.0, combo: str = "f32f64"):
    """Host-only: (tw, syn, wtab, weights) exactly as the library uploads them (no GPU needed)."""
    api = Api(combo)
    fd, fdx = _NP_REAL[combo[3:]], _NP_CPLX[combo[3:]]
    tw = np.empty(dftsize, dtype=fdx)
    syn = np.empty(dftsize, dtype=fdx)
    wtab = np.empty(2 * dftsize, dtype=fdx)
    w = np.empty(2, dtype=fd)
    api.plan_tables(dftsize, latency, tw.ctypes.data, syn.ctypes.data, wtab.ctypes.data, w.ctypes.data)
    return tw, syn, wtab, w


def check_expr(expr: str, arch: str | None = None) -> None:
    """Compiles the statements of an ``op="expr"`` operation without running them (``sdft_hip_check_expr``; needs no GPU).
    Raises :class:`SdftHipError` with the compiler's words when they do not compile."""
    from . import capi
    lib = capi.load()
    lib.sdft_hip_clear_error()
    if lib.sdft_hip_check_expr(str(expr).encode(), arch.encode() if arch else None) != 0:
        e = lib.sdft_hip_last_error()
        lib.sdft_hip_clear_error()
        raise SdftHipError(e.decode() if e else "the expression does not compile")
