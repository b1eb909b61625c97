"""Filterbank analysis (sdft_hip_set_filterbank, sdft_hip_filterbank_bands, sdft_hip_sdft_filterbank_n) without a GPU: the symbols
of every type pair, the NULL-plan answers, the host-side logic (validation, the pieces of a filterbank for a plan's tiles,
workspace slots, row segments, the route; tests/cpp/filterbank_logic_test.cpp under g++ -fsanitize=address,undefined), the kernels'
instantiations in every translation unit's gfx950 code object, and the numpy builders of sdft_amd.filterbank."""

import os
import shutil
import subprocess

import numpy as np
import pytest

from test_capi_cpu import disassemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdft_amd", "csrc")
COMBOS = ("f32f64", "f32f32", "f64f64", "f64f32")
NAMES = ("set_filterbank", "filterbank_bands", "sdft_filterbank_n")


def test_filterbank_symbols_exported_for_all_type_pairs(hip_library):
    from sdft_amd import capi
    lib = capi.load()
    for combo in COMBOS:
        for name in NAMES:
            assert hasattr(lib, f"sdft_hip_{name}_{combo}"), (name, combo)
            assert name in capi.typed_signatures(combo)


@pytest.mark.parametrize("combo", COMBOS)
def test_filterbank_null_plan(hip_library, combo):
    from sdft_amd import capi
    api = capi.Api(combo)
    api.clear()
    assert api.sdft_filterbank_n(None, 100, None, 10, 0, None) == -1
    err = api.last_error()
    assert err and "sdft_hip_sdft_filterbank_n" in err and "NULL plan" in err, err
    api.clear()
    assert api.set_filterbank(None, 0, None, None, None) == -1
    err = api.last_error()
    assert err and "sdft_hip_set_filterbank" in err and "NULL plan" in err, err
    api.clear()
    assert api.filterbank_bands(None) == 0
    assert api.last_error() is None
    api.clear()


def test_filterbank_logic_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ on this host")
    exe = str(tmp_path / "filterbank_logic_test")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
           f"-I{CSRC}", os.path.join(ROOT, "tests", "cpp", "filterbank_logic_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "all properties hold" in r.stdout


@pytest.mark.parametrize("combo", COMBOS)
def test_filterbank_kernel_instantiations_in_code_object(hip_library, combo):
    """The four window instantiations of forward_filterbank_kernel, at the type pair's one bins-per-lane, and
    filterbank_rows_kernel are in the translation unit's gfx950 code object (names only)."""
    kernels = disassemble(combo, hip_library)
    fd = "double" if combo.endswith("f64") else "float"
    bpl = 1 if fd == "double" else 2
    found = {name for name in kernels if name.startswith(("forward_filterbank_kernel", "filterbank_rows_kernel"))}
    assert found == {f"forward_filterbank_kernel<{fd}, {bpl}, {w}>" for w in range(4)} | {f"filterbank_rows_kernel<{fd}>"}, sorted(found)


# ---- sdft_amd.filterbank ---------------------------------------------------------------------------------------------------

def _supports_ok(dftsize, bin0, nbins, weights):
    assert bin0.dtype == np.uint64 and nbins.dtype == np.uint64 and bin0.shape == nbins.shape and bin0.ndim == 1
    assert weights.ndim == 1 and weights.size == int(nbins.sum())
    assert (nbins >= 1).all(), "a band without bins was kept"
    assert (bin0.astype(np.int64) + nbins.astype(np.int64) <= dftsize).all()


@pytest.mark.parametrize("dftsize,samplerate,nbands,fmin,fmax", [(1024, 48000, 80, 0.0, None), (4096, 48000, 128, 0.0, None), (1024, 16000, 40, 60.0, 7600.0),
                                                              (64, 48000, 40, 0.0, None), (125, 44100, 20, 100.0, 20000.0), (1000, 8000, 23, 0.0, 3700.0)])
def test_mel_filterbank(dftsize, samplerate, nbands, fmin, fmax):
    from sdft_amd import filterbank as F
    bin0, nbins, weights = F.mel(dftsize, samplerate, nbands, fmin, fmax)
    _supports_ok(dftsize, bin0, nbins, weights)
    assert 1 <= bin0.size <= nbands
    assert (weights >= 0).all() and (weights <= 1).all()
    assert (weights > 0).all(), "a band's support is where its triangle is positive"
    # between the first and the last centre adjacent triangles sum to 1 at every bin
    top = samplerate / 2.0 if fmax is None else fmax
    corners = F.mel_to_hz(np.linspace(F.hz_to_mel(fmin), F.hz_to_mel(top), nbands + 2))
    f = F.bin_frequencies(dftsize, samplerate)
    inside = (f >= corners[1]) & (f <= corners[nbands])
    total = F.dense(dftsize, bin0, nbins, weights).sum(axis=0)
    assert inside.any() or nbands == 1
    np.testing.assert_allclose(total[inside], 1.0, rtol=0, atol=1e-12)
    # outside the first and last corner nothing
    assert (total[(f <= corners[0]) | (f >= corners[-1])] == 0).all()
    # ascending centres: the supports start in ascending order
    assert (np.diff(bin0.astype(np.int64)) >= 0).all()


def test_mel_drops_bands_without_bins():
    from sdft_amd import filterbank as F
    # 40 triangles on 16 bins: the low ones are narrower than the bin spacing
    bin0, nbins, weights = F.mel(16, 48000, 40)
    _supports_ok(16, bin0, nbins, weights)
    assert bin0.size < 40


@pytest.mark.parametrize("dftsize,samplerate,fraction,fmin", [(1024, 48000, 3, 20.0), (4096, 48000, 3, 20.0), (1024, 48000, 1, 31.25), (125, 8000, 12, 100.0), (64, 48000, 3, 20.0)])
def test_fractional_octave_filterbank(dftsize, samplerate, fraction, fmin):
    from sdft_amd import filterbank as F
    bin0, nbins, weights = F.fractional_octave(dftsize, samplerate, fraction, fmin)
    _supports_ok(dftsize, bin0, nbins, weights)
    assert bin0.size >= 1
    assert (weights == 1).all()
    b0, nb = bin0.astype(np.int64), nbins.astype(np.int64)
    assert (b0[1:] >= b0[:-1] + nb[:-1]).all(), "disjoint and ascending"
    f = F.bin_frequencies(dftsize, samplerate)
    # every bin from fmin up lies in exactly one band, none below it in any
    total = F.dense(dftsize, bin0, nbins, weights).sum(axis=0)
    assert (total[f >= fmin] == 1).all() and (total[f < fmin] == 0).all()
    # a band spans less than 1 / fraction octave
    lo, hi = f[b0], f[b0 + nb - 1]
    assert (hi < lo * 2.0 ** (1.0 / fraction) * (1 + 1e-12)).all()


def test_dense_matrix_of_a_filterbank():
    from sdft_amd import filterbank as F
    W = F.dense(6, [1, 0, 1], [2, 6, 2], np.arange(10, dtype=np.float64) + 1)
    assert W.shape == (3, 6)
    np.testing.assert_array_equal(W[0], [0, 1, 2, 0, 0, 0])
    np.testing.assert_array_equal(W[1], [3, 4, 5, 6, 7, 8])
    np.testing.assert_array_equal(W[2], [0, 9, 10, 0, 0, 0])
