"""Channel-mix analysis (sdft_hip_set_mix, sdft_hip_mix_outputs, sdft_hip_sdft_mix_n) without a GPU: the symbols of every type
pair, the declarations, the NULL-plan errors, the host-side logic (accepted mixes, the table of items for every block size, one
writer per channel, route; tests/cpp/mix_logic_test.cpp under g++ -fsanitize=address,undefined), the MVDR helper of the Python
module and the kernel's instantiations in every translation unit's gfx950 code object."""

import os
import shutil
import subprocess

import numpy as np
import pytest

from test_capi_cpu import disassemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdft_amd", "csrc")
COMBOS = ("f32f64", "f32f32", "f64f64", "f64f32")
SYMBOLS = ("set_mix", "mix_outputs", "sdft_mix_n")
GROUP_BLOCK = {"double": (4, 4), "float": (4, 4)}           # mix_group<FD>, mix_block<FD>: the one pair the product library holds per FD type


def test_mix_symbols_exported_for_all_type_pairs(hip_library):
    from sdft_amd import capi
    lib = capi.load()
    for combo in COMBOS:
        for name in SYMBOLS:
            assert hasattr(lib, f"sdft_hip_{name}_{combo}"), (combo, name)
            assert name in capi.typed_signatures(combo)


def test_mix_declared_in_the_headers():
    with open(os.path.join(ROOT, "include", "sdft", "sdft_hip.h")) as fh:
        c_header = fh.read()
    with open(os.path.join(ROOT, "include", "sdft", "sdft.hpp")) as fh:
        cpp_header = fh.read()
    for name in SYMBOLS:
        assert f"sdft_hip_{name}(" in c_header and f"SDFT_HIP_SYMBOL({name})" in c_header, name
        assert f"sdft_hip_{name}_##SUF" in cpp_header, name
    assert '("last_kernel" = 10)' in c_header and "10 channel-mix analysis" in c_header
    for method in ("void set_mix(", "std::size_t mix_outputs() const", "std::size_t mix("):
        assert method in cpp_header, method


@pytest.mark.parametrize("combo", COMBOS)
def test_mix_null_plan_returns_minus_one(hip_library, combo):
    from sdft_amd import capi
    api = capi.Api(combo)
    api.clear()
    assert api.sdft_mix_n(None, 100, None, 10, 0, 0, 1, None) == -1
    err = api.last_error()
    assert err and "sdft_hip_sdft_mix_n" in err and "NULL plan" in err, err
    api.clear()
    assert api.set_mix(None, 0, 0, None, None) == -1
    err = api.last_error()
    assert err and "sdft_hip_set_mix" in err and "NULL plan" in err, err
    api.clear()
    assert api.mix_outputs(None) == 0 and api.last_error() is None


def test_mix_logic_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ on this host")
    exe = str(tmp_path / "mix_logic_test")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
           f"-I{CSRC}", os.path.join(ROOT, "tests", "cpp", "mix_logic_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "mix-logic: all properties hold" in r.stdout


def hermitian_pd(rng, shape, nch):
    a = rng.standard_normal(shape + (nch, 2 * nch)) + 1j * rng.standard_normal(shape + (nch, 2 * nch))
    return a @ np.conj(np.swapaxes(a, -1, -2)) + 0.1 * np.eye(nch)


def test_mvdr_weights():
    """w^H d = 1 per bin on random Hermitian positive-definite matrices, the shape set_mix takes, the minimum-variance property
    against a perturbed weight of the same constraint, rows summed, diagonal loading, shape errors"""
    from sdft_amd.sdft import mvdr_weights
    rng = np.random.default_rng(5)
    for nch, nbins in ((1, 3), (2, 5), (4, 16), (9, 7)):
        R = hermitian_pd(rng, (nbins,), nch)
        d = rng.standard_normal((nbins, nch)) + 1j * rng.standard_normal((nbins, nch))
        for loading in (0.0, 1e-3):
            w = mvdr_weights(R, d, loading)
            assert w.shape == (1, nch, nbins) and w.dtype == np.complex128 and w.flags.c_contiguous
            wh = w[0].T                                      # w^H per bin: the mix applies the weights as written
            assert np.abs(np.einsum("kc,kc->k", wh, d) - 1).max() <= 1e-12, (nch, nbins, loading)
        # minimum variance: any other weight with v^H d = 1 has v^H R v >= w^H R w
        w = np.conj(mvdr_weights(R, d)[0].T)
        var = np.einsum("kc,kcd,kd->k", np.conj(w), R, w).real
        v = w + 0.1 * (rng.standard_normal(w.shape) + 1j * rng.standard_normal(w.shape))
        v = v / np.conj(np.einsum("kc,kc->k", np.conj(v), d))[:, None]
        assert np.abs(np.einsum("kc,kc->k", np.conj(v), d) - 1).max() <= 1e-12
        assert (np.einsum("kc,kcd,kd->k", np.conj(v), R, v).real >= var * (1 - 1e-12)).all()
        # a stack of rows is summed; one steering vector serves all bins
        rows = hermitian_pd(rng, (3, nbins), nch)
        assert np.allclose(mvdr_weights(rows, d), mvdr_weights(rows.sum(axis=0), d), rtol=1e-13, atol=0)
        assert np.allclose(mvdr_weights(R, d[0]), mvdr_weights(R, np.broadcast_to(d[0], (nbins, nch))), rtol=1e-13, atol=0)
    R = hermitian_pd(rng, (4,), 3)
    for bad_mat, bad_d in ((R[0], np.ones(3)), (np.zeros((4, 3, 2)), np.ones(3)), (R, np.ones(2)), (R, np.ones((3, 3))), (R, np.ones((4, 3, 1)))):
        with pytest.raises(ValueError):
            mvdr_weights(bad_mat, bad_d)


@pytest.mark.parametrize("combo", COMBOS)
def test_mix_kernel_instantiations_in_code_object(hip_library, combo):
    """The four window instantiations of forward_mix_kernel, at the type pair's one bins-per-lane and the FD type's one group and
    block size, are in the translation unit's gfx950 code object (names only; the other candidates exist in the hooks build alone)."""
    kernels = disassemble(combo, hip_library)
    fd = "double" if combo.endswith("f64") else "float"
    bpl = 1 if fd == "double" else 2
    g, o = GROUP_BLOCK[fd]
    found = {name for name in kernels if name.startswith("forward_mix_kernel")}
    assert found == {f"forward_mix_kernel<{fd}, {bpl}, {w}, {g}, {o}>" for w in range(4)}, sorted(found)
