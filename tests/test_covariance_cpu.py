"""Array covariance analysis (sdft_hip_set_array, sdft_hip_array_channels, sdft_hip_sdft_covariance_n) without a GPU: the symbols of
every type pair, the declarations, the NULL-plan errors, the host-side logic (accepted arrays, the index formula, the table of block
items for every group size, one writer per channel, workspace, route; tests/cpp/covariance_logic_test.cpp under
g++ -fsanitize=address,undefined), the host helpers of the Python module and the kernel's instantiations in every translation
unit's gfx950 code object."""

import os
import shutil
import subprocess

import numpy as np
import pytest

from test_capi_cpu import disassemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdft_amd", "csrc")
COMBOS = ("f32f64", "f32f32", "f64f64", "f64f32")
SYMBOLS = ("set_array", "array_channels", "sdft_covariance_n")
GROUP = {"double": 4, "float": 4}                           # cov_group<FD>: the one group size the product library holds per FD type


def test_covariance_symbols_exported_for_all_type_pairs(hip_library):
    from sdft_amd import capi
    lib = capi.load()
    for combo in COMBOS:
        for name in SYMBOLS:
            assert hasattr(lib, f"sdft_hip_{name}_{combo}"), (combo, name)
            assert name in capi.typed_signatures(combo)


def test_covariance_declared_in_the_headers():
    with open(os.path.join(ROOT, "include", "sdft", "sdft_hip.h")) as fh:
        c_header = fh.read()
    with open(os.path.join(ROOT, "include", "sdft", "sdft.hpp")) as fh:
        cpp_header = fh.read()
    for name in SYMBOLS:
        assert f"sdft_hip_{name}(" in c_header and f"SDFT_HIP_SYMBOL({name})" in c_header, name
        assert f"sdft_hip_{name}_##SUF" in cpp_header, name
    assert '("last_kernel" = 9)' in c_header and "9 array covariance analysis" in c_header


@pytest.mark.parametrize("combo", COMBOS)
def test_covariance_null_plan_returns_minus_one(hip_library, combo):
    from sdft_amd import capi
    api = capi.Api(combo)
    api.clear()
    assert api.sdft_covariance_n(None, 100, None, 10, 0, 0, 1, None) == -1
    err = api.last_error()
    assert err and "sdft_hip_sdft_covariance_n" in err and "NULL plan" in err, err
    api.clear()
    assert api.set_array(None, 0, None) == -1
    err = api.last_error()
    assert err and "sdft_hip_set_array" in err and "NULL plan" in err, err
    api.clear()
    assert api.array_channels(None) == 0 and api.last_error() is None


def test_covariance_logic_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ on this host")
    exe = str(tmp_path / "covariance_logic_test")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
           f"-I{CSRC}", os.path.join(ROOT, "tests", "cpp", "covariance_logic_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "covariance-logic: all properties hold" in r.stdout


def test_covariance_pairs_and_matrix_helpers():
    """covariance_pairs is the upper triangle in the output's order (the index formula of the header); covariance_matrix puts
    element p(i, j) at [i, j] and its conjugate at [j, i], and leaves the diagonal as returned."""
    from sdft_amd.sdft import covariance_matrix, covariance_pairs
    for nch in (1, 2, 3, 5, 9):
        a, b = covariance_pairs(nch)
        assert len(a) == len(b) == nch * (nch + 1) // 2
        for p, (i, j) in enumerate(zip(a.tolist(), b.tolist())):
            assert i <= j < nch and p == i * nch - i * (i - 1) // 2 + (j - i), (nch, p, i, j)
        rows, nb = 2, 3
        rng = np.random.default_rng(nch)
        cov = (rng.standard_normal((len(a), rows, nb)) + 1j * rng.standard_normal((len(a), rows, nb))).astype(np.complex128)
        cov[a == b] = cov[a == b].real                       # (the diagonal elements are real)
        m = covariance_matrix(cov, nch)
        assert m.shape == (rows, nb, nch, nch)
        for p, (i, j) in enumerate(zip(a.tolist(), b.tolist())):
            assert np.array_equal(m[:, :, i, j], cov[p]) and np.array_equal(m[:, :, j, i], np.conj(cov[p]) if i != j else cov[p])
        assert np.array_equal(m, np.conj(np.swapaxes(m, -1, -2)))
    with pytest.raises(ValueError):
        covariance_matrix(np.zeros((4, 1, 1), dtype=np.complex64), 3)


@pytest.mark.parametrize("combo", COMBOS)
def test_covariance_kernel_instantiations_in_code_object(hip_library, combo):
    """The four window instantiations of forward_covariance_kernel, at the type pair's one bins-per-lane and the FD type's one group
    size, are in the translation unit's gfx950 code object (names only; the other group sizes exist in the hooks build alone); the
    kernels that add the pieces of cut windows are the pooled power call's."""
    kernels = disassemble(combo, hip_library)
    fd = "double" if combo.endswith("f64") else "float"
    bpl = 1 if fd == "double" else 2
    found = {name for name in kernels if name.startswith("forward_covariance_kernel")}
    assert found == {f"forward_covariance_kernel<{fd}, {bpl}, {w}, {GROUP[fd]}>" for w in range(4)}, sorted(found)
    for helper in ("pooled_power_rows_kernel", "pooled_power_add_kernel"):
        assert any(name.startswith(f"{helper}<{fd}>") for name in kernels), (helper, sorted(k for k in kernels if "pooled" in k))
