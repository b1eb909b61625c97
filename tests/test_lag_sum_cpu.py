"""Lag-product analysis (sdft_hip_sdft_lag_sum_n) without a GPU: the symbol of every type pair, the NULL-plan error, the
declarations in the headers, the argument checks of SDFT.lag_sum that need no plan, lag_frequency on hand-made sums, the host-side
logic (kernel id, route flags and time chunks, workspace, staging bounds, row counts and the next first;
tests/cpp/lag_sum_logic_test.cpp under g++ -fsanitize=address,undefined) and the kernel's instantiations in every translation
unit's gfx950 code object, beside unchanged sets of the pooled-power and cross-spectrum kernels."""

import os
import shutil
import subprocess

import numpy as np
import pytest

from test_capi_cpu import disassemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdft_amd", "csrc")
COMBOS = ("f32f64", "f32f32", "f64f64", "f64f32")


def test_lag_sum_symbol_exported_for_all_type_pairs(hip_library):
    from sdft_amd import capi
    lib = capi.load()
    for combo in COMBOS:
        assert hasattr(lib, f"sdft_hip_sdft_lag_sum_n_{combo}"), combo
        assert "sdft_lag_sum_n" in capi.typed_signatures(combo)
        assert capi.typed_signatures(combo)["sdft_lag_sum_n"] == capi.typed_signatures(combo)["sdft_cross_sum_n"]


@pytest.mark.parametrize("combo", COMBOS)
def test_lag_sum_null_plan_returns_minus_one(hip_library, combo):
    from sdft_amd import capi
    api = capi.Api(combo)
    api.clear()
    assert api.sdft_lag_sum_n(None, 100, None, 10, 0, 0, 1, None) == -1
    err = api.last_error()
    assert err and "sdft_hip_sdft_lag_sum_n" in err and "NULL plan" in err, err
    api.clear()


def test_lag_sum_bad_arguments_are_refused_by_the_python_call(hip_library):
    """SDFT.lag_sum refuses every < 1, first < 0 and a band outside the plan's bins before the plan is touched (the C call's own
    refusals need a plan, hence a GPU: tests/test_gpu_lag_sum.py)"""
    from sdft_amd import sdft as S

    class NoPlan:
        dftsize = 8

        class api:
            @staticmethod
            def clear():
                pass

    for kw in (dict(every=0), dict(every=1, first=-1), dict(every=1, band=(0, 0)), dict(every=1, band=(8, 1)), dict(every=1, band=(1, 8)),
               dict(every=1, band=(-1, 2))):
        with pytest.raises(ValueError):
            S.SDFT.lag_sum(NoPlan(), [0.0] * 4, **kw)


def test_lag_frequency_on_hand_made_sums():
    from sdft_amd.sdft import lag_frequency
    z = np.array([[1 + 0j, 1j, -1j, -1 + 0j], [1 + 1j, 0j, 2 - 2j, np.exp(2j * np.pi * 0.113)]])
    f = lag_frequency(z)
    assert f.shape == z.shape and f.dtype == np.float64
    want = np.array([[0.0, 0.25, -0.25, 0.5], [0.125, np.nan, -0.125, 0.113]])
    assert np.array_equal(np.isnan(f), np.isnan(want)) and np.isnan(f[1, 1])
    ok = ~np.isnan(want)
    assert np.abs(f[ok] - want[ok]).max() <= 1e-15
    # the magnitude does not matter, the sample rate scales, complex64 sums are taken as they are
    assert np.abs(lag_frequency(z * 1e-30)[ok] - want[ok]).max() <= 1e-15
    assert np.abs(lag_frequency(z, 48000.0)[ok] - 48000.0 * want[ok]).max() <= 1e-10
    f32 = lag_frequency(z.astype(np.complex64), 2.0)
    assert f32.dtype == np.float64 and np.isnan(f32[1, 1]) and np.abs(f32[ok] - 2.0 * want[ok]).max() <= 1e-7
    # a zero of either sign in both components is "no estimate"; a zero in one component is an angle
    zeros = np.array([complex(0.0, 0.0), complex(-0.0, 0.0), complex(0.0, -0.0), complex(-0.0, -0.0), complex(0.0, 1e-300)])
    fz = lag_frequency(zeros)
    assert np.isnan(fz[:4]).all() and fz[4] == 0.25
    # a conjugate on the wrong side negates every estimate
    assert np.array_equal(lag_frequency(np.conj(z))[ok][:3], -want[ok][:3])
    assert lag_frequency(np.zeros((0, 4), dtype=np.complex128)).shape == (0, 4)


def test_lag_sum_declared_in_the_headers():
    with open(os.path.join(ROOT, "include", "sdft", "sdft_hip.h")) as fh:
        c_header = fh.read()
    with open(os.path.join(ROOT, "include", "sdft", "sdft.hpp")) as fh:
        cpp_header = fh.read()
    assert "long sdft_hip_sdft_lag_sum_n(sdft_t* sdft, const sdft_size_t nsamples, const sdft_td_t* samples," in c_header
    assert "sdft_fdx_t* sums) SDFT_HIP_SYMBOL(sdft_lag_sum_n);" in c_header
    assert '("last_kernel" = 12)' in c_header and "12 (lag-product analysis)" in c_header
    assert "sdft_hip_sdft_lag_sum_n_##SUF" in cpp_header and "std::size_t lag_sum(" in cpp_header


def test_lag_sum_kernel_header_is_listed():
    from sdft_amd import build as B
    assert "sdft_forward_lag_sum.hpp" in B.KERNEL_FILES
    assert B.KERNEL_FILES.index("sdft_forward_cross_sum.hpp") < B.KERNEL_FILES.index("sdft_forward_lag_sum.hpp")
    with open(os.path.join(CSRC, "sdft_kernels.hpp")) as fh:
        assert '#include "sdft_forward_lag_sum.hpp"' in fh.read()


def test_lag_sum_logic_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ on this host")
    exe = str(tmp_path / "lag_sum_logic_test")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
           f"-I{CSRC}", os.path.join(ROOT, "tests", "cpp", "lag_sum_logic_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "lag-sum-logic: all properties hold" in r.stdout


@pytest.mark.parametrize("combo", COMBOS)
def test_lag_sum_kernel_instantiations_in_code_object(hip_library, combo):
    """The four window instantiations of forward_lag_sum_kernel at the type pair's one bins-per-lane are in the translation unit's
    gfx950 code object (names only); the pooled-power and cross-spectrum kernels beside them, whose adders the call reuses, are the
    sets they were."""
    kernels = disassemble(combo, hip_library)
    fd = "double" if combo.endswith("f64") else "float"
    bpl = 1 if fd == "double" else 2
    found = {name for name in kernels if name.startswith("forward_lag_sum_kernel")}
    assert found == {f"forward_lag_sum_kernel<{fd}, {bpl}, {w}>" for w in range(4)}, sorted(found)
    pooled = {name for name in kernels if name.startswith("forward_pooled_power_kernel")}
    assert pooled == {f"forward_pooled_power_kernel<{fd}, {bpl}, {w}>" for w in range(4)}, sorted(pooled)
    cross = {name for name in kernels if name.startswith("forward_cross_sum_kernel")}
    assert cross == {f"forward_cross_sum_kernel<{fd}, {bpl}, {w}>" for w in range(4)}, sorted(cross)
    for helper in ("pooled_power_rows_kernel", "pooled_power_add_kernel"):
        assert {name.split("(")[0] for name in kernels if name.startswith(helper)} == {f"{helper}<{fd}>"}, helper
