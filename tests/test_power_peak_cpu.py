"""Peak-hold analysis (sdft_hip_sdft_power_peak_n) without a GPU: the symbol of every type pair, the NULL-plan error, a hold that
is neither 0 nor 1, the declarations in the headers, the host-side logic (kernel id, route and time chunks, the combining rule;
tests/cpp/power_peak_logic_test.cpp under g++ -fsanitize=address,undefined) and the kernels' instantiations in every translation
unit's gfx950 code object, beside an unchanged set of pooled-power kernels."""

import os
import shutil
import subprocess

import pytest

from test_capi_cpu import disassemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdft_amd", "csrc")
COMBOS = ("f32f64", "f32f32", "f64f64", "f64f32")


def test_power_peak_symbol_exported_for_all_type_pairs(hip_library):
    from sdft_amd import capi
    lib = capi.load()
    for combo in COMBOS:
        assert hasattr(lib, f"sdft_hip_sdft_power_peak_n_{combo}"), combo
        assert "sdft_power_peak_n" in capi.typed_signatures(combo)


@pytest.mark.parametrize("combo", COMBOS)
def test_power_peak_null_plan_returns_minus_one(hip_library, combo):
    from sdft_amd import capi
    api = capi.Api(combo)
    api.clear()
    for hold in (0, 1):
        assert api.sdft_power_peak_n(None, 100, None, 10, 0, 0, 1, hold, None) == -1
        err = api.last_error()
        assert err and "sdft_hip_sdft_power_peak_n" in err and "NULL plan" in err, err
        api.clear()


def test_power_peak_bad_hold_is_refused_by_the_python_call(hip_library):
    """SDFT.power_peak takes "max" / "min" or the enum's 0 / 1 and refuses anything else before the plan is touched (the C call's
    own refusal needs a plan, hence a GPU: tests/test_gpu_power_peak.py)"""
    from sdft_amd import sdft as S
    assert S.HOLDS == {"max": 0, "min": 1, 0: 0, 1: 1}

    class NoPlan:
        dftsize = 8

        class api:
            @staticmethod
            def clear():
                pass

    for bad in (2, -1, "peak", None, 0.5):
        with pytest.raises(ValueError, match="hold"):
            S.SDFT.power_peak(NoPlan(), [0.0] * 4, hold=bad)


def test_power_peak_declared_in_the_headers():
    with open(os.path.join(ROOT, "include", "sdft", "sdft_hip.h")) as fh:
        c_header = fh.read()
    with open(os.path.join(ROOT, "include", "sdft", "sdft.hpp")) as fh:
        cpp_header = fh.read()
    assert "sdft_hip_sdft_power_peak_n(" in c_header and "SDFT_HIP_SYMBOL(sdft_power_peak_n)" in c_header
    assert "enum sdft_hip_hold { sdft_hip_hold_max = 0, sdft_hip_hold_min = 1 };" in c_header
    assert '("last_kernel" = 11)' in c_header and "10 channel-mix analysis, 11 peak-hold analysis)" in c_header
    assert "sdft_hip_sdft_power_peak_n_##SUF" in cpp_header and "std::size_t power_peak(" in cpp_header


def test_power_peak_logic_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ on this host")
    exe = str(tmp_path / "power_peak_logic_test")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
           f"-I{CSRC}", os.path.join(ROOT, "tests", "cpp", "power_peak_logic_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "power-peak-logic: all properties hold" in r.stdout


@pytest.mark.parametrize("combo", COMBOS)
def test_power_peak_kernel_instantiations_in_code_object(hip_library, combo):
    """The four window instantiations of forward_power_peak_kernel for each hold, at the type pair's one bins-per-lane, and the
    kernels that combine the pieces of cut windows and join segments are in the translation unit's gfx950 code object (names only);
    the pooled-power kernels beside them are the set they were, and no new name begins like one of them or like
    forward_power_kernel."""
    kernels = disassemble(combo, hip_library)
    fd = "double" if combo.endswith("f64") else "float"
    bpl = 1 if fd == "double" else 2
    found = {name for name in kernels if name.startswith("forward_power_peak_kernel")}
    assert found == {f"forward_power_peak_kernel<{fd}, {bpl}, {w}, {h}>" for w in range(4) for h in range(2)}, sorted(found)
    for helper in ("peak_rows_kernel", "peak_join_kernel"):
        assert any(name.startswith(f"{helper}<{fd}>") for name in kernels), (helper, sorted(k for k in kernels if "peak" in k))
    pooled = {name for name in kernels if name.startswith("forward_pooled_power_kernel")}
    assert pooled == {f"forward_pooled_power_kernel<{fd}, {bpl}, {w}>" for w in range(4)}, sorted(pooled)
    for helper in ("pooled_power_rows_kernel", "pooled_power_add_kernel"):
        assert {name.split("(")[0] for name in kernels if name.startswith(helper)} == {f"{helper}<{fd}>"}, helper
    dense = {name for name in kernels if name.startswith("forward_power_kernel")}
    assert dense == {f"forward_power_kernel<{fd}, {bpl}, {w}>" for w in range(4)}, sorted(dense)
