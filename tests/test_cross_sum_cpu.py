"""Pooled cross-spectrum analysis (sdft_hip_set_pairs, sdft_hip_pairs, sdft_hip_sdft_cross_sum_n) without a GPU: the symbols of
every type pair, the NULL-plan errors, the host-side logic (accepted pair lists, the table of work items, one writer per channel,
workspace and slots, time chunks, the route; tests/cpp/cross_sum_logic_test.cpp under g++ -fsanitize=address,undefined) and the
kernel's instantiations in every translation unit's gfx950 code object."""

import os
import shutil
import subprocess

import pytest

from test_capi_cpu import disassemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdft_amd", "csrc")
COMBOS = ("f32f64", "f32f32", "f64f64", "f64f32")
SYMBOLS = ("set_pairs", "pairs", "sdft_cross_sum_n")


def test_cross_sum_symbols_exported_for_all_type_pairs(hip_library):
    from sdft_amd import capi
    lib = capi.load()
    for combo in COMBOS:
        for name in SYMBOLS:
            assert hasattr(lib, f"sdft_hip_{name}_{combo}"), (combo, name)
            assert name in capi.typed_signatures(combo)


def test_cross_sum_declared_in_the_headers():
    with open(os.path.join(ROOT, "include", "sdft", "sdft_hip.h")) as fh:
        c_header = fh.read()
    with open(os.path.join(ROOT, "include", "sdft", "sdft.hpp")) as fh:
        cpp_header = fh.read()
    for name in SYMBOLS:
        assert f"sdft_hip_{name}(" in c_header and f"SDFT_HIP_SYMBOL({name})" in c_header, name
        assert f"sdft_hip_{name}_##SUF" in cpp_header, name


@pytest.mark.parametrize("combo", COMBOS)
def test_cross_sum_null_plan_returns_minus_one(hip_library, combo):
    from sdft_amd import capi
    api = capi.Api(combo)
    api.clear()
    assert api.sdft_cross_sum_n(None, 100, None, 10, 0, 0, 1, None) == -1
    err = api.last_error()
    assert err and "sdft_hip_sdft_cross_sum_n" in err and "NULL plan" in err, err
    api.clear()
    assert api.set_pairs(None, 0, None, None) == -1
    err = api.last_error()
    assert err and "sdft_hip_set_pairs" in err and "NULL plan" in err, err
    api.clear()
    assert api.pairs(None) == 0 and api.last_error() is None


def test_cross_sum_logic_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ on this host")
    exe = str(tmp_path / "cross_sum_logic_test")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
           f"-I{CSRC}", os.path.join(ROOT, "tests", "cpp", "cross_sum_logic_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "cross-sum-logic: all properties hold" in r.stdout


@pytest.mark.parametrize("combo", COMBOS)
def test_cross_sum_kernel_instantiations_in_code_object(hip_library, combo):
    """The four window instantiations of forward_cross_sum_kernel, at the type pair's one bins-per-lane, are in the translation
    unit's gfx950 code object (names only); the kernels that add the pieces of cut windows are the pooled power call's."""
    kernels = disassemble(combo, hip_library)
    fd = "double" if combo.endswith("f64") else "float"
    bpl = 1 if fd == "double" else 2
    found = {name for name in kernels if name.startswith("forward_cross_sum_kernel")}
    assert found == {f"forward_cross_sum_kernel<{fd}, {bpl}, {w}>" for w in range(4)}, sorted(found)
    for helper in ("pooled_power_rows_kernel", "pooled_power_add_kernel"):
        assert any(name.startswith(f"{helper}<{fd}>") for name in kernels), (helper, sorted(k for k in kernels if "pooled" in k))
