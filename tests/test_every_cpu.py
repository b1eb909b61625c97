"""Decimated analysis (sdft_hip_sdft_every_n) without a GPU: the symbol of every type pair, the NULL-plan error, the host-side
logic (row count, streaming grid, time chunks; tests/cpp/every_logic_test.cpp under g++ -fsanitize=address,undefined) and the
kernel itself in every translation unit's gfx950 code object."""

import os
import re
import shutil
import subprocess

import pytest

from test_capi_cpu import disassemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdft_amd", "csrc")
COMBOS = ("f32f64", "f32f32", "f64f64", "f64f32")


def test_every_symbol_exported_for_all_type_pairs(hip_library):
    from sdft_amd import capi
    lib = capi.load()
    for combo in COMBOS:
        assert hasattr(lib, f"sdft_hip_sdft_every_n_{combo}"), combo
    assert "sdft_every_n" in capi.typed_signatures("f32f64")


@pytest.mark.parametrize("combo", COMBOS)
def test_every_null_plan_returns_minus_one(hip_library, combo):
    from sdft_amd import capi
    api = capi.Api(combo)
    api.clear()
    assert api.sdft_every_n(None, 100, None, 10, 0, None) == -1
    err = api.last_error()
    assert err and "sdft_hip_sdft_every_n" in err and "NULL plan" in err, err
    api.clear()


def test_every_logic_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ on this host")
    exe = str(tmp_path / "every_logic_test")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
           f"-I{CSRC}", os.path.join(ROOT, "tests", "cpp", "every_logic_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "all properties hold" in r.stdout


@pytest.mark.parametrize("combo", COMBOS)
def test_every_kernel_in_code_object_without_scratch(hip_library, combo):
    """All four window instantiations of forward_every_kernel (one bins-per-lane each: 16 bytes per lane) are in the
    translation unit's gfx950 code object, hold the recurrence's arithmetic, and spill nothing."""
    kernels = disassemble(combo, hip_library)
    fd = "double" if combo.endswith("f64") else "float"
    bpl = 1 if fd == "double" else 2
    found = {name: body for name, body in kernels.items() if name.startswith("forward_every_kernel")}
    want = {f"forward_every_kernel<{fd}, {bpl}, {w}>" for w in range(4)}
    assert set(found) == want, sorted(found)
    for name, body in found.items():
        spills = [l for l in body if "scratch_" in l]
        assert not spills, (combo, name, spills[:2])
        assert any(re.search(r"\bv_(pk_)?mul_f(32|64)(_e32|_e64|_dpp|_sdwa)?\b", l) for l in body), name
        assert any(re.search(r"\bglobal_store_dwordx4\b", l) for l in body), name          # 16-byte row stores
