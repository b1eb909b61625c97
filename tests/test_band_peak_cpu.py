"""Band-peak analysis (sdft_hip_sdft_band_peak_n) without a GPU: the symbol of every type pair, the NULL-plan error, the
declarations in the headers (which compile as C and C++), the host-side logic (kernel id, route and time chunks, rows of a launch
with a slot of two numbers; tests/cpp/band_peak_logic_test.cpp under g++ -fsanitize=address,undefined), the rule's host
restatement (logic::band_peak_take) against np.argmax on drawn vectors with ties, zeros of both signs, negatives, NaN and inf, the
kernels' instantiations in every translation unit's gfx950 code object beside an unchanged set of the filterbank kernels, and the
Python helpers that need no plan (band_peak_split, filterbank.flat, filterbank.peak_frequency)."""

import os
import shutil
import subprocess

import numpy as np
import pytest

from test_capi_cpu import disassemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdft_amd", "csrc")
INC = os.path.join(ROOT, "include")
COMBOS = ("f32f64", "f32f32", "f64f64", "f64f32")


def test_band_peak_symbol_exported_for_all_type_pairs(hip_library):
    from sdft_amd import capi
    lib = capi.load()
    for combo in COMBOS:
        assert hasattr(lib, f"sdft_hip_sdft_band_peak_n_{combo}"), combo
        assert "sdft_band_peak_n" in capi.typed_signatures(combo)
        assert capi.typed_signatures(combo)["sdft_band_peak_n"] == capi.typed_signatures(combo)["sdft_filterbank_n"]


@pytest.mark.parametrize("combo", COMBOS)
def test_band_peak_null_plan_returns_minus_one(hip_library, combo):
    from sdft_amd import capi
    api = capi.Api(combo)
    api.clear()
    assert api.sdft_band_peak_n(None, 100, None, 10, 0, None) == -1
    err = api.last_error()
    assert err and "sdft_hip_sdft_band_peak_n" in err and "NULL plan" in err, err
    api.clear()


def test_band_peak_declared_in_the_headers():
    with open(os.path.join(INC, "sdft", "sdft_hip.h")) as fh:
        c_header = fh.read()
    with open(os.path.join(INC, "sdft", "sdft.hpp")) as fh:
        cpp_header = fh.read()
    assert "long sdft_hip_sdft_band_peak_n(sdft_t* sdft, const sdft_size_t nsamples, const sdft_td_t* samples," in c_header
    assert "sdft_fd_t* peaks) SDFT_HIP_SYMBOL(sdft_band_peak_n);" in c_header
    assert '("last_kernel" = 14)' in c_header and "14 (band-peak analysis)" in c_header and '"last_band_peak_launches"' in c_header
    assert c_header.index("---- filterbank analysis") < c_header.index("---- band-peak analysis") < c_header.index("---- pooled cross-spectrum analysis")
    section = c_header[c_header.index("---- band-peak analysis"):c_header.index("---- pooled cross-spectrum analysis")]
    # the equivalence the GPU tests rely on, the rule, the refusal and the six promises are stated
    assert "i = np.argmax(v) and m = v[i]" in section
    assert "(v_k > m) || (v_k != v_k && m == m)" in section
    assert "2^24" in section and "2.1e-11" in section
    for k in range(1, 7):
        assert f"({k}) " in section, k
    assert "sdft_hip_sdft_band_peak_n_##SUF" in cpp_header and "std::size_t band_peak(" in cpp_header
    assert cpp_header.index("std::size_t filterbank(") < cpp_header.index("std::size_t band_peak(")


def test_band_peak_headers_compile_as_c_and_cxx(tmp_path):
    """a C host of every type pair refers to its own symbol; the C++ facade's band_peak instantiates for the four pairs"""
    src = tmp_path / "t.c"
    src.write_text("#include <sdft/sdft.h>\n"
                   "long use(sdft_t* p, const sdft_td_t* x, sdft_fd_t* peaks) { return sdft_hip_sdft_band_peak_n(p, 10, x, 2, 1, peaks); }\n")
    for flags in ([], ["-DSDFT_FD_FLOAT"], ["-DSDFT_TD_DOUBLE", "-DSDFT_NO_COMPLEX_H"], ["-DSDFT_TD_DOUBLE", "-DSDFT_FD_FLOAT", "-DSDFT_NO_COMPLEX_H"]):
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INC, *flags, "-c", str(src), "-o", str(tmp_path / "t.o")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        nm = subprocess.run(["nm", str(tmp_path / "t.o")], capture_output=True, text=True).stdout
        suffix = ("f64" if "-DSDFT_TD_DOUBLE" in flags else "f32") + ("f32" if "-DSDFT_FD_FLOAT" in flags else "f64")
        assert f"sdft_hip_sdft_band_peak_n_{suffix}" in nm, (flags, nm)
    r = subprocess.run(["g++", "-x", "c++", "-fsyntax-only", "-I", INC, os.path.join(INC, "sdft", "sdft.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cpp = tmp_path / "t.cpp"
    cpp.write_text("#include <sdft/sdft.h>\n"
                   "template <class T, class F> std::size_t use() { sdft::SDFT<T, F> s(8, sdft::Window::Hann, 1); T x[4] = {}; F peaks[4 * 2 * 2];"
                   " return s.band_peak(4, x, 1, 0, peaks); }\n"
                   "int main() { return (int)(use<float, double>() + use<float, float>() + use<double, double>() + use<double, float>()); }\n")
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(INC, "cpp"), "-c", str(cpp), "-o", str(tmp_path / "tt.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    nm = subprocess.run(["nm", str(tmp_path / "tt.o")], capture_output=True, text=True).stdout
    for suf in COMBOS:
        assert f"sdft_hip_sdft_band_peak_n_{suf}" in nm, suf


def test_band_peak_kernel_header_is_listed():
    from sdft_amd import build as B
    assert "sdft_forward_band_peak.hpp" in B.KERNEL_FILES
    assert B.KERNEL_FILES.index("sdft_forward_filterbank.hpp") < B.KERNEL_FILES.index("sdft_forward_band_peak.hpp")
    with open(os.path.join(CSRC, "sdft_kernels.hpp")) as fh:
        assert '#include "sdft_forward_band_peak.hpp"' in fh.read()
    with open(os.path.join(CSRC, "sdft_forward_band_peak.hpp")) as fh:
        assert "#pragma clang fp contract(off)" in fh.read()


@pytest.fixture(scope="module")
def logic_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ on this host")
    exe = str(tmp_path_factory.mktemp("band_peak_logic") / "band_peak_logic_test")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
           f"-I{CSRC}", os.path.join(ROOT, "tests", "cpp", "band_peak_logic_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_band_peak_logic_under_asan_ubsan(logic_exe):
    """route: FK_BAND_PEAK, the tile form, choose_power_chunks' chunks; workspace: filterbank_segment_rows with 2 * sizeof(FD) a slot"""
    r = subprocess.run([logic_exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "band-peak-logic: all properties hold" in r.stdout


def drawn_vectors(fd, count, length, seed):
    """vectors from a small alphabet, so that ties are the rule: zeros of both signs, negatives, inf of both signs, NaN in some
    vectors, a few drawn numbers; some vectors are constant (all +0, all -0, all NaN, all -inf)"""
    rng = np.random.default_rng(seed)
    alphabet = np.array([0.0, -0.0, 1.0, 1.0, -0.5, -2.0, 3.5, np.inf, -np.inf, np.nan, 2.0 ** -140, -(2.0 ** -140)], dtype=fd)
    v = alphabet[rng.integers(0, alphabet.size, (count, length))]
    plain = rng.integers(0, 3, count) == 0                   # a third without NaN and inf: ties among finite numbers decide
    v[plain] = alphabet[:7][rng.integers(0, 7, (int(plain.sum()), length))]
    zeros = rng.integers(0, 4, count) == 0                   # a quarter of zeros alone: the first one's sign stays
    v[zeros] = alphabet[:2][rng.integers(0, 2, (int(zeros.sum()), length))]
    some = rng.integers(0, 5, count) == 0
    v[some] = rng.standard_normal((int(some.sum()), length)).astype(fd)
    for i, c in enumerate((0.0, -0.0, np.nan, -np.inf, np.inf, 1.0)):
        v[i] = fd(c)
    return np.ascontiguousarray(v)


@pytest.mark.parametrize("fd,name", [(np.float32, "f32"), (np.float64, "f64")])
@pytest.mark.parametrize("length", [1, 2, 7, 8, 61])
def test_band_peak_rule_is_numpy_argmax(logic_exe, tmp_path, fd, name, length):
    """logic::band_peak_take, scanned over a vector in ascending order, is np.argmax -- in one walk, and joined from pieces in
    ascending order (the lower piece held, the higher the candidate) for a regular and for a drawn cut"""
    v = drawn_vectors(fd, 4000, length, 17 * length + (fd == np.float64))
    v.tofile(tmp_path / "v.raw")
    r = subprocess.run([logic_exe, name, str(length), str(tmp_path / "v.raw"), str(tmp_path / "bins.raw")], capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    got = np.fromfile(tmp_path / "bins.raw", dtype=np.int64).reshape(-1, 3)
    want = np.argmax(v, axis=1)
    assert got.shape == (v.shape[0], 3)
    for j, what in enumerate(("one walk", "pieces of 7", "drawn pieces")):
        bad = np.nonzero(got[:, j] != want)[0]
        assert bad.size == 0, (what, name, length, v[bad[0]], got[bad[0]], want[bad[0]])
    # what the equivalence means for the value: equal zeros keep the first one's sign, a NaN wins
    m = np.take_along_axis(v, want[:, None], axis=1)[:, 0]
    assert (np.isnan(m) == np.isnan(v).any(axis=1)).all()
    assert np.signbit(m[0]) == False and np.signbit(m[1]) == True          # (the constant vectors of +0 and of -0)


@pytest.mark.parametrize("combo", COMBOS)
def test_band_peak_kernel_instantiations_in_code_object(hip_library, combo):
    """The four window instantiations of forward_band_peak_kernel at the type pair's one bins-per-lane and band_peak_rows_kernel
    are in the translation unit's gfx950 code object (names only); the filterbank kernels beside them are the set they were."""
    kernels = disassemble(combo, hip_library)
    fd = "double" if combo.endswith("f64") else "float"
    bpl = 1 if fd == "double" else 2
    found = {name for name in kernels if name.startswith(("forward_band_peak_kernel", "band_peak_rows_kernel"))}
    assert found == {f"forward_band_peak_kernel<{fd}, {bpl}, {w}>" for w in range(4)} | {f"band_peak_rows_kernel<{fd}>"}, sorted(found)
    fbank = {name for name in kernels if name.startswith(("forward_filterbank_kernel", "filterbank_rows_kernel"))}
    assert fbank == {f"forward_filterbank_kernel<{fd}, {bpl}, {w}>" for w in range(4)} | {f"filterbank_rows_kernel<{fd}>"}, sorted(fbank)


def trace_table():
    """{kernel: {column: int}} of profiles/band_peak_kernel_trace.txt (the first seven columns)"""
    with open(os.path.join(ROOT, "profiles", "band_peak_kernel_trace.txt")) as fh:
        text = fh.read().splitlines()
    head = next(l for l in text if l.startswith("kernel ")).split()[1:7]
    assert head == ["vgpr", "sgpr", "scratch", "vgpr_spills", "sgpr_spills", "lds"], head
    table = {}
    for l in text:
        if l.startswith(("forward_band_peak_kernel", "band_peak_rows_kernel")):
            name, rest = l[:l.index(">") + 1], l[l.index(">") + 1:].split()
            table[name] = dict(zip(head, (int(v) for v in rest[:6])))
    return table


def test_band_peak_kernel_trace_records_scratch_and_every_kind_of_spill():
    """profiles/band_peak_kernel_trace.txt: a line per instantiation with the scratch, the VGPR spills AND the SGPR spills; scratch
    and VGPR spills are 0 on every line, and the SGPR spills the forward kernel has are stated, with where they go"""
    table = trace_table()
    assert len(table) == 10
    for name, row in table.items():
        assert row["scratch"] == 0 and row["vgpr_spills"] == 0 and row["vgpr"] <= 128, (name, row)
        if name.startswith("band_peak_rows_kernel"):
            assert row["sgpr_spills"] == 0, (name, row)
    with open(os.path.join(ROOT, "profiles", "band_peak_kernel_trace.txt")) as fh:
        text = fh.read()
    assert "SGPR SPILLS" in text and "VGPR lanes" in text and "not to scratch" in text


@pytest.mark.parametrize("combo", ["f32f64", "f32f32"])
def test_band_peak_kernel_trace_is_the_code_objects(hip_library, combo):
    """every figure of the record -- registers, scratch, both spill counts, LDS -- is the one in the code object's metadata"""
    import re
    import tempfile
    llvm = "/opt/rocm/lib/llvm/bin"
    obj = os.path.join(os.path.dirname(hip_library), "obj", f"sdft_capi_{combo}.o")
    if not (os.path.exists(os.path.join(llvm, "llvm-readelf")) and os.path.exists(obj) and shutil.which("c++filt")):
        pytest.skip("llvm-readelf / c++filt / object files not available")
    with tempfile.TemporaryDirectory() as td:
        shutil.copy(obj, os.path.join(td, "dev.o"))
        subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", os.path.join(td, "dev.o")], capture_output=True, text=True, cwd=td)
        cos = [f for f in os.listdir(td) if "amdgcn" in f and "gfx950" in f]
        if not cos:
            pytest.skip("could not extract the gfx950 code object")
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", os.path.join(td, cos[0])], capture_output=True, text=True).stdout
    keys = {"vgpr": ".vgpr_count", "sgpr": ".sgpr_count", "scratch": ".private_segment_fixed_size", "vgpr_spills": ".vgpr_spill_count",
            "sgpr_spills": ".sgpr_spill_count", "lds": ".group_segment_fixed_size"}
    table, seen = trace_table(), 0
    for block in notes.split("  - .agpr_count")[1:]:
        mangled = re.search(r"\.name:\s+(\S+)", block).group(1)
        plain = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
        name = plain.split("(")[0].replace("void sdfthip::", "")
        if name not in table:
            continue
        got = {col: int(re.search(re.escape(key) + r":\s+(\d+)", block).group(1)) for col, key in keys.items()}
        assert got == table[name], (name, got, table[name])
        seen += 1
    assert seen == 5, seen                                   # four windows and the rows kernel of this FD type


# ---- the Python helpers ------------------------------------------------------------------------------------------------------

def test_band_peak_split():
    from sdft_amd.sdft import band_peak_split
    for fd in (np.float32, np.float64):
        peaks = np.zeros((3, 5, 2), dtype=fd)
        peaks[..., 0] = np.arange(15).reshape(3, 5) * 0.5
        peaks[..., 1] = np.arange(15).reshape(3, 5) * 1000 + 7
        peaks[0, 0, 0] = np.nan
        values, bins = band_peak_split(peaks)
        assert values.dtype == fd and values.shape == (3, 5) and bins.dtype == np.int64 and bins.shape == (3, 5)
        assert np.array_equal(values, peaks[..., 0], equal_nan=True) and np.array_equal(bins, np.arange(15).reshape(3, 5) * 1000 + 7)
    big = np.array([[[1.0, 2.0 ** 24 - 1]]], dtype=np.float32)          # the last bin of the largest FD float plan
    assert band_peak_split(big)[1][0, 0] == 2 ** 24 - 1
    batched = np.zeros((2, 3, 5, 2))
    assert band_peak_split(batched)[0].shape == (2, 3, 5)


def test_band_peak_bad_arguments_are_refused_by_the_python_call():
    """SDFT.band_peak refuses every < 1 and first < 0 before the plan is touched"""
    from sdft_amd import sdft as S

    class NoPlan:
        dftsize = 8

        class api:
            @staticmethod
            def clear():
                pass

    for kw in (dict(every=0), dict(every=1, first=-1)):
        with pytest.raises(ValueError):
            S.SDFT.band_peak(NoPlan(), [0.0] * 4, **kw)


def test_band_peak_out_of_another_shape_kind_or_layout_is_refused_by_the_python_call():
    """out is refused before the plan is touched when it does not end in (nbands, 2), is not of the samples' kind, or is not
    contiguous -- a reshape of such an array is a copy, and the library would write the copy: numpy arrays and tensors alike"""
    import torch
    from sdft_amd import sdft as S

    class NoPlan:
        dftsize = 8
        filterbank_bands = 3

        class api:
            @staticmethod
            def clear():
                pass

    x = np.zeros(4, dtype=np.float32)
    bad = [np.zeros((4, 3), dtype=np.float64), np.zeros((4, 2, 3), dtype=np.float64), np.zeros((4, 6), dtype=np.float64),
           np.zeros((4, 3, 4), dtype=np.float64)[:, :, ::2], np.zeros((3, 4, 2), dtype=np.float64).transpose(1, 0, 2),
           np.zeros((8, 3, 2), dtype=np.float64)[::2], torch.zeros((4, 3, 2), dtype=torch.float64)]
    for out in bad:
        with pytest.raises(ValueError):
            S.SDFT.band_peak(NoPlan(), x, out=out)
    xt = torch.zeros(4, dtype=torch.float32)
    bad = [torch.zeros((4, 3, 4), dtype=torch.float64)[:, :, ::2], torch.zeros((3, 4, 2), dtype=torch.float64).permute(1, 0, 2),
           torch.zeros((8, 3, 2), dtype=torch.float64)[::2], torch.zeros((4, 3), dtype=torch.float64), np.zeros((4, 3, 2), dtype=np.float64)]
    for out in bad:
        assert isinstance(out, np.ndarray) or out.dim() < 3 or not out.is_contiguous()
        with pytest.raises(ValueError):
            S.SDFT.band_peak(NoPlan(), xt, out=out)
    with pytest.raises(ValueError):                          # no filterbank: said before out is looked at
        NoPlan.filterbank_bands = 0
        S.SDFT.band_peak(NoPlan(), x, out=np.zeros((4, 3, 2)))


def test_flat_filterbank_and_peak_frequency():
    from sdft_amd import filterbank as F
    b0, nb, w = F.flat([0, 10, 5, 7], [4, 3, 0, 1])
    assert b0.dtype == np.uint64 and nb.dtype == np.uint64 and w.dtype == np.float64
    assert b0.tolist() == [0, 10, 7] and nb.tolist() == [4, 3, 1]           # (the band without bins is dropped)
    assert w.tolist() == [1.0] * 8
    assert np.array_equal(F.dense(16, b0, nb, w), np.array([[1] * 4 + [0] * 12, [0] * 10 + [1] * 3 + [0] * 3, [0] * 7 + [1] + [0] * 8], dtype=np.float64))
    one = F.flat(3, 5)
    assert one[0].tolist() == [3] and one[1].tolist() == [5] and one[2].size == 5
    for bad in (([0, 1], [1]), ([-1], [2]), ([0], [-2])):
        with pytest.raises(ValueError):
            F.flat(*bad)
    f = F.peak_frequency(np.array([[0, 3], [1023, 512]]), 1024, 48000)
    assert f.dtype == np.float64 and f.shape == (2, 2)
    assert np.array_equal(f, F.bin_frequencies(1024, 48000)[np.array([[0, 3], [1023, 512]])])
    assert F.peak_frequency(5, 10, 2.0) == 0.5
