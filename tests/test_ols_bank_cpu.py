"""The overlap-save FIR bank (tsdgpu_fir_bank_create_method), the parts that need no GPU: no CPU fallback, the exported
symbols, and the three-argument filtre_rif_canaux compiled against libtsd's own headers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "libtsd_amd", "host")
REF = "/root/reference/core"


def test_overlap_save_bank_has_no_cpu_fallback():
    import libtsd_amd as t
    if t.device_count() > 0:
        pytest.skip("GPU present")
    for method in (t.FIR_OVERLAP_SAVE, t.FIR_AUTO):
        with pytest.raises(t.TsdGpuError):
            t.FirBank([1.0, 2.0, 3.0], t.F32, 4, method=method)


def test_bank_method_symbols_are_exported_and_declared():
    import libtsd_amd as t
    L = t.lib()
    for name in ("tsdgpu_fir_bank_create_method", "tsdgpu_fir_bank_method_used"):
        assert hasattr(L, name), name
        assert name + "(" in open(os.path.join(ROOT, "include", "tsdgpu.h")).read(), name
    assert L.tsdgpu_fir_bank_method_used(None) == -1


def test_bank_binding_takes_a_method_and_defaults_to_direct():
    import inspect
    import libtsd_amd as t
    sig = inspect.signature(t.FirBank.__init__)
    assert sig.parameters["method"].default == t.FIR_DIRECT
    assert isinstance(t.FirBank.method_used, property)


@pytest.mark.skipif(not os.path.isdir(REF) or shutil.which("g++") is None,
                    reason="needs the reference tree and g++ (build container only)")
def test_bank_adaptor_defines_the_method_overload_against_reference_headers(tmp_path):
    """gpu_canaux.cc against libtsd's own headers (the compiler line of test_bank_cpu.py): both forms of filtre_rif_canaux."""
    import torch
    inc = os.path.join(os.path.dirname(torch.__file__), "include")
    cmd = ["g++", "-std=c++20", "-O0", "-w", "-DFMT_HEADER_ONLY=1", "-DLIBTSD_USE_PNG=0", "-DLIBTSD_USE_FREETYPE=0",
           "-DLIBTSD_USE_GTKMM=0", f"-I{REF}/include", f"-I{inc}", f"-I{HOST}/include_ext", f"-I{ROOT}/include", "-c",
           f"{HOST}/adaptors/gpu_canaux.cc", "-o", str(tmp_path / "gpu_canaux.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    syms = subprocess.run(["nm", "-C", "--defined-only", str(tmp_path / "gpu_canaux.o")], capture_output=True, text=True).stdout
    forms = [l for l in syms.splitlines() if "tsd_amd::filtre_rif_canaux<" in l]
    assert any("MethodeRIF" in l for l in forms), forms
    assert any("MethodeRIF" not in l for l in forms), forms
