"""Channel banks (include/tsdgpu.h: tsdgpu_fir_bank / tsdgpu_sos_bank), the parts that need no GPU: the binding's 2-D
pointer / stride helper, the absence of a CPU fallback, and the bank adaptor compiled against libtsd's own headers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "libtsd_amd", "host")
REF = "/root/reference/core"


def test_ptr2d_accepts_packed_and_row_strided_views():
    from libtsd_amd import capi
    a = np.zeros((3, 10), np.float32)
    assert capi._ptr2d(a, 3) == (a.ctypes.data, 10)
    b = np.zeros((3, 17), np.complex64)[:, :10]          # rows of 17 samples, 10 used
    assert capi._ptr2d(b, 3) == (b.ctypes.data, 17)
    import torch
    t = torch.zeros(4, 33)[:, 1:9]
    assert capi._ptr2d(t, 4) == (t.data_ptr(), 33)
    one = np.zeros((1, 5), np.float32)
    assert capi._ptr2d(one, 1) == (one.ctypes.data, 5)


def test_ptr2d_refuses_what_the_banks_cannot_read():
    from libtsd_amd import capi
    import torch
    for bad in (np.zeros((2, 4), np.float64), np.zeros((2, 4), np.complex128), np.zeros((2, 4), np.int32),
                torch.zeros(2, 4, dtype=torch.float64)):
        with pytest.raises(capi.TsdGpuError):
            capi._ptr2d(bad, 2)
    for wrong_rank in (np.zeros(8, np.float32), torch.zeros(8), np.zeros((1, 2, 2), np.float32)):
        with pytest.raises(capi.TsdGpuError):
            capi._ptr2d(wrong_rank, 1)
    with pytest.raises(capi.TsdGpuError):
        capi._ptr2d(np.zeros((3, 4), np.float32), 2)             # channel count mismatch
    with pytest.raises(capi.TsdGpuError):
        capi._ptr2d(np.zeros((2, 8), np.float32)[:, ::2], 2)     # stride(-1) != 1
    with pytest.raises(capi.TsdGpuError):
        capi._ptr2d(torch.zeros(2, 8)[:, ::2], 2)
    with pytest.raises(capi.TsdGpuError):
        capi._ptr2d(np.zeros((4, 2), np.float32).T, 2)           # column-major view: samples of a row not contiguous
    with pytest.raises(capi.TsdGpuError):
        capi._ptr2d(np.zeros((2, 4), np.float32)[::-1], 2)       # negative row stride


def test_banks_have_no_cpu_fallback():
    import libtsd_amd as t
    if t.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(t.TsdGpuError):
        t.FirBank([1.0, 2.0, 3.0], t.F32, 4)
    with pytest.raises(t.TsdGpuError):
        t.SosBank(np.array([[1.0, 2.0, 1.0, -0.5, 0.25]]), 1.0, t.F32, 4)


@pytest.mark.skipif(not os.path.isdir(REF) or shutil.which("g++") is None,
                    reason="needs the reference tree and g++ (build container only)")
def test_bank_adaptor_compiles_against_reference_headers(tmp_path):
    """gpu_canaux.cc, unchanged, against libtsd's own headers (the compiler line of test_boundary_ref_headers.py)."""
    import torch
    inc = os.path.join(os.path.dirname(torch.__file__), "include")
    cmd = ["g++", "-std=c++20", "-O0", "-w", "-DFMT_HEADER_ONLY=1", "-DLIBTSD_USE_PNG=0", "-DLIBTSD_USE_FREETYPE=0",
           "-DLIBTSD_USE_GTKMM=0", f"-I{REF}/include", f"-I{inc}", f"-I{HOST}/include_ext", f"-I{ROOT}/include", "-c",
           f"{HOST}/adaptors/gpu_canaux.cc", "-o", str(tmp_path / "gpu_canaux.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    syms = subprocess.run(["nm", "-C", "--defined-only", str(tmp_path / "gpu_canaux.o")], capture_output=True, text=True).stdout
    assert "tsd_amd::filtre_rif_canaux" in syms and "tsd_amd::filtre_sois_canaux" in syms
