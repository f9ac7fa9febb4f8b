"""Rate-changing channel bank (include/tsdgpu.h: tsdgpu_polyfir_bank), the parts that need no GPU: the absence of a CPU
fallback, and the bank adaptor compiled against libtsd's own headers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "libtsd_amd", "host")
REF = "/root/reference/core"


def test_rate_bank_has_no_cpu_fallback():
    import libtsd_amd as t
    bank = t.PolyFirBank                      # (the class exists whether or not a GPU does)
    for s in ("create", "out_count", "step", "reset", "history_len", "get_state", "set_state", "destroy"):
        assert hasattr(t.lib(), "tsdgpu_polyfir_bank_" + s), s
    if t.device_count() > 0:
        pytest.skip("GPU present")
    for kind, taps in ((t.POLY_DECIM, [1.0, 2.0, 3.0]), (t.POLY_HALFBAND, [1.0, 2.0, 3.0]), (t.POLY_UPS, [1.0, 2.0, 3.0]),
                       (t.POLY_PICK, None)):
        with pytest.raises(t.TsdGpuError):
            bank(kind, t.F32, 4, taps, 2)


@pytest.mark.skipif(not os.path.isdir(REF) or shutil.which("g++") is None,
                    reason="needs the reference tree and g++ (build container only)")
def test_rate_bank_adaptor_compiles_against_reference_headers(tmp_path):
    """gpu_canaux_rythme.cc, unchanged, against libtsd's own headers (the compiler line of test_bank_cpu.py)."""
    import torch
    inc = os.path.join(os.path.dirname(torch.__file__), "include")
    cmd = ["g++", "-std=c++20", "-O0", "-w", "-DFMT_HEADER_ONLY=1", "-DLIBTSD_USE_PNG=0", "-DLIBTSD_USE_FREETYPE=0",
           "-DLIBTSD_USE_GTKMM=0", f"-I{REF}/include", f"-I{inc}", f"-I{HOST}/include_ext", f"-I{ROOT}/include", "-c",
           f"{HOST}/adaptors/gpu_canaux_rythme.cc", "-o", str(tmp_path / "gpu_canaux_rythme.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    syms = subprocess.run(["nm", "-C", "--defined-only", str(tmp_path / "gpu_canaux_rythme.o")], capture_output=True, text=True).stdout
    for name in ("filtre_rif_decim_canaux", "filtre_rif_demi_bande_canaux", "filtre_rif_ups_canaux", "decimateur_canaux"):
        assert "tsd_amd::" + name in syms, name
