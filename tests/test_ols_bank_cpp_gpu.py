"""tsd_amd::filtre_rif_canaux(h, nb_canaux, méthode) (libtsd_amd/host/adaptors/gpu_canaux.cc) on the overlap-save bank through
the C++ host library, float and cfloat, against the oracle's FiltreRIF (tests/cpp/test_canaux_ols.cc)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_overlap_save_channel_bank_cpp(tmp_path):
    lib = os.path.join(ROOT, "libtsd_amd", "lib")
    subprocess.run(["make", "-C", os.path.join(ROOT, "libtsd_amd", "host")], check=True, capture_output=True)
    exe = str(tmp_path / "test_canaux_ols")
    subprocess.run(["g++", "-std=c++20", "-O1", "-I" + os.path.join(ROOT, "libtsd_amd", "host", "include"),
                    "-I" + os.path.join(ROOT, "libtsd_amd", "host", "include_ext"), "-I" + os.path.join(ROOT, "oracle"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "test_canaux_ols.cc"), "-x", "c", os.path.join(ROOT, "oracle", "tsd_oracle.c"),
                    "-x", "none", "-L" + lib, "-ltsd_host", "-ltsdgpu", "-Wl,-rpath," + lib, "-lm"], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "test_canaux_ols OK" in r.stdout, r.stdout + r.stderr
