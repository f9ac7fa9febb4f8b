"""tsd_amd::filtre_rif_decim_canaux / filtre_rif_demi_bande_canaux / filtre_rif_ups_canaux / decimateur_canaux
(libtsd_amd/host/adaptors/gpu_canaux_rythme.cc) through the C++ host library, on host and resident vectors, against separate
filtre_rif_decim / filtre_rif_demi_bande / filtre_rif_ups / decimateur objects (tests/cpp/test_canaux_rythme.cc)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rate_changing_channel_banks_cpp(tmp_path):
    lib = os.path.join(ROOT, "libtsd_amd", "lib")
    subprocess.run(["make", "-C", os.path.join(ROOT, "libtsd_amd", "host")], check=True, capture_output=True)
    exe = str(tmp_path / "test_canaux_rythme")
    subprocess.run(["g++", "-std=c++20", "-O1", "-I" + os.path.join(ROOT, "libtsd_amd", "host", "include"),
                    "-I" + os.path.join(ROOT, "libtsd_amd", "host", "include_ext"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "test_canaux_rythme.cc"), "-L" + lib, "-ltsd_host", "-ltsdgpu",
                    "-Wl,-rpath," + lib], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "test_canaux_rythme OK" in r.stdout, r.stdout + r.stderr
