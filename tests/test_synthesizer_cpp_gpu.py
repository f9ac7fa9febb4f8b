"""tsd_amd::synthetiseur_polyphase (libtsd_amd/host/adaptors/gpu_synthetiseur.cc) through the C++ host library, on host and
resident vectors, against a double-precision loop of the definition, then canaliseur_polyphase -> filtre_rif_canaux ->
synthetiseur_polyphase on resident vectors (tests/cpp/test_synthetiseur.cc)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_synthesizer_cpp(tmp_path):
    lib = os.path.join(ROOT, "libtsd_amd", "lib")
    subprocess.run(["make", "-C", os.path.join(ROOT, "libtsd_amd", "host")], check=True, capture_output=True)
    exe = str(tmp_path / "test_synthetiseur")
    subprocess.run(["g++", "-std=c++20", "-O1", "-I" + os.path.join(ROOT, "libtsd_amd", "host", "include"),
                    "-I" + os.path.join(ROOT, "libtsd_amd", "host", "include_ext"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "test_synthetiseur.cc"), "-L" + lib, "-ltsd_host", "-ltsdgpu",
                    "-Wl,-rpath," + lib], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "test_synthetiseur OK" in r.stdout, r.stdout + r.stderr
