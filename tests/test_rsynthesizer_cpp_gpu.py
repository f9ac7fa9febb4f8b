"""tsd_amd::synthetiseur_polyphase_reel (libtsd_amd/host/adaptors/gpu_synthetiseur_reel.cc) through the C++ host library, on host and
resident vectors, against a double-precision loop of the definition and the bits of the C ABI: M = 32, K = 100, two steps
(tests/cpp/test_synthetiseur_reel.cc)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_real_synthesizer_cpp(tmp_path):
    lib = os.path.join(ROOT, "libtsd_amd", "lib")
    subprocess.run(["make", "-C", os.path.join(ROOT, "libtsd_amd", "host")], check=True, capture_output=True)
    exe = str(tmp_path / "test_synthetiseur_reel")
    subprocess.run(["g++", "-std=c++20", "-O1", "-I" + os.path.join(ROOT, "libtsd_amd", "host", "include"),
                    "-I" + os.path.join(ROOT, "libtsd_amd", "host", "include_ext"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "test_synthetiseur_reel.cc"), "-L" + lib, "-ltsd_host", "-ltsdgpu",
                    "-Wl,-rpath," + lib], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "test_synthetiseur_reel OK" in r.stdout, r.stdout + r.stderr
