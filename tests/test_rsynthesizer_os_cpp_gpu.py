"""The three-argument tsd_amd::synthetiseur_polyphase_reel(h, M, surech) (libtsd_amd/host/adaptors/gpu_synthetiseur_reel.cc) through
the C++ host library, on host and resident vectors, against a double-precision loop of the definition; chunked steps bit-identical
to one step; surech = 1 bit-identical to the two-argument factory; the bits of the C ABI; the échec texts of a bad n and a bad
surech (tests/cpp/test_synthetiseur_reel_os.cc)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oversampled_real_synthesizer_cpp(tmp_path):
    lib = os.path.join(ROOT, "libtsd_amd", "lib")
    subprocess.run(["make", "-C", os.path.join(ROOT, "libtsd_amd", "host")], check=True, capture_output=True)
    exe = str(tmp_path / "test_synthetiseur_reel_os")
    subprocess.run(["g++", "-std=c++20", "-O1", "-I" + os.path.join(ROOT, "libtsd_amd", "host", "include"),
                    "-I" + os.path.join(ROOT, "libtsd_amd", "host", "include_ext"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "test_synthetiseur_reel_os.cc"), "-L" + lib, "-ltsd_host", "-ltsdgpu",
                    "-Wl,-rpath," + lib], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "test_synthetiseur_reel_os OK" in r.stdout, r.stdout + r.stderr
