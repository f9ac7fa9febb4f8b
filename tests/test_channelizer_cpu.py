"""Polyphase channelizer (include/tsdgpu.h: tsdgpu_channelizer), the parts that need no GPU: the two float64 references of
tests/chan_ref.py against each other, the exported symbols and the absence of a CPU fallback, and the adaptor compiled against
libtsd's own headers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import chan_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "libtsd_amd", "host")
REF = "/root/reference/core"


@pytest.mark.parametrize("M", [8, 16, 64])
def test_definition_and_fast_form_agree(M):
    F = 12
    x = R.stream(F * M, M, seed=M)
    for K in (1, M - 1, M + 1, 3 * M - 3):
        h = R.prototype(M, K)
        d, p = R.definition(x, h, M), R.polyphase64(x, h, M)
        assert d.shape == p.shape == (M, F)
        assert R.rel_err(p, d) <= 1e-12, (M, K)
        # the run split in two steps, the second from the carried history
        H = (-(-K // M) - 1) * M
        cut = 5 * M
        hist = np.concatenate([np.zeros(H, np.complex64), x[:cut]])[cut:cut + H] if H else None
        for fn in (R.definition, R.polyphase64):
            two = np.concatenate([fn(x[:cut], h, M), fn(x[cut:], h, M, hist)], axis=1)
            assert R.rel_err(two, d) <= 1e-12, (M, K, fn.__name__)


def test_channel_centre_gain_is_the_sum_of_the_taps():
    M, K, F = 16, 40, 30
    h = R.prototype(M, K)
    x = np.exp(2j * np.pi * (5 / M) * np.arange(F * M)).astype(np.complex64)
    y = R.polyphase64(x, h, M)
    assert abs(y[5, -1] - h.sum()) <= 1e-6 * abs(h.sum())


def test_channelizer_has_no_cpu_fallback():
    import libtsd_amd as t
    for s in ("create", "out_count", "step", "reset", "history_len", "get_state", "set_state", "destroy"):
        assert hasattr(t.lib(), "tsdgpu_channelizer_" + s), s
    chan = t.Channelizer                     # (the class exists whether or not a GPU does)
    if t.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(t.TsdGpuError):
        chan(R.prototype(8, 17), 8)


@pytest.mark.skipif(not os.path.isdir(REF) or shutil.which("g++") is None,
                    reason="needs the reference tree and g++ (build container only)")
def test_channelizer_adaptor_compiles_against_reference_headers(tmp_path):
    """gpu_canaliseur.cc, unchanged, against libtsd's own headers (the compiler line of test_rate_bank_cpu.py)."""
    import torch
    inc = os.path.join(os.path.dirname(torch.__file__), "include")
    cmd = ["g++", "-std=c++20", "-O0", "-w", "-DFMT_HEADER_ONLY=1", "-DLIBTSD_USE_PNG=0", "-DLIBTSD_USE_FREETYPE=0",
           "-DLIBTSD_USE_GTKMM=0", f"-I{REF}/include", f"-I{inc}", f"-I{HOST}/include_ext", f"-I{ROOT}/include", "-c",
           f"{HOST}/adaptors/gpu_canaliseur.cc", "-o", str(tmp_path / "gpu_canaliseur.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    syms = subprocess.run(["nm", "-C", "--defined-only", str(tmp_path / "gpu_canaliseur.o")], capture_output=True, text=True).stdout
    assert "tsd_amd::canaliseur_polyphase" in syms
