"""Oversampled polyphase channelizer (include/tsdgpu.h: tsdgpu_channelizer_create_oversampled), the parts that need no GPU: the
two float64 references of tests/chan_os_ref.py against each other and against chan_ref at OS = 1, the band an oversampled row
keeps beyond the critically sampled edge, the exported symbols and the absence of a CPU fallback, and the adaptor compiled
against libtsd's own headers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import chan_os_ref as O
import chan_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "libtsd_amd", "host")
REF = "/root/reference/core"


def _taps(M, OS):
    D = M // OS
    return sorted({1, max(D - 1, 1), M + 1, 3 * M - 3})


def _carried(x, cut, H):
    """the H samples before x[cut], zeros before x[0]"""
    return np.concatenate([np.zeros(H, np.complex64), x[:cut]])[cut:cut + H]


@pytest.mark.parametrize("OS", [2, 4])
@pytest.mark.parametrize("M", [8, 16, 64])
def test_definition_and_fast_form_agree(M, OS):
    F, D = 13, M // OS
    x = R.stream(F * D, M, seed=M + OS)
    for K in _taps(M, OS):
        h = R.prototype(M, K)
        d, p = O.definition(x, h, M, OS), O.polyphase64(x, h, M, OS)
        assert d.shape == p.shape == (M, F)
        assert R.rel_err(p, d) <= 1e-12, (M, OS, K)
        # the run split at hop 5 (an odd hop): the second step from the carried history and phase
        H = -(-K // M) * M - D
        cut = 5 * D
        for fn in (O.definition, O.polyphase64):
            two = np.concatenate([fn(x[:cut], h, M, OS), fn(x[cut:], h, M, OS, hops0=5, history=_carried(x, cut, H))], axis=1)
            assert R.rel_err(two, d) <= 1e-12, (M, OS, K, fn.__name__)


@pytest.mark.parametrize("M", [8, 16, 64])
def test_oversampling_one_is_the_maximally_decimated_bank(M):
    F = 13
    x = R.stream(F * M, M, seed=M)
    for K in _taps(M, 1):
        h = R.prototype(M, K)
        d = R.definition(x, h, M)
        assert R.rel_err(O.definition(x, h, M, 1), d) <= 1e-12, (M, K)
        assert R.rel_err(O.polyphase64(x, h, M, 1), d) <= 1e-12, (M, K)
        H = (-(-K // M) - 1) * M
        cut = 5 * M
        hist = _carried(x, cut, H)
        for fn in (O.definition, O.polyphase64):
            assert R.rel_err(fn(x[cut:], h, M, 1, hops0=5, history=hist), d[:, 5:]) <= 1e-12, (M, K, fn.__name__)


@pytest.mark.parametrize("OS", [2, 4])
def test_a_tone_beyond_the_critically_sampled_edge_keeps_its_gain(OS):
    """(c + 0.4) / M lies in channel c's passband and aliases onto the band edge of a maximally decimated row; the oversampled
    row carries it with the prototype's own gain there"""
    M, K, c = 16, 8 * 16, 5
    D = M // OS
    h = R.prototype(M, K)
    n = 40 * M
    x = np.exp(2j * np.pi * ((c + 0.4) / M) * np.arange(n))
    y = O.polyphase64(x, h, M, OS)
    gain = abs(np.sum(h.astype(np.float64) * np.exp(-2j * np.pi * 0.4 * np.arange(K) / M)))
    steady = y[c, -(-K // D):]                          # frames whose K taps all lie in the stream
    assert len(steady) > 8
    assert np.abs(np.abs(steady) - gain).max() <= 1e-6 * gain
    # and at the rate it is sampled, M / D per channel width, the tone sits at 0.4 / OS cycles per output: no fold
    step = steady[1:] / steady[:-1]
    assert np.abs(step - np.exp(2j * np.pi * 0.4 / OS)).max() <= 1e-6


def test_oversampled_channelizer_has_no_cpu_fallback():
    import libtsd_amd as t
    for s in ("create_oversampled", "hop", "get_phase", "set_phase"):
        assert hasattr(t.lib(), "tsdgpu_channelizer_" + s), s
    chan = t.Channelizer
    if t.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(t.TsdGpuError):
        chan(R.prototype(8, 17), 8, oversample=2)


@pytest.mark.skipif(not os.path.isdir(REF) or shutil.which("g++") is None,
                    reason="needs the reference tree and g++ (build container only)")
def test_oversampled_adaptor_compiles_against_reference_headers(tmp_path):
    """gpu_canaliseur.cc, unchanged, against libtsd's own headers (the compiler line of test_channelizer_cpu.py)."""
    import torch
    inc = os.path.join(os.path.dirname(torch.__file__), "include")
    cmd = ["g++", "-std=c++20", "-O0", "-w", "-DFMT_HEADER_ONLY=1", "-DLIBTSD_USE_PNG=0", "-DLIBTSD_USE_FREETYPE=0",
           "-DLIBTSD_USE_GTKMM=0", f"-I{REF}/include", f"-I{inc}", f"-I{HOST}/include_ext", f"-I{ROOT}/include", "-c",
           f"{HOST}/adaptors/gpu_canaliseur.cc", "-o", str(tmp_path / "gpu_canaliseur.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    syms = subprocess.run(["nm", "-C", "--defined-only", str(tmp_path / "gpu_canaliseur.o")], capture_output=True, text=True).stdout
    three = [l for l in syms.splitlines() if "tsd_amd::canaliseur_polyphase(" in l and l.count(",") == 2]
    assert three, syms
