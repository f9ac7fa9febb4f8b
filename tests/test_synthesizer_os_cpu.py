"""Oversampled polyphase synthesizer (include/tsdgpu.h: tsdgpu_synthesizer_create_oversampled), the parts that need no GPU: the
two float64 references of tests/syn_os_ref.py against each other and against syn_ref at OS = 1, the reconstruction of a stream
through the oversampled analysis bank of tests/chan_os_ref.py (the reason the operator exists), the exported symbols and the
absence of a CPU fallback, and the adaptor compiled against libtsd's own headers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import chan_os_ref
import chan_ref
import syn_os_ref as R
import syn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "libtsd_amd", "host")
REF = "/root/reference/core"


def _tap_counts(M, OS):
    D = M // OS
    return sorted({1, max(D - 1, 1), D + 1, M + 1, 3 * M - 3, 16 * D})


@pytest.mark.parametrize("OS", [2, 4])
@pytest.mark.parametrize("M", [8, 16, 64])
def test_definition_and_fast_form_agree(M, OS):
    F, D, cut = 13, M // OS, 5
    u = R.rows(M, F, seed=M + OS)
    for K in _tap_counts(M, OS):
        f = R.prototype(M, K)
        d, s = R.definition(u, f, M, OS), R.synth64(u, f, M, OS)
        assert d.shape == s.shape == (F * D,)
        assert R.rel_err(s, d) <= 1e-12, (M, OS, K)
        # the run split at frame 5, the second step from the carried history (the last Q - 1 input frames) and 5 hops consumed
        QW = -(-K // D) - 1
        hist = np.concatenate([np.zeros((M, QW), np.complex64), u[:, :cut]], axis=1)[:, cut:cut + QW]
        for fn in (R.definition, R.synth64):
            two = np.concatenate([fn(u[:, :cut], f, M, OS), fn(u[:, cut:], f, M, OS, hops0=cut, history=hist)])
            assert R.rel_err(two, d) <= 1e-12, (M, OS, K, fn.__name__)


@pytest.mark.parametrize("M", [8, 16, 64])
def test_oversample_one_is_the_plain_reference(M):
    F = 13
    u = R.rows(M, F, seed=M)
    for K in _tap_counts(M, 1):
        f = R.prototype(M, K)
        want = syn_ref.synth64(u, f)
        assert R.rel_err(R.synth64(u, f, M, 1), want) <= 1e-12, (M, K)
        assert R.rel_err(R.definition(u, f, M, 1), want) <= 1e-12, (M, K)


def sine_window(M):
    """h[k] = sin(pi (k + 1/2) / M), k < M, in float32, and f = h reversed: analysed at hop M / OS and resynthesised, a stream comes
    back as (M OS / 2) x[p - M] (the window's squares at hop M / 2 sum to 1, at hop M / 4 to 2; the transform pair gives M)"""
    h = np.sin(np.pi * (np.arange(M) + 0.5) / M).astype(np.float32)
    return h, np.ascontiguousarray(h[::-1])


def reconstruction_error(x, rows, f, M, OS, delay):
    """rows delayed by `delay` frames (zero columns in front), synthesised in float64, against (M OS / 2) x[p - M] past the first 2 M
    samples, relative to the peak"""
    F = rows.shape[1]
    ud = np.concatenate([np.zeros((M, delay), rows.dtype), rows], axis=1)[:, :F]
    back = R.synth64(ud, f, M, OS)
    want = (M * OS / 2) * np.concatenate([np.zeros(M, np.complex128), np.asarray(x, np.complex128)])[: len(back)]
    return np.abs(back - want)[2 * M:].max() / np.abs(want).max()


@pytest.mark.parametrize("OS", [2, 4])
@pytest.mark.parametrize("M", [16, 64])
def test_sine_window_pair_reconstructs_the_stream(M, OS):
    F, D = 60, M // OS
    h, f = sine_window(M)
    rng = np.random.default_rng(M + OS)
    x = rng.standard_normal(F * D) + 1j * rng.standard_normal(F * D)
    y = chan_os_ref.polyphase64(x, h, M, OS)
    err = reconstruction_error(x, y, f, M, OS, 1)
    print(f"M={M} OS={OS}: {err:.2e}")
    assert err <= 1e-6                            # float64 arithmetic; what is left is the float32 rounding of the taps
    if OS == 2:
        # the frame alignment is part of the convention: no delay, or two frames, do not reconstruct
        assert reconstruction_error(x, y, f, M, OS, 0) > 1e-2
        assert reconstruction_error(x, y, f, M, OS, 2) > 1e-2


def test_oversampled_synthesizer_has_no_cpu_fallback():
    import libtsd_amd as t
    for s in ("create_oversampled", "hop", "get_phase", "set_phase"):
        assert hasattr(t.lib(), "tsdgpu_synthesizer_" + s), s
    if t.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(t.TsdGpuError):
        t.Synthesizer(R.prototype(8, 17), 8, oversample=2)


@pytest.mark.skipif(not os.path.isdir(REF) or shutil.which("g++") is None,
                    reason="needs the reference tree and g++ (build container only)")
def test_synthesizer_adaptor_compiles_against_reference_headers(tmp_path):
    """gpu_synthetiseur.cc, unchanged, against libtsd's own headers (the compiler line of test_synthesizer_cpu.py): both factories"""
    import torch
    inc = os.path.join(os.path.dirname(torch.__file__), "include")
    cmd = ["g++", "-std=c++20", "-O0", "-w", "-DFMT_HEADER_ONLY=1", "-DLIBTSD_USE_PNG=0", "-DLIBTSD_USE_FREETYPE=0",
           "-DLIBTSD_USE_GTKMM=0", f"-I{REF}/include", f"-I{inc}", f"-I{HOST}/include_ext", f"-I{ROOT}/include", "-c",
           f"{HOST}/adaptors/gpu_synthetiseur.cc", "-o", str(tmp_path / "gpu_synthetiseur.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    syms = subprocess.run(["nm", "-C", "--defined-only", str(tmp_path / "gpu_synthetiseur.o")], capture_output=True, text=True).stdout
    three = [l for l in syms.splitlines() if "tsd_amd::synthetiseur_polyphase(" in l and l.count(", int") >= 2]
    assert three, syms[-2000:]
