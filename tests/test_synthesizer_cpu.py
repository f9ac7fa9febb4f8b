"""Polyphase synthesizer (include/tsdgpu.h: tsdgpu_synthesizer), the parts that need no GPU: the two float64 references of
tests/syn_ref.py against each other, the synthesis bank against the analysis bank of tests/chan_ref.py, the exported symbols and
the absence of a CPU fallback, and the adaptor compiled against libtsd's own headers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import chan_ref
import syn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "libtsd_amd", "host")
REF = "/root/reference/core"


@pytest.mark.parametrize("M", [8, 16])
def test_definition_and_fast_form_agree(M):
    F = 12
    u = R.rows(M, F, seed=M)
    for K in (1, M - 1, M, M + 1, 3 * M - 3):
        f = R.prototype(M, K)
        d, s = R.definition(u, f), R.synth64(u, f)
        assert d.shape == s.shape == (F * M,)
        assert R.rel_err(s, d) <= 1e-12, (M, K)
        # the run split in two steps, the second from the carried history: the last P - 1 input frames
        PW = -(-K // M) - 1
        cut = 5
        hist = np.concatenate([np.zeros((M, PW), np.complex64), u[:, :cut]], axis=1)[:, cut:cut + PW]
        for fn in (R.definition, R.synth64):
            two = np.concatenate([fn(u[:, :cut], f), fn(u[:, cut:], f, hist)])
            assert R.rel_err(two, d) <= 1e-12, (M, K, fn.__name__)


@pytest.mark.parametrize("M", [8, 16, 64])
def test_synthesis_inverts_analysis_with_inverse_taps(M):
    """K = M: the analysis bank weights sample s of a frame with h[M - 1 - s] and transforms; f[s] = 1 / (M h[M - 1 - s]) undoes
    both.  Pins the two banks' conventions (channel order, sign of the exponent, frame alignment) to each other."""
    F = 9
    h = chan_ref.prototype(M, M).astype(np.float64)
    f = 1.0 / (M * h[::-1])
    x = chan_ref.stream(F * M, M, seed=M).astype(np.complex128)
    back = R.synth64(chan_ref.polyphase64(x, h, M), f)
    assert R.rel_err(back, x) <= 1e-12


def test_single_row_gives_a_tone_with_the_branch_sums_as_gain():
    M, K, F, c = 16, 40, 30, 5
    f = R.prototype(M, K)
    P = -(-K // M)
    u = np.zeros((M, F), np.complex64)
    u[c] = 1.0
    x = R.synth64(u, f)
    fp = np.zeros(P * M)
    fp[:K] = f
    gain = fp.reshape(P, M).sum(axis=0)                       # sum_j f[j M + s]
    p = np.arange((P - 1) * M, F * M)                         # past the start-up of P - 1 frames
    want = np.exp(2j * np.pi * c * p / M) * gain[p % M]
    assert np.abs(x[p] - want).max() <= 1e-12 * np.abs(want).max()


def test_synthesizer_has_no_cpu_fallback():
    import libtsd_amd as t
    for s in ("create", "out_count", "step", "reset", "history_len", "get_state", "set_state", "destroy"):
        assert hasattr(t.lib(), "tsdgpu_synthesizer_" + s), s
    syn = t.Synthesizer                      # (the class exists whether or not a GPU does)
    if t.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(t.TsdGpuError):
        syn(R.prototype(8, 17), 8)


@pytest.mark.skipif(not os.path.isdir(REF) or shutil.which("g++") is None,
                    reason="needs the reference tree and g++ (build container only)")
def test_synthesizer_adaptor_compiles_against_reference_headers(tmp_path):
    """gpu_synthetiseur.cc, unchanged, against libtsd's own headers (the compiler line of test_channelizer_cpu.py)."""
    import torch
    inc = os.path.join(os.path.dirname(torch.__file__), "include")
    cmd = ["g++", "-std=c++20", "-O0", "-w", "-DFMT_HEADER_ONLY=1", "-DLIBTSD_USE_PNG=0", "-DLIBTSD_USE_FREETYPE=0",
           "-DLIBTSD_USE_GTKMM=0", f"-I{REF}/include", f"-I{inc}", f"-I{HOST}/include_ext", f"-I{ROOT}/include", "-c",
           f"{HOST}/adaptors/gpu_synthetiseur.cc", "-o", str(tmp_path / "gpu_synthetiseur.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    syms = subprocess.run(["nm", "-C", "--defined-only", str(tmp_path / "gpu_synthetiseur.o")], capture_output=True, text=True).stdout
    assert "tsd_amd::synthetiseur_polyphase" in syms
