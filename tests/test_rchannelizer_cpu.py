"""Real-input polyphase channelizer (include/tsdgpu.h: tsdgpu_channelizer_create_real), the parts that need no GPU: the float64
references of tests/rchan_ref.py, the conjugate symmetry of the rows that are not produced, the untangling identity, the
per-frame bound shown to discriminate on the inputs the GPU tests use, the exported symbols and the absence of a CPU fallback,
and the adaptor compiled against libtsd's own headers."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import chan_ref
import poly_f64 as PF
import rchan_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "libtsd_amd", "host")
REF = "/root/reference/core"
FRAMES = 300


# ------------------------------------------------------------------------------------------------------- 1. references
@pytest.mark.parametrize("M", [16, 64])
def test_definition_and_fast_form_agree(M):
    F = 12
    x = R.stream(F * M, M, seed=M)
    assert x.dtype == np.float32
    for K in (1, M - 3, M + 1, 3 * M - 3):
        h = chan_ref.prototype(M, K)
        d, p = R.definition(x, h, M), R.polyphase64(x, h, M)
        assert d.shape == p.shape == (M // 2 + 1, F)
        assert R.rel_err(p, d) <= 1e-12, (M, K)
        # the run split in two steps, the second from the carried history of FLOATS
        H = (-(-K // M) - 1) * M
        cut = 5 * M
        hist = np.concatenate([np.zeros(H, np.float32), x[:cut]])[cut:cut + H] if H else None
        two = np.concatenate([R.polyphase64(x[:cut], h, M), R.polyphase64(x[cut:], h, M, hist)], axis=1)
        assert R.rel_err(two, d) <= 1e-12, (M, K)


# ----------------------------------------------------------------------------------------------- 2. conjugate symmetry
@pytest.mark.parametrize("M", [16, 256])
def test_dropped_rows_are_the_conjugates(M):
    K, F = 4 * M - 3, 20
    x = R.stream(F * M, M, seed=1)
    y = chan_ref.polyphase64(R.widen(x), chan_ref.prototype(M, K), M)
    N = M // 2
    diff = np.abs(y[N + 1:] - np.conj(y[N - 1:0:-1])).max()
    print(f"M={M}: max |y[M - c] - conj y[c]| = {diff:.2e}, peak {np.abs(y).max():.2e}")
    assert diff <= 1e-12 * np.abs(y).max()
    assert np.abs(y[[0, N]].imag).max() <= 1e-12 * np.abs(y).max()      # rows 0 and M / 2 are real


# ----------------------------------------------------------------------------------------------- 3. untangling identity
@pytest.mark.parametrize("M", [16, 32, 64, 128, 256, 512, 1024])
def test_untangling_reproduces_the_rfft(M):
    rng = np.random.default_rng(M)
    v = rng.standard_normal((7, M))
    got, want = R.untangle(v), np.fft.rfft(v, axis=1)
    assert got.shape == want.shape == (7, M // 2 + 1)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max() * np.log2(M)
    assert not got[:, [0, M // 2]].imag.any()                           # exactly real, not only nearly


# ------------------------------------------------------------------------------------------- 4. the bound discriminates
@functools.lru_cache(maxsize=None)
def case(M, P):
    rng = np.random.default_rng([14, M, P])
    K = R.two_tap_counts(rng, M, P)[0]
    h = PF.taps(rng, K)
    x = R.f64_input(rng, FRAMES * M, M)
    y64, bound = R.f64_case(x, h, M)
    good = PF.chan_table(h, M)
    # a branch whose newest tap is live: one frame late, its taps move (with P = 1, the tap is dropped)
    s0 = M - 1 - int(rng.integers(min(K, M)))
    assert good[0, s0] != 0
    wrong = {name: R.emulate32(x, tab, M) for name, tab in PF.mutants(h, PF.chan_table, M, s0).items()}
    return K, y64, bound, R.emulate32(x, good, M), wrong


@pytest.mark.parametrize("P", [1, 2, 3, 7, 16])
@pytest.mark.parametrize("M", [16, 32, 64, 128, 256, 2048])
def test_bound_discriminates(M, P):
    """a float32 emulation of the kernel's scheme sits well inside the bound, three wrong banks outside it"""
    K, y64, bound, y32, wrong = case(M, P)
    ratio = PF.chan_judge(y32, y64, bound, f"M={M} K={K}")
    print(f"M={M} P={P} K={K}: float32 emulation, worst err / bound {ratio:.3f}; zero-bound frames {int((bound == 0).sum())}")
    assert ratio <= 0.5
    assert len(wrong) == 3
    live = bound > 0
    for name, y in wrong.items():
        err = np.abs(y.astype(np.complex128) - y64).max(axis=0)
        r = float((err[live] / bound[live]).max())
        print(f"M={M} P={P} K={K}: {name}, worst err / bound {r:.3g}")
        assert r > 1.0, (name, r)


# ------------------------------------------------------------------------------------------------------ 5. no fallback
def test_real_channelizer_has_no_cpu_fallback():
    import libtsd_amd as t
    for s in ("create_real", "rows", "is_real", "step", "reset", "history_len", "get_state", "set_state", "out_count", "hop",
              "destroy"):
        assert hasattr(t.lib(), "tsdgpu_channelizer_" + s), s
    chan = t.RealChannelizer                 # (the class exists whether or not a GPU does)
    if t.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(t.TsdGpuError):
        chan(chan_ref.prototype(16, 33), 16)


@pytest.mark.skipif(not os.path.isdir(REF) or shutil.which("g++") is None,
                    reason="needs the reference tree and g++ (build container only)")
def test_real_channelizer_adaptor_compiles_against_reference_headers(tmp_path):
    """gpu_canaliseur_reel.cc, unchanged, against libtsd's own headers (the compiler line of test_channelizer_cpu.py)."""
    import torch
    inc = os.path.join(os.path.dirname(torch.__file__), "include")
    cmd = ["g++", "-std=c++20", "-O0", "-w", "-DFMT_HEADER_ONLY=1", "-DLIBTSD_USE_PNG=0", "-DLIBTSD_USE_FREETYPE=0",
           "-DLIBTSD_USE_GTKMM=0", f"-I{REF}/include", f"-I{inc}", f"-I{HOST}/include_ext", f"-I{ROOT}/include", "-c",
           f"{HOST}/adaptors/gpu_canaliseur_reel.cc", "-o", str(tmp_path / "gpu_canaliseur_reel.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    syms = subprocess.run(["nm", "-C", "--defined-only", str(tmp_path / "gpu_canaliseur_reel.o")], capture_output=True,
                          text=True).stdout
    assert "tsd_amd::canaliseur_polyphase_reel" in syms
