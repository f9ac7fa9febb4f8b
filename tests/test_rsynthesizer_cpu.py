"""Real-output polyphase synthesizer (include/tsdgpu.h: tsdgpu_synthesizer_create_real), the parts that need no GPU: the float64
references of tests/rsyn_ref.py, the extension by conjugate rows, the per-sample bound shown to discriminate on the inputs the GPU
tests use, the analysis / synthesis round trip in float64, the exported symbols and the absence of a CPU fallback, and the adaptor
compiled against libtsd's own headers."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import chan_ref
import poly_f64 as PF
import rchan_ref
import rsyn_ref as R
import syn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "libtsd_amd", "host")
REF = "/root/reference/core"
FRAMES = 120


# ------------------------------------------------------------------------------------------------------- 1. references
@pytest.mark.parametrize("M", [16, 64])
def test_definition_and_fast_form_agree(M):
    F = 12
    u = syn_ref.rows(M, F, seed=M)[: M // 2 + 1]
    for K in (1, M - 3, M + 1, 3 * M - 3):
        f = chan_ref.prototype(M, K)
        d, p = R.definition(u, f), R.synth64(u, f)
        assert d.shape == p.shape == (F * M,) and d.dtype == np.float64
        assert R.rel_err(p, d) <= 1e-12, (M, K)
        # the run split in two steps, the second from the carried history of (M / 2 + 1, P - 1) input frames
        P, cut = -(-K // M), 5
        hist = np.concatenate([np.zeros((M // 2 + 1, P - 1), np.complex64), u[:, :cut]], axis=1)[:, cut:cut + P - 1]
        two = np.concatenate([R.synth64(u[:, :cut], f), R.synth64(u[:, cut:], f, hist)])
        assert R.rel_err(two, d) <= 1e-12, (M, K)


# ------------------------------------------------------------------------------------------------------- 2. extension
@pytest.mark.parametrize("M", [16, 256])
def test_extend_against_a_hermitian_block(M):
    """a block built Hermitian by hand, row by row, through syn_ref itself: its output is real, and extend() of its first
    M / 2 + 1 rows (their imaginary parts at rows 0 and M / 2 overwritten) is that block"""
    rng = np.random.default_rng(M)
    N, F, K = M // 2, 9, 3 * M - 3
    full = np.zeros((M, F), np.complex128)
    full[0], full[N] = rng.standard_normal(F), rng.standard_normal(F)
    for c in range(1, N):
        full[c] = rng.standard_normal(F) + 1j * rng.standard_normal(F)
        full[M - c] = np.conj(full[c])
    half = full[: N + 1].copy()
    half[0].imag = rng.standard_normal(F)                                # not used
    half[N].imag = np.nan
    assert np.array_equal(R.extend(half), full)
    f = chan_ref.prototype(M, K)
    x = syn_ref.synth64(full, f)
    assert np.abs(x.imag).max() <= 1e-12 * np.abs(x).max()
    assert R.rel_err(R.synth64(half, f), x.real) <= 1e-15
    assert np.isnan(half[N].imag).all()                                  # extend() copies: the caller's block is as it was


# ------------------------------------------------------------------------------------------- 3. the bound discriminates
@functools.lru_cache(maxsize=None)
def case(M, P):
    rng = np.random.default_rng([15, M, P])
    K = rchan_ref.two_tap_counts(rng, M, P)[0]
    f = PF.taps(rng, K)
    u = R.input(rng, M, FRAMES)
    x64, bound = R.f64_case(u, f, M)
    good = PF.syn_table(f, M)
    # a branch whose newest tap is live: one frame late, its taps move (with P = 1, the tap is dropped)
    s0 = int(rng.integers(min(K, M)))
    assert good[0, s0] != 0
    wrong = {name: R.emulate32(u, tab, M) for name, tab in PF.mutants(f, PF.syn_table, M, s0).items()}
    return K, x64, bound, R.emulate32(u, good, M), wrong


@pytest.mark.parametrize("P", [1, 5, 16])
@pytest.mark.parametrize("M", [16, 64, 1024])
def test_bound_discriminates(M, P):
    """a float32 emulation of the kernel's scheme sits well inside the bound, three wrong banks outside it"""
    K, x64, bound, x32, wrong = case(M, P)
    assert x32.dtype == np.float32
    ratio = PF.syn_judge(x32, x64, bound, f"M={M} K={K}")
    print(f"M={M} P={P} K={K}: float32 emulation, worst err / bound {ratio:.3f}; zero-bound samples {int((bound == 0).sum())}")
    assert ratio <= 0.5
    assert len(wrong) == 3
    live = bound > 0
    for name, x in wrong.items():
        r = float((np.abs(x.astype(np.float64) - x64)[live] / bound[live]).max())
        print(f"M={M} P={P} K={K}: {name}, worst err / bound {r:.3g}")
        assert r > 1.0, (name, r)


# ------------------------------------------------------------------------------------------------------ 4. round trip
@pytest.mark.parametrize("M", [16, 256])
def test_round_trip_identity_in_float64(M):
    """K <= M: every branch has one tap, and analysis then synthesis is x^[q M + s] = M f[s] h[M - 1 - s] x[q M + s]"""
    rng = np.random.default_rng(M + 1)
    F = 7
    x = rng.standard_normal(F * M).astype(np.float32)
    for K in (M, M - 5):
        h = (0.5 + rng.random(K)).astype(np.float32)
        f = (0.5 + rng.random(K)).astype(np.float32)
        hp, fp = np.zeros(M), np.zeros(M)
        hp[:K], fp[:K] = h, f
        y = rchan_ref.polyphase64(x, h, M)
        back = R.synth64(y, f)
        want = (M * fp * hp[::-1])[None, :] * x.reshape(F, M).astype(np.float64)
        assert np.abs(back - want.reshape(-1)).max() <= 1e-12 * np.abs(want).max(), (M, K)


# ------------------------------------------------------------------------------------------------------ 5. no fallback
def test_real_synthesizer_symbols_are_exported_and_declared():
    import libtsd_amd as t
    for s in ("create_real", "rows", "is_real", "step", "reset", "history_len", "get_state", "set_state", "out_count", "hop",
              "get_phase", "set_phase", "destroy"):
        assert hasattr(t.lib(), "tsdgpu_synthesizer_" + s), s
    header = open(os.path.join(ROOT, "include", "tsdgpu.h")).read()
    for s in ("create_real", "rows", "is_real"):
        assert "tsdgpu_synthesizer_" + s + "(" in header, s


def test_real_synthesizer_has_no_cpu_fallback():
    import libtsd_amd as t
    syn = t.RealSynthesizer                  # (the class exists whether or not a GPU does)
    if t.device_count() > 0:
        return                               # (with a GPU the handle is made: tests/test_rsynthesizer_gpu.py)
    with pytest.raises(t.TsdGpuError):
        syn(chan_ref.prototype(16, 33), 16)


@pytest.mark.skipif(not os.path.isdir(REF) or shutil.which("g++") is None,
                    reason="needs the reference tree and g++ (build container only)")
def test_real_synthesizer_adaptor_compiles_against_reference_headers(tmp_path):
    """gpu_synthetiseur_reel.cc, unchanged, against libtsd's own headers (the compiler line of test_rchannelizer_cpu.py)."""
    import torch
    inc = os.path.join(os.path.dirname(torch.__file__), "include")
    cmd = ["g++", "-std=c++20", "-O0", "-w", "-DFMT_HEADER_ONLY=1", "-DLIBTSD_USE_PNG=0", "-DLIBTSD_USE_FREETYPE=0",
           "-DLIBTSD_USE_GTKMM=0", f"-I{REF}/include", f"-I{inc}", f"-I{HOST}/include_ext", f"-I{ROOT}/include", "-c",
           f"{HOST}/adaptors/gpu_synthetiseur_reel.cc", "-o", str(tmp_path / "gpu_synthetiseur_reel.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    syms = subprocess.run(["nm", "-C", "--defined-only", str(tmp_path / "gpu_synthetiseur_reel.o")], capture_output=True,
                          text=True).stdout
    assert "tsd_amd::synthetiseur_polyphase_reel" in syms
