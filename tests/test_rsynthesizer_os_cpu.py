"""Oversampled real-output polyphase synthesizer (include/tsdgpu.h: tsdgpu_synthesizer_create_real_oversampled), the parts that
need no GPU: the float64 references of tests/rsyn_os_ref.py, the per-sample bound shown to discriminate on the tangled,
half-length scheme of synthesizer_real_os.hip, the analysis / synthesis round trip in float64, the exported symbol and the absence
of a CPU fallback, and the adaptor with both factories compiled against libtsd's own headers."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import chan_ref
import poly_f64 as PF
import rchan_os_ref
import rsyn_os_ref as RO
import syn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "libtsd_amd", "host")
REF = "/root/reference/core"
FRAMES = 120


# ------------------------------------------------------------------------------------------------------- 1. references
@pytest.mark.parametrize("OS", [2, 4])
@pytest.mark.parametrize("M", [16, 64])
def test_definition_and_fast_form_agree(M, OS):
    D, F, C = M // OS, 12, M // 2 + 1
    u = syn_ref.rows(M, F, seed=M + OS)[:C]
    for K in (1, D - 3, M + 1, 3 * M - 3):
        f = chan_ref.prototype(M, K)
        d = RO.definition(u, f, M, OS)
        assert d.shape == (F * D,) and d.dtype == np.float64
        for fn in (RO.synth64, RO.fast64):
            assert RO.rel_err(fn(u, f, M, OS), d) <= 1e-12, (M, OS, K, fn.__name__)
        # the run cut after an odd number of hops: the second part from the carried (M / 2 + 1, Q - 1) history and hops0
        Q, cut = -(-K // D), 5
        hist = np.concatenate([np.zeros((C, Q - 1), np.complex64), u[:, :cut]], axis=1)[:, cut:cut + Q - 1]
        for fn in (RO.definition, RO.synth64, RO.fast64):
            two = np.concatenate([fn(u[:, :cut], f, M, OS), fn(u[:, cut:], f, M, OS, cut, hist)])
            assert RO.rel_err(two, d) <= 1e-12, (M, OS, K, fn.__name__)
        # the phase matters: without hops0 the second part is another stream
        wrong = RO.fast64(u[:, cut:], f, M, OS, 0, hist)
        assert RO.rel_err(wrong, d[cut * D:]) > 1e-3, (M, OS, K)


def test_extended_block_gives_a_real_stream():
    """syn_os_ref.synth64 on the extended block: an imaginary part below 1e-12, the real part the fast form to 1e-9"""
    import syn_os_ref
    M, OS, F = 32, 4, 40
    rng = np.random.default_rng(5)
    u = RO.input(rng, M, F)
    f = PF.taps(rng, 5 * (M // OS) - 3)
    full = syn_os_ref.synth64(RO.extend(u), f, M, OS)
    peak = np.abs(full).max()
    assert np.abs(full.imag).max() <= 1e-12 * peak
    assert np.abs(full.real - RO.fast64(u, f, M, OS)).max() <= 1e-9 * peak


# ------------------------------------------------------------------------------------------- 2. the bound discriminates
@functools.lru_cache(maxsize=None)
def case(M, OS, Q):
    rng = np.random.default_rng([17, M, OS, Q])
    D = M // OS
    K = (Q - 1) * D + 1 + int(rng.integers(0, D - 1))
    f = PF.taps(rng, K)
    u = RO.input(rng, M, FRAMES)
    x64, bound = RO.f64_case(u, f, M, OS)
    ref = RO.fast64(u, f, M, OS)
    assert np.abs(ref - x64).max() <= 1e-9 * np.abs(ref).max()
    good = PF.syn_table(f, D)
    assert good.shape == (Q, D)
    # a branch whose newest tap is live: one frame late, its taps move (with Q = 1, the tap is dropped)
    s0 = int(rng.integers(min(K, D)))
    assert good[0, s0] != 0
    wrong = {name: RO.emulate32(u, tab, M, OS) for name, tab in PF.mutants(f, PF.syn_table, D, s0).items()}
    return K, x64, bound, RO.emulate32(u, good, M, OS), wrong


@pytest.mark.parametrize("Q", [1, 2, 16])
@pytest.mark.parametrize("OS", [2, 4])
@pytest.mark.parametrize("M", [16, 32, 64, 256, 1024])
def test_bound_discriminates(M, OS, Q):
    """a float32 emulation of the kernel's scheme (complex64 tangle, half-length complex64 transform, paired chains oldest first at
    the positions r) sits well inside the bound, three wrong banks outside it"""
    K, x64, bound, x32, wrong = case(M, OS, Q)
    assert x32.dtype == np.float32
    ratio = PF.syn_judge(x32, x64, bound, f"M={M} OS={OS} K={K}")
    print(f"M={M} OS={OS} Q={Q} K={K}: float32 emulation, worst err / bound {ratio:.3f}; zero-bound samples {int((bound == 0).sum())}")
    assert ratio <= 0.5
    assert len(wrong) == 3
    live = bound > 0
    for name, x in wrong.items():
        r = float((np.abs(x.astype(np.float64) - x64)[live] / bound[live]).max())
        print(f"M={M} OS={OS} Q={Q} K={K}: {name}, worst err / bound {r:.3g}")
        assert r > 1.0, (name, r)


# ------------------------------------------------------------------------------------------------------ 3. round trip
@pytest.mark.parametrize("OS", [2, 4])
@pytest.mark.parametrize("M", [16, 256])
def test_round_trip_identity_in_float64(M, OS):
    """rchan_os_ref.polyphase64 with the float32 sine window of length M -> the rows delayed by one frame -> the synthesis
    reference with f = h reversed: (M OS / 2) x[p - M] past the first 2 M samples, to 1e-6 of the peak (what is left is the
    float32 rounding of the window: 3.5e-8 ... 5.6e-8 measured)"""
    F, D = 60, M // OS
    h = np.sin(np.pi * (np.arange(M) + 0.5) / M).astype(np.float32)
    f = np.ascontiguousarray(h[::-1])
    x = np.random.default_rng(100 + M + OS).standard_normal(F * D).astype(np.float32)
    y = rchan_os_ref.polyphase64(x, h, M, OS)
    assert y.shape == (M // 2 + 1, F)
    delayed = np.concatenate([np.zeros((M // 2 + 1, 1), np.complex128), y[:, :F - 1]], axis=1)
    want = (M * OS / 2) * np.concatenate([np.zeros(M), x.astype(np.float64)])[:F * D]
    peak = np.abs(want).max()
    for fn in (RO.synth64, RO.fast64):
        err = np.abs(fn(delayed, f, M, OS) - want)[2 * M:].max() / peak
        print(f"M={M} OS={OS} {fn.__name__}: round trip {err:.2e} of the peak")
        assert err <= 1e-6, (M, OS, fn.__name__)


# ------------------------------------------------------------------------------------------------------ 4. no fallback
def test_oversampled_real_synthesizer_symbol_is_exported_and_declared():
    import libtsd_amd as t
    assert hasattr(t.lib(), "tsdgpu_synthesizer_create_real_oversampled")
    header = open(os.path.join(ROOT, "include", "tsdgpu.h")).read()
    assert "tsdgpu_synthesizer_create_real_oversampled(" in header


def test_oversampled_real_synthesizer_has_no_cpu_fallback():
    import libtsd_amd as t
    make = t.RealSynthesizer.oversampled     # (the classmethod exists whether or not a GPU does)
    assert isinstance(t.RealSynthesizer.phase, property) and t.RealSynthesizer.phase.fset is not None
    if t.device_count() > 0:
        return                               # (with a GPU the handle is made: tests/test_rsynthesizer_os_gpu.py)
    for OS in (1, 2, 4):
        with pytest.raises(t.TsdGpuError):
            make(chan_ref.prototype(16, 33), 16, OS)


@pytest.mark.skipif(not os.path.isdir(REF) or shutil.which("g++") is None,
                    reason="needs the reference tree and g++ (build container only)")
def test_adaptor_with_both_factories_compiles_against_reference_headers(tmp_path):
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
    defs = {ln.split(" ", 2)[2] for ln in syms.splitlines() if " T " in ln and "tsd_amd::synthetiseur_polyphase_reel(" in ln}
    assert len(defs) == 2, syms[-3000:]
    assert sum(d.rstrip().endswith(", int, int)") for d in defs) == 1, defs
