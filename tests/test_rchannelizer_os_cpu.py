"""Oversampled real-input polyphase channelizer (include/tsdgpu.h: tsdgpu_channelizer_create_real_oversampled), the parts that need
no GPU: the float64 references of tests/rchan_os_ref.py, the per-frame bound shown to discriminate on the paired, rotated scheme
of channelizer_real_os.hip, the exported symbol and the absence of a CPU fallback, and the adaptor with both factories compiled
against libtsd's own headers."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import chan_ref
import poly_f64 as PF
import rchan_os_ref as RO
import rchan_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "libtsd_amd", "host")
REF = "/root/reference/core"
FRAMES = 203


# ------------------------------------------------------------------------------------------------------- 1. references
@pytest.mark.parametrize("OS", [2, 4])
@pytest.mark.parametrize("M", [16, 64])
def test_definition_and_fast_form_agree(M, OS):
    D, F = M // OS, 12
    x = R.stream(F * D, M, seed=M + OS)
    for K in (1, D - 3, M + 1, 3 * M - 3):
        h = chan_ref.prototype(M, K)
        d, p = RO.definition(x, h, M, OS), RO.polyphase64(x, h, M, OS)
        assert d.shape == p.shape == (M // 2 + 1, F)
        assert R.rel_err(p, d) <= 1e-12, (M, OS, K)
        # the run split after an odd number of hops: the second part from the carried history of FLOATS and a non-zero hops0
        H = -(-K // M) * M - D
        cut = 5
        hist = np.concatenate([np.zeros(H, np.float32), x[:cut * D]])[cut * D:cut * D + H]
        for fn in (RO.definition, RO.polyphase64):
            two = np.concatenate([fn(x[:cut * D], h, M, OS), fn(x[cut * D:], h, M, OS, cut, hist)], axis=1)
            assert R.rel_err(two, d) <= 1e-12, (M, OS, K, fn.__name__)
        # the phase matters: without hops0 the second part is another stream
        wrong = RO.polyphase64(x[cut * D:], h, M, OS, 0, hist)
        assert R.rel_err(wrong, d[:, cut:]) > 1e-3, (M, OS, K)


# ------------------------------------------------------------------------------------------- 2. the bound discriminates
@functools.lru_cache(maxsize=None)
def case(M, OS, P):
    rng = np.random.default_rng([7, M, OS, P])
    K = (P - 1) * M + 1 + int(rng.integers(0, M - 1))
    h = PF.taps(rng, K)
    x = R.f64_input(rng, FRAMES * (M // OS), M)
    good = PF.chan_table(h, M)
    y64, bound = RO.f64_case(x, h, M, OS)
    ref = RO.polyphase64(x, h, M, OS)
    assert np.abs(ref - y64).max() <= 1e-9 * np.abs(ref).max()
    s0 = M - 1 - int(rng.integers(min(K, M)))
    assert good[0, s0] != 0
    wrong = {name: RO.emulate32(x, tab, M, OS) for name, tab in PF.mutants(h, PF.chan_table, M, s0).items()}
    return K, y64, bound, RO.emulate32(x, good, M, OS), wrong


@pytest.mark.parametrize("pp", ["1", "2", "16/OS"])
@pytest.mark.parametrize("OS", [2, 4])
@pytest.mark.parametrize("M", [16, 32, 64, 256, 1024])
def test_bound_discriminates(M, OS, pp):
    """a float32 emulation of the kernel's scheme (pairs rotated, half-length transform, untangling) sits well inside the bound,
    three wrong banks outside it"""
    P = {"1": 1, "2": 2, "16/OS": 16 // OS}[pp]
    K, y64, bound, y32, wrong = case(M, OS, P)
    ratio = PF.chan_judge(y32, y64, bound, f"M={M} OS={OS} K={K}")
    print(f"M={M} OS={OS} P={P} K={K}: float32 emulation, worst err / bound {ratio:.3f}; zero-bound frames {int((bound == 0).sum())}")
    assert ratio <= 0.5
    assert len(wrong) == 3
    live = bound > 0
    for name, y in wrong.items():
        err = np.abs(y.astype(np.complex128) - y64).max(axis=0)
        r = float((err[live] / bound[live]).max())
        print(f"M={M} OS={OS} P={P} K={K}: {name}, worst err / bound {r:.3g}")
        assert r > 1.0, (name, r)


# ------------------------------------------------------------------------------------------------------ 3. no fallback
def test_oversampled_real_channelizer_has_no_cpu_fallback():
    import libtsd_amd as t
    assert hasattr(t.lib(), "tsdgpu_channelizer_create_real_oversampled")
    make = t.RealChannelizer.oversampled     # (the classmethod exists whether or not a GPU does)
    assert isinstance(t.RealChannelizer.phase, property)
    if t.device_count() > 0:
        return
    for OS in (1, 2, 4):
        with pytest.raises(t.TsdGpuError):
            make(chan_ref.prototype(16, 33), 16, OS)


@pytest.mark.skipif(not os.path.isdir(REF) or shutil.which("g++") is None,
                    reason="needs the reference tree and g++ (build container only)")
def test_adaptor_with_both_factories_compiles_against_reference_headers(tmp_path):
    """gpu_canaliseur_reel.cc, unchanged, against libtsd's own headers (the compiler line of test_rchannelizer_cpu.py)."""
    import torch
    inc = os.path.join(os.path.dirname(torch.__file__), "include")
    cmd = ["g++", "-std=c++20", "-O0", "-w", "-DFMT_HEADER_ONLY=1", "-DLIBTSD_USE_PNG=0", "-DLIBTSD_USE_FREETYPE=0",
           "-DLIBTSD_USE_GTKMM=0", f"-I{REF}/include", f"-I{inc}", f"-I{HOST}/include_ext", f"-I{ROOT}/include", "-c",
           f"{HOST}/adaptors/gpu_canaliseur_reel.cc", "-o", str(tmp_path / "gpu_canaliseur_reel.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    syms = subprocess.run(["nm", "-C", "--defined-only", str(tmp_path / "gpu_canaliseur_reel.o")], capture_output=True,
                          text=True).stdout
    defs = {ln.split(" ", 2)[2] for ln in syms.splitlines() if " T " in ln and "tsd_amd::canaliseur_polyphase_reel(" in ln}
    assert len(defs) == 2, syms[-3000:]
    assert sum(d.rstrip().endswith(", int, int)") for d in defs) == 1, defs
