"""The overlap-save FIR bank against the direct bank (the only bank before it), timed in the same process: C = 4096 channels
of n = 4096 samples, HIP events, median of 60 warm steps.

Measured on one MI355X (profiles/r7_perf_ols_bank.txt), direct / overlap-save:
  complex data, real taps, K = 127:  0.098 / 0.067 ms = 1.47  -> the guard asks for 1.23, halfway between 1 and the measurement
  real data, K = 127:                0.0565 / 0.0537 ms = 1.05 -- below 1.2: the real-data kernel moves 4-B rows and is not
                                     ahead enough at this tap count to carry a guard (AUTO keeps the direct scheme below 97
                                     real taps); it is guarded at the next tap count of the measured grid instead:
  real data, K = 255:                0.0946 / 0.0538 ms = 1.76  -> the guard asks for 1.38."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu_perf
CASES = {"c64_K127": (True, 127, 1.23), "f32_K255": (False, 255, 1.38)}


def _median_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


@pytest.mark.parametrize("which", list(CASES) + ["f32_K127_report"])
def test_overlap_save_bank_beats_the_direct_bank(orc, which):
    import torch
    import libtsd_amd as t
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box")       # (as test_perf_guards.py: `-m gpu_perf` runs there)
    cplx, K, factor = CASES.get(which, (False, 127, None))
    C, n = 4096, 4096
    x = torch.randn(C, n, device="cuda", dtype=torch.complex64 if cplx else torch.float32)
    y = torch.empty_like(x)
    h = orc.design_rif_fen(K, "lp", 0.1)
    dt = t.C64 if cplx else t.F32
    ols, direct = t.FirBank(h, dt, C, method=t.FIR_OVERLAP_SAVE), t.FirBank(h, dt, C, method=t.FIR_DIRECT)
    for _ in range(5):
        ols.step(x, y)
        direct.step(x, y)
    assert ols.method_used == t.FIR_OVERLAP_SAVE and direct.method_used == t.FIR_DIRECT
    t_ols = _median_ms(lambda: ols.step(x, y), 60)
    t_dir = _median_ms(lambda: direct.step(x, y), 60)
    print(f"{which}: direct bank {t_dir * 1e3:.1f} us, overlap-save bank {t_ols * 1e3:.1f} us, x{t_dir / t_ols:.2f}")
    if factor is not None:         # (real data at 127 taps: measured at 1.05 and reported above, no guard)
        assert t_ols * factor <= t_dir, (t_ols, t_dir, factor)
