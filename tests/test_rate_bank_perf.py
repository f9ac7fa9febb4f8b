"""Rate-changing channel bank against the loop of single-stream steps it replaces: 256 channels of 4096 samples, resident data.
One bank step must be at least 10x faster than 256 PolyFir steps (each two launches of several microseconds)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu_perf


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


@pytest.mark.parametrize("which", ["decim_r4_k31", "ups_r2_k31"])
def test_rate_bank_step_beats_the_loop_of_single_steps(orc, which):
    import torch
    import libtsd_amd as t
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box")       # (as test_perf_guards.py: `-m gpu_perf` runs there)
    C, n = 256, 4096
    kind, Rr = (t.POLY_DECIM, 4) if which == "decim_r4_k31" else (t.POLY_UPS, 2)
    h = orc.design_rif_fen(31, "lp", 0.4 / Rr)
    x = torch.randn(C, n, device="cuda")
    bank, singles = t.PolyFirBank(kind, t.F32, C, h, Rr), [t.PolyFir(kind, t.F32, h, Rr) for _ in range(C)]
    y = torch.empty(C, bank.out_count(n), device="cuda")
    for _ in range(5):
        bank.step(x, y)
    t_bank = _median_ms(lambda: bank.step(x, y), 60)

    def loop():
        for c in range(C):
            singles[c].step(x[c])
    t_loop = _median_ms(loop, 7)
    print(f"{which}: bank {t_bank * 1e3:.1f} us, loop of {C} single steps {t_loop * 1e3:.1f} us, x{t_loop / t_bank:.0f}")
    assert t_bank * 10 <= t_loop, (t_bank, t_loop)
