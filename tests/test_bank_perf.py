"""Channel banks against the loop of single-stream steps they replace: 256 channels of 4096 samples, resident data.  One bank
step must be at least 10x faster than 256 single-stream steps (each a launch of several microseconds)."""
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


@pytest.mark.parametrize("which", ["fir31", "sos_cfg4"])
def test_bank_step_beats_the_loop_of_single_steps(orc, which):
    import torch
    import libtsd_amd as t
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box")       # (as test_perf_guards.py: `-m gpu_perf` runs there)
    C, n = 256, 4096
    x = torch.randn(C, n, device="cuda")
    y = torch.empty_like(x)
    if which == "fir31":
        h = orc.design_rif_fen(31, "lp", 0.25)
        bank, singles = t.FirBank(h, t.F32, C), [t.Fir(h, t.F32, t.FIR_DIRECT) for _ in range(C)]
    else:
        z, p, mn, md = orc.design_butter_lp(12, 0.25)
        co, gain, r1 = orc.SosChain(z, p, mn, md).coefs()
        bank, singles = t.SosBank(co, gain, t.F32, C, r1), [t.Sos(co, gain, t.F32, r1) for _ in range(C)]
    for _ in range(5):
        bank.step(x, y)
    t_bank = _median_ms(lambda: bank.step(x, y), 60)

    def loop():
        for c in range(C):
            singles[c].step(x[c], y[c])
    t_loop = _median_ms(loop, 7)
    print(f"{which}: bank {t_bank * 1e3:.1f} us, loop of {C} single steps {t_loop * 1e3:.1f} us, x{t_loop / t_bank:.0f}")
    assert t_bank * 10 <= t_loop, (t_bank, t_loop)
