"""The real-input channelizer against what a user could do before it: Channelizer(h, M).step on the same stream already widened to
complex64 (the widening pass is not timed, so the yardstick is generous), in the same process: M = 256, K = 2048 (P = 8),
n = 2^26 real samples, HIP events, median of 20 warm steps, the two interleaved.  The real bank moves 4 + 8 (M / 2 + 1) / M B per
sample against 16 B: a ratio near 0.5 is the expectation.

Measured on one MI355X (profiles/r14_perf_rchannelizer.txt): MEASURED_RATIO below.  The guard asks for
t_real <= 1.25 x MEASURED_RATIO x t_complex: the 25 % covers the spread between boxes and a busy box."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu_perf
MEASURED_RATIO = 0.643        # t_real / t_complex, profiles/r14_perf_rchannelizer.txt


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def test_real_channelizer_beats_the_widened_complex_one():
    import torch
    import libtsd_amd as t
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box")       # (as test_perf_guards.py: `-m gpu_perf` runs there)
    M, K, n = 256, 2048, 1 << 26
    F, C = n // M, M // 2 + 1
    k = np.arange(K) - (K - 1) / 2
    h = (np.sinc(k / M) / M * np.hanning(K + 2)[1:-1]).astype(np.float32)
    x = torch.randn(n, device="cuda", dtype=torch.float32)
    xc = x.to(torch.complex64)
    y = torch.empty(n, device="cuda", dtype=torch.complex64)
    rc, cc = t.RealChannelizer(h, M), t.Channelizer(h, M)
    yr, ym = y[: C * F].view(C, F), y.view(M, F)
    for _ in range(3):
        rc.step(x, yr)
        cc.step(xc, ym)
    torch.cuda.synchronize()
    tr, tc = [], []
    for _ in range(20):
        tr.append(_event_ms(lambda: rc.step(x, yr)))
        tc.append(_event_ms(lambda: cc.step(xc, ym)))
    t_real, t_cplx = float(np.median(tr)), float(np.median(tc))
    print(f"real {t_real:.4f} ms, complex on the widened stream {t_cplx:.4f} ms, ratio {t_real / t_cplx:.3f} (measured {MEASURED_RATIO})")
    assert t_real <= 1.25 * MEASURED_RATIO * t_cplx, (t_real, t_cplx, MEASURED_RATIO)
