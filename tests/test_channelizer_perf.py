"""The polyphase channelizer against the batched FFT of the same points, timed in the same process: M = 256 channels, K = 2048
taps (P = 8), n = 2^26 complex samples, HIP events, median of 20 warm steps, the two interleaved.  Both move 16 B per sample.

Measured on one MI355X (profiles/r8_perf_channelizer.txt): channelizer 0.2370 ms, Fft(256).step 0.2055 ms, ratio 1.153
(the guard itself, a fresh process on another box of the pool: 0.2586 / 0.1999 ms = 1.293).
The guard asks for t_channelizer <= 1.25 x 1.153 x t_fft: the 25 % covers the spread between boxes and a busy box; a lost
coalescing or a second pass over the data costs 50 % and more."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu_perf
MEASURED_RATIO = 1.153        # t_channelizer / t_fft, profiles/r8_perf_channelizer.txt


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def test_channelizer_stays_near_the_batched_fft():
    import torch
    import libtsd_amd as t
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box")       # (as test_perf_guards.py: `-m gpu_perf` runs there)
    M, K, n = 256, 2048, 1 << 26
    k = np.arange(K) - (K - 1) / 2
    h = (np.sinc(k / M) / M * np.hanning(K + 2)[1:-1]).astype(np.float32)
    x = torch.randn(n, device="cuda", dtype=torch.complex64)
    y = torch.empty_like(x)
    ch, plan = t.Channelizer(h, M), t.Fft(M)
    ym, xb, yb = y.view(M, n // M), x.view(n // M, M), y.view(n // M, M)
    for _ in range(3):
        ch.step(x, ym)
        plan.step(xb, True, yb)
    torch.cuda.synchronize()
    tc, tf = [], []
    for _ in range(20):
        tc.append(_event_ms(lambda: ch.step(x, ym)))
        tf.append(_event_ms(lambda: plan.step(xb, True, yb)))
    t_ch, t_fft = float(np.median(tc)), float(np.median(tf))
    print(f"channelizer {t_ch:.4f} ms, Fft({M}) {t_fft:.4f} ms, ratio {t_ch / t_fft:.3f} (measured {MEASURED_RATIO})")
    assert t_ch <= 1.25 * MEASURED_RATIO * t_fft, (t_ch, t_fft, MEASURED_RATIO)
