"""The polyphase synthesizer against the batched FFT of the same points, timed in the same process: M = 256 channels, K = 2048
taps (P = 8), n = 2^26 complex samples, HIP events, median of 20 warm steps, the two interleaved.  Both move 16 B per sample.

Fft(M).step over these points runs at the rate of a plain copy, so any composition of two passes over the data (a batched
inverse transform, then the polyphase filter) costs at least 2 t_fft.  The fused kernel has to beat that: the guard asks for
t_synth <= 2 t_fft.  The bound is the design's, not a measured ratio with a margin.

Measured on one MI355X (profiles/r9_perf_synthesizer.txt): synthesizer 0.3245 ms, Fft(256).step 0.2014 ms, ratio 1.611
(the guard itself, a fresh process on the same box: 0.3422 / 0.2001 ms = 1.710)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu_perf
BOUND = 2.0                   # t_synth / t_fft: the cheapest two-pass composition


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def test_synthesizer_beats_two_passes_of_the_batched_fft():
    import torch
    import libtsd_amd as t
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box")       # (as test_perf_guards.py: `-m gpu_perf` runs there)
    M, K, n = 256, 2048, 1 << 26
    k = np.arange(K) - (K - 1) / 2
    h = (np.sinc(k / M) / M * np.hanning(K + 2)[1:-1]).astype(np.float32)
    x = torch.randn(n, device="cuda", dtype=torch.complex64)
    y = torch.empty_like(x)
    sy, plan = t.Synthesizer(h, M), t.Fft(M)
    um, xb, yb = x.view(M, n // M), x.view(n // M, M), y.view(n // M, M)
    for _ in range(3):
        sy.step(um, y)
        plan.step(xb, True, yb)
    torch.cuda.synchronize()
    ts, tf = [], []
    for _ in range(20):
        ts.append(_event_ms(lambda: sy.step(um, y)))
        tf.append(_event_ms(lambda: plan.step(xb, True, yb)))
    t_sy, t_fft = float(np.median(ts)), float(np.median(tf))
    print(f"synthesizer {t_sy:.4f} ms, Fft({M}) {t_fft:.4f} ms, ratio {t_sy / t_fft:.3f} (bound {BOUND})")
    assert t_sy <= BOUND * t_fft, (t_sy, t_fft)
