"""The 2x oversampled channelizer against the critically sampled one, timed in the same process: M = 256 channels, K = 2048 taps
(P = 8), n = 2^25 input samples (2^26 points written), HIP events, median of 20 warm steps, the candidates interleaved.

Two yardsticks, both Channelizer(h, 256) with P = 8:
 - over the same n = 2^25 samples.  What a user could build before is two such launches on delayed copies of the stream plus an
   interleave, so the oversampled step must take less than 2 x that: a condition, not a measurement.
 - over 2^26 samples: the same number of frames, transforms, multiply-adds and stores as the oversampled step.  Measured on one
   MI355X (profiles/r10_perf_channelizer_os.txt): oversampled 0.2259 ms, critical 0.2343 ms, MEASURED_RATIO = t_os /
   t_critical(2^26) = 0.964.  The guard asks for t_os <= 1.25 x MEASURED_RATIO x t_critical(2^26): the 25 % covers the spread
   between boxes and a busy box.

The guard's own runs, fresh processes (oversampled; critical over n, x 2; critical over 2^26, ratio):
    0.2456 ms;  0.1310 ms, 0.2621 ms;  0.2487 ms, 0.988
    0.2409 ms;  0.1311 ms, 0.2623 ms;  0.2456 ms, 0.981
    0.2410 ms;  0.1312 ms, 0.2625 ms;  0.2468 ms, 0.977
    0.2507 ms;  0.1341 ms, 0.2682 ms;  0.2494 ms, 1.005
    0.2455 ms;  0.1276 ms, 0.2552 ms;  0.2363 ms, 1.039
The first condition holds by 4-8 %.  This shape's window takes its kernel over 128 VGPRs, one workgroup per CU, where the critically
sampled P = 8 kernel has two; what carries it is the load-ahead of the next unit under the transform.  Without
it the same condition was met by 1 % in one run and missed by 3.6 % in another."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu_perf
MEASURED_RATIO = 0.964        # t_os / t_critical(2^26), profiles/r10_perf_channelizer_os.txt


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def test_oversampled_channelizer_against_the_critically_sampled_one():
    import torch
    import libtsd_amd as t
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box")       # (as test_perf_guards.py: `-m gpu_perf` runs there)
    M, K, OS, npts = 256, 2048, 2, 1 << 26
    n = npts // OS
    k = np.arange(K) - (K - 1) / 2
    h = (np.sinc(k / M) / M * np.hanning(K + 2)[1:-1]).astype(np.float32)
    x = torch.randn(npts, device="cuda", dtype=torch.complex64)
    y = torch.empty_like(x)
    ch, crit_n, crit = t.Channelizer(h, M, oversample=OS), t.Channelizer(h, M), t.Channelizer(h, M)
    ym, yh, xo = y.view(M, npts // M), y[:n].view(M, n // M), x[:n]
    for _ in range(3):
        ch.step(xo, ym)
        crit_n.step(xo, yh)
        crit.step(x, ym)
    torch.cuda.synchronize()
    to, tn, tc = [], [], []
    for _ in range(20):
        to.append(_event_ms(lambda: ch.step(xo, ym)))
        tn.append(_event_ms(lambda: crit_n.step(xo, yh)))
        tc.append(_event_ms(lambda: crit.step(x, ym)))
    t_os, t_n, t_c = float(np.median(to)), float(np.median(tn)), float(np.median(tc))
    print(f"oversampled {t_os:.4f} ms, critical over n {t_n:.4f} ms (x2 = {2 * t_n:.4f}), critical over 2^26 {t_c:.4f} ms, "
          f"ratio {t_os / t_c:.3f} (measured {MEASURED_RATIO})")
    assert t_os < 2 * t_n, (t_os, t_n)
    assert t_os <= 1.25 * MEASURED_RATIO * t_c, (t_os, t_c, MEASURED_RATIO)
