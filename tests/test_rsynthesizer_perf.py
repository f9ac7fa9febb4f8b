"""The real-output synthesizer against what a user could do before it: Synthesizer(f, M).step on the (M, F) block already extended by
the conjugate rows (the extension pass is not timed, so the yardstick is generous), in the same process: M = 256, K = 2048 (P = 8),
n = 2^26 real samples, HIP events, median of 20 warm steps, the two interleaved.  The real bank moves 8 (M / 2 + 1) / M + 4 B per
sample against 16 B: a ratio near 0.5 is the expectation.

Measured on one MI355X (profiles/r15_perf_rsynthesizer.txt): MEASURED_RATIO below.  The guard asks for
t_real <= 1.25 x MEASURED_RATIO x t_complex (the 25 % covers the spread between boxes and a busy box, as in
test_rchannelizer_perf.py), and in any case for t_real < t_complex."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu_perf
MEASURED_RATIO = 0.629        # t_real / t_complex, profiles/r15_perf_rsynthesizer.txt


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def test_real_synthesizer_beats_the_complex_one_on_the_extended_block():
    import torch
    import libtsd_amd as t
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box")       # (as test_perf_guards.py: `-m gpu_perf` runs there)
    M, K, n = 256, 2048, 1 << 26
    F, N = n // M, M // 2
    k = np.arange(K) - (K - 1) / 2
    f = (np.sinc(k / M) / M * np.hanning(K + 2)[1:-1]).astype(np.float32)
    um = torch.view_as_complex(torch.randn((n, 2), device="cuda", dtype=torch.float32)).view(M, F)
    um[0].imag.zero_()
    um[N].imag.zero_()
    um[N + 1:] = torch.conj(torch.flip(um[1:N], dims=(0,)))             # the extension pass: not timed
    ur = um[: N + 1]
    x = torch.empty(n, device="cuda", dtype=torch.float32)
    xc = torch.empty(n, device="cuda", dtype=torch.complex64)
    rs, cs = t.RealSynthesizer(f, M), t.Synthesizer(f, M)
    for _ in range(3):
        rs.step(ur, x)
        cs.step(um, xc)
    torch.cuda.synchronize()
    tr, tc = [], []
    for _ in range(20):
        tr.append(_event_ms(lambda: rs.step(ur, x)))
        tc.append(_event_ms(lambda: cs.step(um, xc)))
    t_real, t_cplx = float(np.median(tr)), float(np.median(tc))
    print(f"real {t_real:.4f} ms, complex on the extended block {t_cplx:.4f} ms, ratio {t_real / t_cplx:.3f} (measured {MEASURED_RATIO})")
    assert t_real < t_cplx, (t_real, t_cplx)
    assert t_real <= 1.25 * MEASURED_RATIO * t_cplx, (t_real, t_cplx, MEASURED_RATIO)
