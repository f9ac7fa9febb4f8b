"""The oversampled real-input channelizer against what a user could do before it: Channelizer(h, M, oversample=OS).step on the same
stream already widened to complex64 (the widening pass is not timed, so the yardstick is generous), in the same process: M = 256,
OS = 2, K = 2048 (P = 8, the widest window), n = 2^25 real samples, HIP events, median of 20 warm steps, the two interleaved.  The
real bank moves 4 + 8 OS (M / 2 + 1) / M B per sample against 8 + 8 OS: a ratio near 0.5 is the expectation.

MEASURED_RATIO is read from the committed measurement of one MI355X (profiles/r16_perf_rchannelizer_os.txt), the line
of this shape.  The guard asks for t_real <= 1.25 x MEASURED_RATIO x t_complex: the 25 % covers the spread between boxes and a
busy box."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu_perf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = {"M": 256, "OS": 2, "K": 2048}


def measured_ratio():
    """real_over_cplx of SHAPE in the committed profile"""
    with open(os.path.join(ROOT, "profiles", "r16_perf_rchannelizer_os.txt")) as f:
        rows = [json.loads(ln) for ln in f if ln.startswith("{")]
    hit = [r for r in rows if all(r[k] == v for k, v in SHAPE.items())]
    assert len(hit) == 1, hit
    return float(hit[0]["real_over_cplx"])


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def test_oversampled_real_channelizer_beats_the_widened_complex_one():
    import torch
    import libtsd_amd as t
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box")       # (as test_perf_guards.py: `-m gpu_perf` runs there)
    ratio = measured_ratio()
    M, OS, K = SHAPE["M"], SHAPE["OS"], SHAPE["K"]
    n = (1 << 26) // OS
    F, C = n // (M // OS), M // 2 + 1
    k = np.arange(K) - (K - 1) / 2
    h = (np.sinc(k / M) / M * np.hanning(K + 2)[1:-1]).astype(np.float32)
    x = torch.randn(n, device="cuda", dtype=torch.float32)
    xc = x.to(torch.complex64)
    y = torch.empty(M * F, device="cuda", dtype=torch.complex64)
    rc, cc = t.RealChannelizer.oversampled(h, M, OS), t.Channelizer(h, M, oversample=OS)
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
    print(f"real {t_real:.4f} ms, complex on the widened stream {t_cplx:.4f} ms, ratio {t_real / t_cplx:.3f} (measured {ratio})")
    assert t_real <= 1.25 * ratio * t_cplx, (t_real, t_cplx, ratio)
