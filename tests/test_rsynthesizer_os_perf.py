"""The oversampled real-output synthesizer against what a user could do before it: Synthesizer(f, M, oversample=OS).step on the block
already extended by the conjugate rows (the extension pass is not timed, so the yardstick is generous), in the same process:
M = 256, OS = 2, K = 8 D = 1024 (the shape test_synthesizer_os_perf.py guards), F = 2^26 / M frames, HIP events, median of 20 warm
steps, the two interleaved.  The real bank moves 8 (M / 2 + 1) / M + 4 / OS B per point against 8 + 8 / OS: a ratio near 0.5 is the
expectation.

MEASURED_RATIO is read from the committed measurement of one MI355X (profiles/r17_perf_rsynthesizer_os.txt), the line
of this shape.  The guard asks for t_real <= 1.25 x MEASURED_RATIO x t_complex (the 25 % covers the spread between boxes and a busy
box) and for t_real < t_complex in any case."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu_perf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = {"M": 256, "OS": 2, "K": 1024}


def measured_ratio():
    """real_over_cplx of SHAPE in the committed profile"""
    with open(os.path.join(ROOT, "profiles", "r17_perf_rsynthesizer_os.txt")) as f:
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


def test_oversampled_real_synthesizer_beats_the_complex_one_on_the_extended_block():
    import torch
    import libtsd_amd as t
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box")       # (as test_perf_guards.py: `-m gpu_perf` runs there)
    ratio = measured_ratio()
    M, OS, K = SHAPE["M"], SHAPE["OS"], SHAPE["K"]
    D, N = M // OS, M // 2
    F, C = (1 << 26) // M, N + 1
    k = np.arange(K) - (K - 1) / 2
    f = (np.sinc(k / M) / M * np.hanning(K + 2)[1:-1]).astype(np.float32)
    um = torch.randn((M, F), device="cuda", dtype=torch.complex64)
    um[0].imag.zero_()                         # the extension pass: not timed
    um[N].imag.zero_()
    um[N + 1:] = torch.conj(torch.flip(um[1:N], dims=(0,)))
    ur = um[:C]
    x = torch.empty(F * D, device="cuda", dtype=torch.float32)
    xc = torch.empty(F * D, device="cuda", dtype=torch.complex64)
    rs, cs = t.RealSynthesizer.oversampled(f, M, OS), t.Synthesizer(f, M, oversample=OS)
    for _ in range(3):
        rs.step(ur, x)
        cs.step(um, xc)
    torch.cuda.synchronize()
    tr, tc = [], []
    for _ in range(20):
        tr.append(_event_ms(lambda: rs.step(ur, x)))
        tc.append(_event_ms(lambda: cs.step(um, xc)))
    t_real, t_cplx = float(np.median(tr)), float(np.median(tc))
    print(f"real {t_real:.4f} ms, complex on the extended block {t_cplx:.4f} ms, ratio {t_real / t_cplx:.3f} (measured {ratio})")
    assert t_real <= 1.25 * ratio * t_cplx, (t_real, t_cplx, ratio)
    assert t_real < t_cplx, (t_real, t_cplx)
