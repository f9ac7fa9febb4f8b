#!/usr/bin/env python3
"""Real-output polyphase synthesizer (tsdgpu_synthesizer_create_real) at n = 2^26 real samples per step, M in {16, 64, 256, 1024} x
K in {4 M, 8 M, 16 M}: ms per step by HIP events (median of 20 warm steps) and the share of 8 TB/s on the algorithmic
8 (M / 2 + 1) / M + 4 B per real sample.  Beside each line, interleaved in the same process:
  cplx_ms   the yardstick, what a user could do before: Synthesizer(f, M).step on the (M, F) block already extended by the
            conjugate rows (16 B per sample; the extension pass is NOT timed);
  rchan_ms  RealChannelizer(f, M).step on the same shape, the other direction.  Reported, not guarded.
--quick: two steps per shape and no yardsticks (for a profiler); --shapes MxK,...; --log2n L."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import libtsd_amd as t  # noqa: E402


def prototype(M, K):
    k = np.arange(K) - (K - 1) / 2
    w = 0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(K) + 1) / (K + 1))
    return (np.sinc(k / M) / M * w).astype(np.float32)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    quick = "--quick" in sys.argv
    n = 1 << 26
    if "--log2n" in sys.argv:
        n = 1 << int(sys.argv[sys.argv.index("--log2n") + 1])
    shapes = [(M, m * M) for M in (16, 64, 256, 1024) for m in (4, 8, 16)]
    if "--shapes" in sys.argv:
        shapes = [tuple(int(v) for v in s.split("x")) for s in sys.argv[sys.argv.index("--shapes") + 1].split(",")]
    reps = 20
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    rows = torch.view_as_complex(torch.randn((n, 2), device=dev, generator=g, dtype=torch.float32))   # room for M rows of n / M
    x = torch.empty(n, device=dev, dtype=torch.float32)
    xc = None if quick else torch.empty(n, device=dev, dtype=torch.complex64)
    for M, K in shapes:
        F, N = n // M, M // 2
        C = N + 1
        sy = t.RealSynthesizer(prototype(M, K), M)
        bytes_per_sample = 8 * C / M + 4
        row = {"M": M, "K": K, "P": -(-K // M), "n": n}
        if quick:
            ur = rows[: C * F].view(C, F)
            sy.step(ur, x)
            sy.step(ur, x)
            torch.cuda.synchronize()
            print(json.dumps(row), flush=True)
            sy.close()
            continue
        um = rows.view(M, F)
        um[0].imag.zero_()                         # the extension pass: not timed
        um[N].imag.zero_()
        um[N + 1:] = torch.conj(torch.flip(um[1:N], dims=(0,)))
        ur = um[:C]
        cs, rc = t.Synthesizer(prototype(M, K), M), t.RealChannelizer(prototype(M, K), M)
        yr = xc[: C * F].view(C, F)
        for _ in range(3):
            sy.step(ur, x)
            cs.step(um, xc)
            rc.step(x, yr)
        torch.cuda.synchronize()
        tr, tc, ta = [], [], []
        for _ in range(reps):                      # the candidates interleaved
            tr.append(event_ms(lambda: sy.step(ur, x)))
            tc.append(event_ms(lambda: cs.step(um, xc)))
            ta.append(event_ms(lambda: rc.step(x, yr)))
        mr, mc, ma = float(np.median(tr)), float(np.median(tc)), float(np.median(ta))
        row.update({"real_ms": round(mr, 4), "frac_8TBs": round(bytes_per_sample * n / (mr * 1e-3) / 8e12, 3), "cplx_ms": round(mc, 4),
                    "real_over_cplx": round(mr / mc, 3), "rchan_ms": round(ma, 4), "real_over_rchan": round(mr / ma, 3)})
        print(json.dumps(row), flush=True)
        for o in (sy, cs, rc):
            o.close()


if __name__ == "__main__":
    main()
