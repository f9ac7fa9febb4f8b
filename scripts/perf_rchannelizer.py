#!/usr/bin/env python3
"""Real-input polyphase channelizer (tsdgpu_channelizer_create_real) at n = 2^26 real samples per step, M in {16, 64, 256, 1024} x
K in {4 M, 8 M, 16 M}: ms per step by HIP events (median of 20 warm steps) and the share of 8 TB/s on the algorithmic
4 + 8 (M / 2 + 1) / M B per real sample.  Beside each line, interleaved in the same process:
  cplx_ms   the yardstick, what a user could do before: Channelizer(h, M).step on the same stream already widened to complex64
            (16 B per sample; the widening pass is NOT timed);
  half_ms   Channelizer(h', M / 2).step over the same input bytes (2^25 complex points, K / 2 taps: the same P): the kernel this
            one derives from.  Reported, not guarded.
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
    x = torch.randn(n, device=dev, generator=g, dtype=torch.float32)
    xc = None if quick else x.to(torch.complex64)                      # the widening pass: not timed
    y = torch.empty(n, device=dev, dtype=torch.complex64)               # room for M rows of n / M
    for M, K in shapes:
        F, C = n // M, M // 2 + 1
        ch = t.RealChannelizer(prototype(M, K), M)
        yr = y[: C * F].view(C, F)
        bytes_per_sample = 4 + 8 * C / M
        row = {"M": M, "K": K, "P": -(-K // M), "n": n}
        if quick:
            ch.step(x, yr)
            ch.step(x, yr)
            torch.cuda.synchronize()
            print(json.dumps(row), flush=True)
            ch.close()
            continue
        cc, hc = t.Channelizer(prototype(M, K), M), t.Channelizer(prototype(M // 2, K // 2), M // 2)
        ym, xh, yh = y.view(M, F), xc[: n // 2], y[: n // 2].view(M // 2, F)
        for _ in range(3):
            ch.step(x, yr)
            cc.step(xc, ym)
            hc.step(xh, yh)
        torch.cuda.synchronize()
        tr, tc, th = [], [], []
        for _ in range(reps):                      # the candidates interleaved
            tr.append(event_ms(lambda: ch.step(x, yr)))
            tc.append(event_ms(lambda: cc.step(xc, ym)))
            th.append(event_ms(lambda: hc.step(xh, yh)))
        mr, mc, mh = float(np.median(tr)), float(np.median(tc)), float(np.median(th))
        row.update({"real_ms": round(mr, 4), "frac_8TBs": round(bytes_per_sample * n / (mr * 1e-3) / 8e12, 3), "cplx_ms": round(mc, 4),
                    "real_over_cplx": round(mr / mc, 3), "half_ms": round(mh, 4), "real_over_half": round(mr / mh, 3)})
        print(json.dumps(row), flush=True)
        for o in (ch, cc, hc):
            o.close()


if __name__ == "__main__":
    main()
