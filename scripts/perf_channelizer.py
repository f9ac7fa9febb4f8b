#!/usr/bin/env python3
"""Polyphase channelizer (tsdgpu_channelizer) at n = 2^26 complex samples, M in {8, 64, 256, 1024} x K in {4 M, 8 M, 16 M}: ms per
step by HIP events (median of warm steps), the share of 8 TB/s on the algorithmic 16 B per sample, and beside each line the
yardstick Fft(M).step over the same 2^26 points (the same 16 B per point), the two interleaved in one process.  Kernel times
and launch counts: run under `rocprofv3 --kernel-trace --stats` with --quick (two steps per shape, no yardstick); traffic:
--quick --shapes 64x256,64x1024,1024x4096,1024x16384 under `rocprofv3 --pmc FETCH_SIZE WRITE_SIZE`, a run of its own."""
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
    shapes = [(M, m * M) for M in (8, 64, 256, 1024) for m in (4, 8, 16)]
    if "--shapes" in sys.argv:
        shapes = [tuple(int(v) for v in s.split("x")) for s in sys.argv[sys.argv.index("--shapes") + 1].split(",")]
    reps = 20
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(n, device=dev, generator=g, dtype=torch.complex64)
    y = torch.empty(n, device=dev, dtype=torch.complex64)
    for M, K in shapes:
        ch = t.Channelizer(prototype(M, K), M)
        ym = y.view(M, n // M)
        row = {"M": M, "K": K, "P": -(-K // M), "n": n}
        if quick:
            ch.step(x, ym)
            ch.step(x, ym)
            torch.cuda.synchronize()
            print(json.dumps(row), flush=True)
            ch.close()
            continue
        plan = t.Fft(M)
        xb = x.view(n // M, M)
        yb = y.view(n // M, M)
        for _ in range(3):
            ch.step(x, ym)
            plan.step(xb, True, yb)
        torch.cuda.synchronize()
        tc, tf = [], []
        for _ in range(reps):                      # the candidates interleaved
            tc.append(event_ms(lambda: ch.step(x, ym)))
            tf.append(event_ms(lambda: plan.step(xb, True, yb)))
        mc, mf = float(np.median(tc)), float(np.median(tf))
        row.update({"chan_ms": round(mc, 4), "frac_8TBs": round(16 * n / (mc * 1e-3) / 8e12, 3), "fft_ms": round(mf, 4),
                    "fft_frac_8TBs": round(16 * n / (mf * 1e-3) / 8e12, 3), "chan_over_fft": round(mc / mf, 3)})
        print(json.dumps(row), flush=True)
        ch.close()
        plan.close()


if __name__ == "__main__":
    main()
