#!/usr/bin/env python3
"""Polyphase synthesizer (tsdgpu_synthesizer) at n = 2^26 complex samples, M in {8, 64, 256, 1024} x K in {4 M, 8 M, 16 M}: ms per
step by HIP events (median of 20 warm steps), the share of 8 TB/s on the algorithmic 16 B per sample, and beside each line the
two yardsticks on the same shape, all three interleaved in one process: Fft(M).step over the same 2^26 points and
Channelizer.step, the analysis kernel that moves the same bytes the other way.  --quick: two steps per shape, no yardstick (for a
run under `rocprofv3 --kernel-trace --stats`)."""
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
        h = prototype(M, K)
        sy = t.Synthesizer(h, M)
        um = x.view(M, n // M)                         # the rows the synthesizer reads
        row = {"M": M, "K": K, "P": -(-K // M), "n": n}
        if quick:
            sy.step(um, y)
            sy.step(um, y)
            torch.cuda.synchronize()
            print(json.dumps(row), flush=True)
            sy.close()
            continue
        ch, plan = t.Channelizer(h, M), t.Fft(M)
        ym, xb, yb = y.view(M, n // M), x.view(n // M, M), y.view(n // M, M)
        for _ in range(3):
            sy.step(um, y)
            plan.step(xb, True, yb)
            ch.step(x, ym)
        torch.cuda.synchronize()
        ts, tf, tc = [], [], []
        for _ in range(reps):                      # the candidates interleaved
            ts.append(event_ms(lambda: sy.step(um, y)))
            tf.append(event_ms(lambda: plan.step(xb, True, yb)))
            tc.append(event_ms(lambda: ch.step(x, ym)))
        ms, mf, mc = float(np.median(ts)), float(np.median(tf)), float(np.median(tc))
        row.update({"synth_ms": round(ms, 4), "frac_8TBs": round(16 * n / (ms * 1e-3) / 8e12, 3), "fft_ms": round(mf, 4),
                    "chan_ms": round(mc, 4), "synth_over_fft": round(ms / mf, 3), "synth_over_chan": round(ms / mc, 3)})
        print(json.dumps(row), flush=True)
        sy.close()
        ch.close()
        plan.close()


if __name__ == "__main__":
    main()
