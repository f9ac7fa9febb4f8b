#!/usr/bin/env python3
"""Oversampled real-input polyphase channelizer (tsdgpu_channelizer_create_real_oversampled), M in {16, 64, 256, 1024} x (OS, K) in
{(2, 4 D), (2, 16 D), (4, 4 D), (4, 16 D)} (D = M / OS the hop), n = 2^26 / OS real samples per step so that 2^26 / 2 points (and
the Nyquist row) are written: ms per step by HIP events (median of 20 warm steps) and the share of 8 TB/s on the algorithmic
4 + 8 OS (M / 2 + 1) / M bytes per input sample.  Beside each line, interleaved in the same process:
  cplx_ms   the yardstick, what a user could do before: Channelizer(h, M, oversample=OS).step on the same stream already widened to
            complex64 (8 + 8 OS B per sample; the widening pass is NOT timed).
--quick: two steps per shape and no yardstick (for a profiler); --shapes MxOSxK,...; --log2n L."""
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
    npts = 1 << 26                                 # points the complex yardstick writes per step
    if "--log2n" in sys.argv:
        npts = 1 << int(sys.argv[sys.argv.index("--log2n") + 1])
    shapes = [(M, OS, m * (M // OS)) for M in (16, 64, 256, 1024) for OS in (2, 4) for m in (4, 16)]
    if "--shapes" in sys.argv:                     # M x OS x K
        shapes = [tuple(int(v) for v in s.split("x")) for s in sys.argv[sys.argv.index("--shapes") + 1].split(",")]
    reps = 20
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(npts // 2, device=dev, generator=g, dtype=torch.float32)
    xc = None if quick else x.to(torch.complex64)                      # the widening pass: not timed
    y = torch.empty(npts, device=dev, dtype=torch.complex64)            # room for M rows of n / D
    for M, OS, K in shapes:
        n, F, C = npts // OS, npts // M, M // 2 + 1
        ch = t.RealChannelizer.oversampled(prototype(M, K), M, OS)
        xo, yr = x[:n], y[: C * F].view(C, F)
        bytes_per_sample = 4 + 8 * OS * C / M
        row = {"M": M, "OS": OS, "K": K, "P": -(-K // M), "n": n}
        if quick:
            ch.step(xo, yr)
            ch.step(xo, yr)
            torch.cuda.synchronize()
            print(json.dumps(row), flush=True)
            ch.close()
            continue
        cc = t.Channelizer(prototype(M, K), M, oversample=OS)
        xw, ym = xc[:n], y.view(M, F)
        for _ in range(3):
            ch.step(xo, yr)
            cc.step(xw, ym)
        torch.cuda.synchronize()
        tr, tc = [], []
        for _ in range(reps):                      # the candidates interleaved
            tr.append(event_ms(lambda: ch.step(xo, yr)))
            tc.append(event_ms(lambda: cc.step(xw, ym)))
        mr, mc = float(np.median(tr)), float(np.median(tc))
        row.update({"real_ms": round(mr, 4), "frac_8TBs": round(bytes_per_sample * n / (mr * 1e-3) / 8e12, 3), "cplx_ms": round(mc, 4),
                    "real_over_cplx": round(mr / mc, 3)})
        print(json.dumps(row), flush=True)
        ch.close()
        cc.close()


if __name__ == "__main__":
    main()
