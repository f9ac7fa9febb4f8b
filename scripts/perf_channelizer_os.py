#!/usr/bin/env python3
"""Oversampled polyphase channelizer (tsdgpu_channelizer_create_oversampled), M in {8, 64, 256, 1024} x OS in {2, 4} x K in
{4 D, 16 D} (D = M / OS the hop), n = 2^26 / OS input samples per step so that 2^26 points are written: ms per step by HIP events
(median of 20 warm steps) and the share of 8 TB/s on the algorithmic 8 + 8 OS bytes per input sample (each sample read once, OS
points written per sample).  Beside each line the yardstick, interleaved in one process: the critically sampled Channelizer of
the same M and the same P = ceil(K / M) over 2^26 samples -- the same number of frames, transforms, multiply-adds and stores,
and OS times the reads.  Traffic: --quick --shapes 64x2x512,1024x2x8192 (two steps per shape, no yardstick) under
`rocprofv3 --pmc FETCH_SIZE` and, in a run of its own, `rocprofv3 --pmc WRITE_SIZE`, no tracing in either."""
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
    npts = 1 << 26                                 # points written per step
    if "--log2n" in sys.argv:
        npts = 1 << int(sys.argv[sys.argv.index("--log2n") + 1])
    shapes = [(M, OS, m * (M // OS)) for M in (8, 64, 256, 1024) for OS in (2, 4) for m in (4, 16)]
    if "--shapes" in sys.argv:                     # M x OS x K
        shapes = [tuple(int(v) for v in s.split("x")) for s in sys.argv[sys.argv.index("--shapes") + 1].split(",")]
    reps = 20
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(npts, device=dev, generator=g, dtype=torch.complex64)
    y = torch.empty(npts, device=dev, dtype=torch.complex64)
    for M, OS, K in shapes:
        n, P = npts // OS, -(-K // M)
        ch = t.Channelizer(prototype(M, K), M, oversample=OS)
        ym, xo = y.view(M, npts // M), x[:n]
        row = {"M": M, "OS": OS, "K": K, "P": P, "n": n}
        if quick:
            ch.step(xo, ym)
            ch.step(xo, ym)
            torch.cuda.synchronize()
            print(json.dumps(row), flush=True)
            ch.close()
            continue
        crit = t.Channelizer(prototype(M, P * M), M)            # the same P, over 2^26 samples: the same frames
        for _ in range(3):
            ch.step(xo, ym)
            crit.step(x, ym)
        torch.cuda.synchronize()
        to, tc = [], []
        for _ in range(reps):                      # the candidates interleaved
            to.append(event_ms(lambda: ch.step(xo, ym)))
            tc.append(event_ms(lambda: crit.step(x, ym)))
        mo, mc = float(np.median(to)), float(np.median(tc))
        row.update({"os_ms": round(mo, 4), "frac_8TBs": round((8 + 8 * OS) * n / (mo * 1e-3) / 8e12, 3), "crit_ms": round(mc, 4),
                    "crit_frac_8TBs": round(16 * npts / (mc * 1e-3) / 8e12, 3), "os_over_crit": round(mo / mc, 3)})
        print(json.dumps(row), flush=True)
        ch.close()
        crit.close()


if __name__ == "__main__":
    main()
