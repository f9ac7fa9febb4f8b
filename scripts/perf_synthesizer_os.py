#!/usr/bin/env python3
"""Oversampled polyphase synthesizer (tsdgpu_synthesizer_create_oversampled), M in {8, 64, 256, 1024} x OS in {2, 4} x Q in
{4, 16} taps per hop sample (K = Q D, D = M / OS the hop), F = 2^26 / M frames per step so that 2^26 points are read and
2^26 / OS samples written: ms per step by HIP events (median of 20 warm steps) and the share of 8 TB/s on the algorithmic
8 + 8 / OS bytes per point read.  Beside each line two yardsticks, interleaved in one process:
 (A) the critically sampled Synthesizer of the same M with P = Q taps per position over the same F frames: the same loads,
     transforms and register window, OS times the stores and, from D = 64, OS times the chains;
 (B) Fft(M).step over the same 2^26 points.
Traffic: --quick --shapes 256x2x1024 (two steps per shape, no yardstick) under `rocprofv3 --pmc FETCH_SIZE` and, in a run of its
own, `rocprofv3 --pmc WRITE_SIZE`, no tracing in either."""
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
    npts = 1 << 26                                 # points read per step
    if "--log2n" in sys.argv:
        npts = 1 << int(sys.argv[sys.argv.index("--log2n") + 1])
    shapes = [(M, OS, Q * (M // OS)) for M in (8, 64, 256, 1024) for OS in (2, 4) for Q in (4, 16)]
    if "--shapes" in sys.argv:                     # M x OS x K
        shapes = [tuple(int(v) for v in s.split("x")) for s in sys.argv[sys.argv.index("--shapes") + 1].split(",")]
    reps = 20
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    u = torch.randn(npts, device=dev, generator=g, dtype=torch.complex64)
    x = torch.empty(npts, device=dev, dtype=torch.complex64)
    for M, OS, K in shapes:
        D = M // OS
        F, Q = npts // M, -(-K // D)
        sy = t.Synthesizer(prototype(M, K), M, oversample=OS)
        um, xo = u.view(M, F), x[:F * D]
        row = {"M": M, "OS": OS, "K": K, "Q": Q, "F": F}
        if quick:
            sy.step(um, xo)
            sy.step(um, xo)
            torch.cuda.synchronize()
            print(json.dumps(row), flush=True)
            sy.close()
            continue
        crit, plan = t.Synthesizer(prototype(M, Q * M), M), t.Fft(M)      # (A): P = Q over the same frames; (B)
        ub, xb = u.view(F, M), x.view(F, M)
        for _ in range(3):
            sy.step(um, xo)
            crit.step(um, x)
            plan.step(ub, True, xb)
        torch.cuda.synchronize()
        to, tc, tf = [], [], []
        for _ in range(reps):                      # the candidates interleaved
            to.append(event_ms(lambda: sy.step(um, xo)))
            tc.append(event_ms(lambda: crit.step(um, x)))
            tf.append(event_ms(lambda: plan.step(ub, True, xb)))
        mo, mc, mf = float(np.median(to)), float(np.median(tc)), float(np.median(tf))
        row.update({"os_ms": round(mo, 4), "frac_8TBs": round((8 + 8 / OS) * npts / (mo * 1e-3) / 8e12, 3), "crit_ms": round(mc, 4),
                    "fft_ms": round(mf, 4), "os_over_crit": round(mo / mc, 3), "os_over_fft": round(mo / mf, 3)})
        print(json.dumps(row), flush=True)
        sy.close()
        crit.close()


if __name__ == "__main__":
    main()
