#!/usr/bin/env python3
"""Host cost of the small calls of csrc/ola.hip, data resident: one-block Ola.step at the three fused geometries, a half-block step
(samples only buffered on every other call), a five-segment welch, a one-block Spectrum.step.  Per case five repetitions of a timed
loop (LOOP calls, one synchronize at the end), wall microseconds per call; the line gives the five and their median.
TSDGPU_LIB selects the build (scripts/build_variant.sh)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import libtsd_amd as t  # noqa: E402

LOOP, WARM, REPS = 1000, 100, 5


def hann(n):
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)).astype(np.float32)


def randc(n):
    return torch.view_as_complex(torch.randn(n, 2, device="cuda", generator=torch.Generator(device="cuda").manual_seed(n)))


def five(name, fn):
    for _ in range(WARM):
        fn()
    us = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(LOOP):
            fn()
        torch.cuda.synchronize()
        us.append(round((time.perf_counter() - t0) / LOOP * 1e6, 2))
    print(json.dumps({"case": name, "us_per_call": us, "median": sorted(us)[REPS // 2]}), flush=True)


def ola_case(name, Ne, nz, windowed, n):
    g = t.Ola(Ne, nz, hann(Ne) if windowed else None)
    g.set_response(np.ones(g.N, np.complex64))
    x, y = randc(n), torch.empty(Ne, dtype=torch.complex64, device="cuda")
    five(name, lambda: g.step(x, y))
    g.close()


def main():
    ola_case("ola step 512/127 one block", 512, 127, False, 512)
    ola_case("olaw step 512/0 one block", 512, 0, True, 512)
    ola_case("ola step 2048/127 one block", 2048, 127, False, 2048)
    ola_case("ola step 512/127 half block", 512, 127, False, 256)
    x, w = randc(5120), hann(1024)
    five("welch N=1024 n=5120", lambda: t.welch(x, 1024, w))
    s = t.Spectrum(1024, 1, 2, hann(1024))
    xs, ys = randc(1024), torch.empty((1, 1024), dtype=torch.float32, device="cuda")
    five("spectrum step 1024/1/2 one block", lambda: s.step(xs, ys))
    s.close()


if __name__ == "__main__":
    main()
