#!/usr/bin/env python3
"""Oversampled real-output polyphase synthesizer (tsdgpu_synthesizer_create_real_oversampled), M in {16, 64, 256, 1024} x OS in
{2, 4} x Q in {4, 16} taps per hop sample (K = Q D, D = M / OS the hop), plus the shape tests/test_rsynthesizer_os_perf.py guards
(M = 256, OS = 2, K = 8 D).  F = 2^26 / M frames per step, so that 2^26 / 2 points and the Nyquist row are read and 2^26 / OS floats
written: ms per step by HIP events (median of 20 warm steps) and the share of 8 TB/s on the algorithmic 8 (M / 2 + 1) / M + 4 / OS
bytes per point of the extended block.  Beside each line two yardsticks this bank shares no kernel with, interleaved in one process:
  cplx_ms  (A) what a user could do before: Synthesizer(f, M, oversample=OS).step on the (M, F) block already extended by the
           conjugate rows (8 + 8 / OS B per point; the extension pass is NOT timed).  The bytes say x 0.5.
  crit_ms  (B) RealSynthesizer with P = Q taps per position over the same F frames: the same loads and transforms, OS times the
           stores and, from D = 128, OS times the chains.
Prints JSON lines, then a table.  --quick: two steps per shape and no yardsticks (for a profiler); --shapes MxOSxK,...; --log2n L."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import libtsd_amd as t  # noqa: E402

GUARDED = (256, 2, 8 * 128)


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
    npts = 1 << 26                                 # points of the extended block per step
    if "--log2n" in sys.argv:
        npts = 1 << int(sys.argv[sys.argv.index("--log2n") + 1])
    shapes = [(M, OS, Q * (M // OS)) for M in (16, 64, 256, 1024) for OS in (2, 4) for Q in (4, 16)] + [GUARDED]
    if "--shapes" in sys.argv:                     # M x OS x K
        shapes = [tuple(int(v) for v in s.split("x")) for s in sys.argv[sys.argv.index("--shapes") + 1].split(",")]
    reps = 20
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    rows = torch.view_as_complex(torch.randn((npts, 2), device=dev, generator=g, dtype=torch.float32))   # room for M rows of F
    x = torch.empty(npts, device=dev, dtype=torch.float32)
    xc = None if quick else torch.empty(npts // 2, device=dev, dtype=torch.complex64)
    table = []
    for M, OS, K in shapes:
        D, N = M // OS, M // 2
        F, Q, C = npts // M, -(-K // D), N + 1
        sy = t.RealSynthesizer.oversampled(prototype(M, K), M, OS)
        row = {"M": M, "OS": OS, "K": K, "Q": Q, "F": F}
        xo = x[:F * D]
        if quick:
            ur = rows[: C * F].view(C, F)
            sy.step(ur, xo)
            sy.step(ur, xo)
            torch.cuda.synchronize()
            print(json.dumps(row), flush=True)
            sy.close()
            continue
        um = rows.view(M, F)
        um[0].imag.zero_()                         # the extension pass: not timed
        um[N].imag.zero_()
        um[N + 1:] = torch.conj(torch.flip(um[1:N], dims=(0,)))
        ur = um[:C]
        cs, crit = t.Synthesizer(prototype(M, K), M, oversample=OS), t.RealSynthesizer(prototype(M, Q * M), M)     # (A), (B)
        xa = xc[:F * D]
        for _ in range(3):
            sy.step(ur, xo)
            cs.step(um, xa)
            crit.step(ur, x)
        torch.cuda.synchronize()
        tr, ta, tb = [], [], []
        for _ in range(reps):                      # the candidates interleaved
            tr.append(event_ms(lambda: sy.step(ur, xo)))
            ta.append(event_ms(lambda: cs.step(um, xa)))
            tb.append(event_ms(lambda: crit.step(ur, x)))
        mr, ma, mb = float(np.median(tr)), float(np.median(ta)), float(np.median(tb))
        row.update({"real_ms": round(mr, 4), "frac_8TBs": round((8 * C / M + 4 / OS) * npts / (mr * 1e-3) / 8e12, 3),
                    "cplx_ms": round(ma, 4), "real_over_cplx": round(mr / ma, 3), "crit_ms": round(mb, 4),
                    "real_over_crit": round(mr / mb, 3)})
        print(json.dumps(row), flush=True)
        table.append(row)
        for o in (sy, cs, crit):
            o.close()
    if table:
        print("#")
        print("# M     OS  Q   K      real ms  (of 8 TB/s)  x (A) complex  x (B) critical real")
        for r in table:
            print(f"# {r['M']:<5} {r['OS']:<3} {r['Q']:<3} {r['K']:<6} {r['real_ms']:<8.4f} ({r['frac_8TBs']:.3f})      "
                  f"x {r['real_over_cplx']:<12.3f} x {r['real_over_crit']:.3f}")


if __name__ == "__main__":
    main()
