#!/usr/bin/env python3
"""Channel banks (tsdgpu_fir_bank / tsdgpu_sos_bank) at C * n = 2^24 samples, n in {512, 4096, 65536}: ms per step by HIP
events, next to the loop of C single-stream steps (timed on min(C, 256) channels and scaled), and the share of 8 TB/s on
the algorithmic bytes 2 C n sizeof(T).  Kernel times: run under `rocprofv3 --kernel-trace --stats` (--quick: one step per
shape, no loops)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import libtsd_amd as t  # noqa: E402
from oracle import pyoracle as orc  # noqa: E402


def ms_per(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    quick = "--quick" in sys.argv
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    total = 1 << 24
    z, p, mn, md = orc.design_butter_lp(12, 0.25)
    co, gain, r1 = orc.SosChain(z, p, mn, md).coefs()
    cases = [("fir", K, cplx) for K in (7, 31, 127) for cplx in (False, True)] + [("sos6", 12, False), ("sos6", 12, True)]
    for n in (512, 4096, 65536):
        C = total // n
        for kind, K, cplx in cases:
            dt = t.C64 if cplx else t.F32
            x = torch.randn(C, n, device=dev, generator=g, dtype=torch.complex64 if cplx else torch.float32)
            y = torch.empty_like(x)
            if kind == "fir":
                h = orc.design_rif_fen(K, "lp", 0.25)
                bank = t.FirBank(h, dt, C)
                single = lambda: t.Fir(h, dt, t.FIR_DIRECT)  # noqa: E731
            else:
                bank = t.SosBank(co, gain, dt, C, r1)
                single = lambda: t.Sos(co, gain, dt, r1)  # noqa: E731
            row = {"op": kind if kind != "fir" else f"fir{K}", "data": "c64" if cplx else "f32", "C": C, "n": n}
            if quick:
                bank.step(x, y)
                torch.cuda.synchronize()
                print(json.dumps(row), flush=True)
                continue
            ms = ms_per(lambda: bank.step(x, y), 30)
            bytes_alg = 2.0 * C * n * (8 if cplx else 4)
            row.update({"bank_ms": round(ms, 4), "frac_8TBs": round(bytes_alg / (ms * 1e-3) / 8e12, 3)})
            Cl = min(C, 256)
            hs = [single() for _ in range(Cl)]

            def loop():
                for c in range(Cl):
                    hs[c].step(x[c], y[c])
            lm = ms_per(loop, 3, 1) * C / Cl
            row.update({"loop_ms": round(lm, 3), "speedup": round(lm / ms, 1)})
            print(json.dumps(row), flush=True)
            del x, y, bank, hs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
