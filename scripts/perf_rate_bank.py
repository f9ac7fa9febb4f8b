#!/usr/bin/env python3
"""Rate-changing channel bank (tsdgpu_polyfir_bank) at C * n = 2^24 input samples, n in {512, 4096, 65536}: ms per step by HIP
events (median, warm), the share of 8 TB/s on the algorithmic bytes C n sizeof(T) (1 + 1/R) (decimators) or (1 + R)
(upsamplers), next to the loop of C single-stream steps (timed on min(C, 256) channels and scaled).  Kernel times: run under
`rocprofv3 --kernel-trace --stats` with --quick (two steps per shape, no loops).  --no-loop: the bank alone; --n 64,512: other
block lengths."""
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


CASES = ([("decim", R, K) for R in (2, 4, 8) for K in (15, 31)] + [("halfband", 2, 15)] + [("ups", R, 31) for R in (2, 4)])
KINDS = {"decim": t.POLY_DECIM, "halfband": t.POLY_HALFBAND, "ups": t.POLY_UPS}


def main():
    quick = "--quick" in sys.argv
    no_loop = "--no-loop" in sys.argv
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    total = 1 << 24
    lengths = (512, 4096, 65536)
    if "--n" in sys.argv:
        lengths = tuple(int(v) for v in sys.argv[sys.argv.index("--n") + 1].split(","))
    for n in lengths:
        C = total // n
        for cplx in (False, True):
            dt = t.C64 if cplx else t.F32
            x = torch.randn(C, n, device=dev, generator=g, dtype=torch.complex64 if cplx else torch.float32)
            for op, R, K in CASES:
                h = orc.design_rif_fen(K, "lp", 0.4 / R)
                bank = t.PolyFirBank(KINDS[op], dt, C, h, R)
                y = torch.empty(C, bank.out_count(n), device=dev, dtype=x.dtype)
                row = {"op": f"{op}{K}", "R": R, "data": "c64" if cplx else "f32", "C": C, "n": n}
                if quick:
                    bank.step(x, y)
                    bank.step(x, y)
                    torch.cuda.synchronize()
                    print(json.dumps(row), flush=True)
                    continue
                ms = ms_per(lambda: bank.step(x, y), 30)
                bytes_alg = C * n * (8 if cplx else 4) * ((1 + R) if op == "ups" else (1 + 1 / R))
                row.update({"bank_ms": round(ms, 4), "frac_8TBs": round(bytes_alg / (ms * 1e-3) / 8e12, 3)})
                if not no_loop:
                    Cl = min(C, 256)
                    hs = [t.PolyFir(KINDS[op], dt, h, R) for _ in range(Cl)]

                    def loop():
                        for c in range(Cl):
                            hs[c].step(x[c])
                    lm = ms_per(loop, 3, 1) * C / Cl
                    row.update({"loop_ms": round(lm, 3), "speedup": round(lm / ms, 1)})
                    del hs
                print(json.dumps(row), flush=True)
                del y, bank
            del x
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
