#!/usr/bin/env python3
"""The FIR bank's two schemes at C * n = 2^24 samples: ms per step by HIP events (median, the two methods interleaved
round by round in one process) over n in {64 .. 65536} x K in {57 .. 961}, float and complex data with real taps, and the
share of 8 TB/s on the algorithmic bytes 2 C n sizeof(T).  The AUTO rule of ols_bank.hip (ols_bank_preferred) is read off
this table.  --shapes: only the three shapes of DESIGN 3.9 at K = 127; --quick: one step per case (for rocprofv3);
--K=a,b,.. / --n=a,b,..: other tap counts / channel lengths (the refinement around the crossovers)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import libtsd_amd as t  # noqa: E402
from oracle import pyoracle as orc  # noqa: E402


def interleaved_ms(fns, rounds, per=5):
    for f in fns:
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            for _ in range(per):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                ts[i].append(a.elapsed_time(b))
    return [float(np.median(v)) for v in ts]


def main():
    quick, shapes = "--quick" in sys.argv, "--shapes" in sys.argv
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    total = 1 << 24
    ns = (512, 4096, 65536) if shapes or quick else (64, 128, 256, 512, 1024, 4096, 65536)
    Ks = (127,) if shapes or quick else (57, 127, 255, 513, 769, 961)
    for a in sys.argv[1:]:
        if a.startswith("--K="):
            Ks = tuple(int(v) for v in a[4:].split(","))
        if a.startswith("--n="):
            ns = tuple(int(v) for v in a[4:].split(","))
    for cplx in (False, True):
        dt = t.C64 if cplx else t.F32
        for n in ns:
            C = total // n
            x = torch.randn(C, n, device=dev, generator=g, dtype=torch.complex64 if cplx else torch.float32)
            y = torch.empty_like(x)
            for K in Ks:
                h = orc.design_rif_fen(K, "lp", 0.1)
                d, o = t.FirBank(h, dt, C, method=t.FIR_DIRECT), t.FirBank(h, dt, C, method=t.FIR_OVERLAP_SAVE)
                row = {"data": "c64" if cplx else "f32", "K": K, "C": C, "n": n}
                if quick:
                    o.step(x, y)
                    torch.cuda.synchronize()
                    print(json.dumps(row), flush=True)
                    continue
                md, mo = interleaved_ms([lambda: d.step(x, y), lambda: o.step(x, y)], 6)
                by = 2 * C * n * (8 if cplx else 4)
                row.update(direct_ms=round(md, 4), ols_ms=round(mo, 4), direct_over_ols=round(md / mo, 2),
                           ols_frac_8TBs=round(by / (mo * 1e-3) / 8e12, 3), direct_frac_8TBs=round(by / (md * 1e-3) / 8e12, 3))
                print(json.dumps(row), flush=True)
                d.close()
                o.close()
            del x, y


if __name__ == "__main__":
    main()
