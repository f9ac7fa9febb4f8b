#!/usr/bin/env python3
"""One sha256 per branch of the single-stream rate changers (csrc/resample.hip, the tsdgpu_polyfir half of csrc/polyphase.hip): the
resampler's three kernels with the static and the dynamic tile hand-out, table-driven and analytic interpolators, seek / reset, input
from the host and the chunked host pipeline; the integer-rate stages' direct, rows, oldest-first and composed paths.  Each case at the
smallest shape that reaches the branch, on seeded randn input, float and complex, fed as one call and again in pieces; the outputs
are copied to the host and hashed.  Two builds of the library compute the same bits exactly when their lists are equal (TSDGPU_LIB
selects the build, see scripts/build_variant.sh).  The cases under a developer switch run in child processes of their own, one per
switch, each under a time limit; the first child that fails ends the run.
usage (GPU box, repo root): python3 scripts/digest_rate.py"""
import hashlib
import os
import subprocess
import sys

N = 20000
CUTS = [0, 311, 4412, N]
R160 = 160.0 / 147.0
# resampler, table-driven: (K, phases, ratio).  K = 15 with up to 511 phases at a ratio <= 2: resample15s_kernel; 24 taps and more at
# a ratio <= 2: resample_long_kernel (one and several tap phases); the rest resample_kernel (table in LDS with 8 or fewer waves, or
# read in place)
K15 = [(15, 256, R160), (15, 256, 0.5), (15, 256, 1.999)]
TABLES = {
    "": K15 + [(4, 256, R160), (15, 512, R160), (31, 256, R160), (127, 256, R160), (256, 128, R160), (63, 8191, R160), (31, 256, 3.1)],
    "TSDGPU_RS_DYN_MIN=0": K15,
    "TSDGPU_RS_DYN=0": K15,
    "TSDGPU_RS15=0": K15,
    "TSDGPU_RS_LONG=0": [(127, 256, R160)],
}
ANALYTIC = [("lin", 0), ("lagrange", 3)]
# integer-rate stages: (kind, R, K).  DECIM 2 / 4 / 8 up to 64 taps: decim_direct_kernel; small rates from 32 taps: decim_rows_kernel;
# the others polyfir_fused_kernel or, beyond its LDS, the composition; UPS 2 / 4 with branches up to 32 taps: ups_direct_kernel
DECIM, HALFBAND, UPS, PICK = 0, 1, 2, 3
STAGES = [(DECIM, R, K) for R, K in [(2, 15), (4, 15), (8, 15), (2, 64), (2, 65), (3, 33), (5, 15), (16, 63), (60, 15), (7, 200), (100, 31)]] + \
         [(HALFBAND, 2, 15), (HALFBAND, 2, 31)] + [(UPS, R, K) for R, K in [(2, 31), (4, 127), (4, 129), (3, 15), (2, 4100)]] + [(PICK, 3, 0)]
SWITCHED = [(DECIM, 2, 15), (DECIM, 3, 33), (UPS, 2, 31)]
POLY = {"": STAGES, "TSDGPU_POLY_COMPOSED=1": SWITCHED, "TSDGPU_POLY_NO_DIRECT=1": SWITCHED, "TSDGPU_POLY_NO_ROWS=1": SWITCHED}
GROUPS = ["", "TSDGPU_RS_DYN_MIN=0", "TSDGPU_RS_DYN=0", "TSDGPU_RS15=0", "TSDGPU_RS_LONG=0", "TSDGPU_POLY_COMPOSED=1",
          "TSDGPU_POLY_NO_DIRECT=1", "TSDGPU_POLY_NO_ROWS=1"]
CHILD_SECONDS = 240


def child(group):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    import libtsd_amd as t

    def randn(seed, n, cplx):
        g = torch.Generator().manual_seed(seed)
        return torch.view_as_complex(torch.randn(n, 2, generator=g)) if cplx else torch.randn(n, generator=g)

    def host(y):
        return y.cpu().numpy() if torch.is_tensor(y) else np.asarray(y)

    def show(name, *ys):
        d = hashlib.sha256()
        for y in ys:
            d.update(host(y).tobytes())
        print("%-72s %s" % ((group + " " if group else "") + name, d.hexdigest()), flush=True)

    def pieces(op, x, cuts):
        return [op.step(x[a:b]) for a, b in zip(cuts, cuts[1:])]

    def table(K, nph):
        return (randn(7 * K + nph, (nph + 1) * K, False) / K).numpy().reshape(nph + 1, K)

    types = [(False, t.F32, "f32"), (True, t.C64, "c64")]
    for K, nph, ratio in TABLES.get(group, []):
        lut = table(K, nph)
        for cplx, dt, tn in types:
            x = randn(K + nph, N, cplx).cuda()
            name = "resampler K=%d nph=%d ratio=%.6g %s" % (K, nph, ratio, tn)
            r = t.Resampler(ratio, dt, K, nph, lut=lut)
            show(name + " whole", r.step(x))
            r.close()
            r = t.Resampler(ratio, dt, K, nph, lut=lut)
            show(name + " cut", *pieces(r, x, CUTS))
            r.close()
            if group == "TSDGPU_RS_DYN_MIN=0":       # the counters' base is not 0 at the second step; a second handle starts its own
                r, r2 = t.Resampler(ratio, dt, K, nph, lut=lut), t.Resampler(ratio, dt, K, nph, lut=lut)
                show(name + " two steps, a third on a second handle", r.step(x[:N // 2]), r.step(x[N // 2:]), r2.step(x))
                r.close()
                r2.close()
    if group == "":
        lut = table(15, 256)
        for cplx, dt, tn in types:
            x = randn(99, N, cplx).cuda()
            for kind, d in ANALYTIC:
                for ratio in (1.5, 3.1):
                    name = "resampler %s %d ratio=%.6g %s" % (kind, d, ratio, tn)
                    r = t.Resampler(ratio, dt, analytic=(kind, d))
                    show(name + " whole", r.step(x))
                    r.close()
                    r = t.Resampler(ratio, dt, analytic=(kind, d))
                    show(name + " cut", *pieces(r, x, CUTS))
                    r.close()
            w = randn(5, 14, cplx)
            for how, hist in [("device", w.cuda()), ("host", w.numpy()), ("none", None)]:
                r = t.Resampler(R160, dt, 15, 256, lut=lut)
                r.seek(12345, hist)
                show("resampler seek 12345 window %s %s" % (how, tn), r.step(x), np.int64(r.out_offset))
                r.close()
            for ratio in (1.0, 2.5):
                r = t.Resampler(ratio, dt, 15, 256, lut=lut)
                r.seek(10 ** 9)
                off = r.out_offset
                show("resampler seek 1e9 ratio=%.6g %s" % (ratio, tn), np.int64(off), r.step(x), np.int64(r.out_offset))
                r.close()
            r = t.Resampler(R160, dt, 15, 256, lut=lut)
            a = r.step(x[:5000])
            r.reset()
            show("resampler reset, then step %s" % tn, a, r.step(x))
            r.close()
            r = t.Resampler(R160, dt, 15, 256, lut=lut)
            show("resampler from the host %s" % tn, *pieces(r, x.cpu().numpy(), CUTS))
            r.close()
        r = t.Resampler(R160, t.C64, 15, 256, lut=lut)
        show("resampler host vector of 2^20 c64 (chunked)", r.step(randn(3, 1 << 20, True).numpy()))
        r.close()

    for kind, R, K in POLY.get(group, []):
        taps = None if kind == PICK else (randn(11 * R + K, K, False) / 4).numpy()
        for cplx, dt, tn in types:
            x = randn(R + K, N, cplx).cuda()
            name = "polyfir kind=%d R=%d K=%d %s" % (kind, R, K, tn)
            p = t.PolyFir(kind, dt, taps, R)
            show(name + " whole", p.step(x))
            p = t.PolyFir(kind, dt, taps, R)
            show(name + " cut", *pieces(p, x, CUTS))
            p = t.PolyFir(kind, dt, taps, R)
            show(name + " blocks of 37", *pieces(p, x, list(range(0, N, 37)) + [N]))
            p = t.PolyFir(kind, dt, taps, R)
            show(name + " blocks of 1", *pieces(p, x, list(range(0, 401))))
            if group == "" and (kind, R, K) == (DECIM, 3, 33):
                p = t.PolyFir(kind, dt, taps, R)
                a = p.step(x[:5000])
                p.reset()
                show(name + " reset, then step", a, p.step(x))
                p = t.PolyFir(kind, dt, taps, R)
                show(name + " from the host", *pieces(p, x.cpu().numpy(), CUTS))
    if group == "":
        taps = (randn(1, 33, False) / 4).numpy()
        p = t.PolyFir(DECIM, t.C64, taps, 3)
        show("polyfir kind=0 R=3 K=33 host vector of 2^20 c64 (chunked)", p.step(randn(4, 1 << 20, True).numpy()))
        p = t.PolyFir(UPS, t.C64, taps, 2)
        show("polyfir kind=2 R=2 K=33 host vector of 2^20 c64 (chunked)", p.step(randn(4, 1 << 20, True).numpy()))


if __name__ == "__main__":
    if len(sys.argv) > 1:
        child(sys.argv[1] if sys.argv[1] != "-" else "")
    else:
        for group in GROUPS:
            env = dict(os.environ)
            if group:
                env.update([group.split("=")])
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), group or "-"], env=env, timeout=CHILD_SECONDS).returncode
            if rc:
                sys.exit(rc)
