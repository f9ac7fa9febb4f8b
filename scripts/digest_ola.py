#!/usr/bin/env python3
"""One sha256 per branch of csrc/ola.hip: the OLA engine (every fused kernel geometry, whole and ragged calls, in place, from the
host), psd_welch and rt_spectrum, each at the smallest shape that reaches the branch, on seeded randn complex64 input; the output is
copied to the host and hashed.  Two builds of the library compute the same bits exactly when their lists are equal (TSDGPU_LIB
selects the build, see scripts/build_variant.sh).  The cases under a developer switch run in child processes of their own, one per
switch.
usage (GPU box, repo root): python3 scripts/digest_ola.py"""
import hashlib
import os
import subprocess
import sys

BLOCKS = 8
# (Ne, min_zeros) without window: in-wave + ola_run on the ragged calls; 256 threads smallest N / half / not half; N = 4096 half / not;
# 512 threads half / not; 1024 threads half; no fused kernel (analyse / synthese)
OLA = {
    "": [(512, 127), (16, 15), (64, 64), (900, 100), (2048, 2048), (3000, 500), (4096, 4096), (6000, 2000), (8192, 8192), (12000, 100)],
    "TSDGPU_OLA_UNFUSED=1": [(512, 127)],
    "TSDGPU_OLAW512=0": [],
}
# Hann-windowed: olaw512; windowed run kernel x 3; no fused kernel
OLAW = {
    "": [(512, 0), (64, 64), (100, 20), (1000, 24), (4096, 0)],
    "TSDGPU_OLA_UNFUSED=1": [(512, 0)],
    "TSDGPU_OLAW512=0": [(512, 0)],
}
INPLACE = {"": [(512, 127, False), (2048, 127, False), (512, 0, True)]}
HOST = {"": [(512, 127)]}
# (N, samples): in-wave; run kernel at 256 and 1024 threads; framed Bluestein x 3; N < 16 (plan path); no segment; the framed-FFT
# path with 65 groups, the fewest that take its two-stage sum (1025 segments of 8 every 4 samples)
WELCH = {
    "": [(1024, 1024 * 5), (64, 64 * 9), (16384, 16384 * 3), (255, 4096), (1000, 8000), (2000, 16000), (1, 8), (1024, 1000), (8, 4105)],
    "TSDGPU_OLA_UNFUSED=1": [(1024, 1024 * 5)],
}
# (BS, nsubs, nmeans, sweep step or None): run kernel; sub-blocks; plan path; sweep; BS no multiple of nsubs
SPECTRUM = {"": [(1024, 1, 2, None), (4096, 4, 3, None), (1000, 1, 4, None), (4096, 4, 2, 700), (4099, 4, 2, None)]}
GROUPS = ["", "TSDGPU_OLA_UNFUSED=1", "TSDGPU_OLAW512=0"]


def child(group):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    import libtsd_amd as t

    def randc(seed, n):
        return torch.view_as_complex(torch.randn(n, 2, generator=torch.Generator().manual_seed(seed)))

    def host(y):
        return y if isinstance(y, np.ndarray) else y.cpu().numpy()

    def show(name, *ys):
        d = hashlib.sha256()
        for y in ys:
            d.update(host(y).tobytes())
        print("%-52s %s" % ((group + " " if group else "") + name, d.hexdigest()), flush=True)

    def hann(n):
        return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)).astype(np.float32)

    def ola(Ne, nz, windowed):
        g = t.Ola(Ne, nz, hann(Ne) if windowed else None)
        g.set_response(randc(1000 + g.N, g.N).numpy())
        return g

    def both_feeds(Ne, nz, windowed):
        tag = "olaw" if windowed else "ola"
        x = randc(Ne + nz, BLOCKS * Ne).cuda()
        g = ola(Ne, nz, windowed)
        show("%s Ne=%d nz=%d whole" % (tag, Ne, nz), g.step(x))
        g.close()
        g = ola(Ne, nz, windowed)
        cuts = [0, Ne // 2 + 3, Ne // 2 + 3 + 3 * Ne + 5, BLOCKS * Ne]
        show("%s Ne=%d nz=%d ragged" % (tag, Ne, nz), *[g.step(x[a:b]) for a, b in zip(cuts, cuts[1:])])
        g.close()

    for Ne, nz in OLA.get(group, []):
        both_feeds(Ne, nz, False)
    for Ne, nz in OLAW.get(group, []):
        both_feeds(Ne, nz, True)
    for Ne, nz, windowed in INPLACE.get(group, []):
        x = randc(Ne + nz, BLOCKS * Ne).cuda()
        g = ola(Ne, nz, windowed)
        show("%s Ne=%d nz=%d in place" % ("olaw" if windowed else "ola", Ne, nz), g.step(x, y=x))
        g.close()
    for Ne, nz in HOST.get(group, []):
        g = ola(Ne, nz, False)
        show("ola Ne=%d nz=%d from the host" % (Ne, nz), g.step(randc(Ne + nz, BLOCKS * Ne).numpy()))
        g.close()
    for N, samples in WELCH.get(group, []):
        S, nseg = t.welch(randc(N, samples).cuda(), N, hann(N))
        show("welch N=%d of %d (%d segments)" % (N, samples, nseg), S)
    for BS, nsubs, nmeans, step in SPECTRUM.get(group, []):
        Nf = BS // nsubs
        w = hann(Nf)
        w *= np.float32(np.sqrt(Nf / np.sum(w.astype(np.float64) ** 2)))
        s = t.Spectrum(BS, nsubs, nmeans, w, None if step is None else (step, None))
        x = randc(BS + nsubs, 5 * BS).cuda()
        show("spectrum BS=%d nsubs=%d nmeans=%d%s" % (BS, nsubs, nmeans, "" if step is None else " sweep %d" % step),
             s.step(x[:2 * BS]), s.step(x[2 * BS:]))
        s.close()


if __name__ == "__main__":
    if len(sys.argv) > 1:
        child(sys.argv[1] if sys.argv[1] != "-" else "")
    else:
        for group in GROUPS:
            env = dict(os.environ)
            if group:
                env.update([group.split("=")])
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), group or "-"], env=env).returncode
            if rc:
                sys.exit(rc)
