#!/usr/bin/env python3
"""One sha256 per FFT plan branch: the smallest shape that reaches each branch of csrc/fft.hip, forward and inverse, on seeded
randn complex64 input; the output is copied to the host and hashed.  Two builds of the library compute the same bits exactly when
their lists are equal (TSDGPU_LIB selects the build, see scripts/build_variant.sh).  The cases under a developer switch run in
child processes of their own, one per switch.
usage (GPU box, repo root): python3 scripts/digest_fft_plans.py"""
import hashlib
import os
import subprocess
import sys

GROUPS = {
    "": [  # (n, batch) complex cases
        (1, 3), (2, 3), (8, 3), (16, 3), (32, 3), (64, 3), (128, 3), (16384, 1025), (1 << 15, 3), (1 << 15, 64), (1 << 18, 2),
        (1 << 20, 1), (1 << 20, 16), (1 << 21, 1), (1 << 21, 20), (1 << 22, 2), (1 << 23, 1), (1 << 24, 1), (1 << 25, 1),
        (48, 3), (96, 3), (160, 3), (896, 3), (2304, 3), (34, 3), (68, 3), (136, 3), (272, 3), (74, 3), (37 * 32, 3),
        (17, 3), (511, 3), (513, 3), (4097, 3), (8193, 2), (2 * 8193, 2)],
    "TSDGPU_FFT_DYN=0": [(1 << 20, 16)],
    "TSDGPU_FFT_3PASS_23=1": [(1 << 23, 1)],
    "TSDGPU_FFT_GENERIC=1": [(1024, 3), (1 << 16, 2)],
    "TSDGPU_RFFT_TWO_PASS=1": [],
}
RFFT = {"": [(32, 3), (4096, 3), (1 << 16, 2), (17, 3)], "TSDGPU_RFFT_TWO_PASS=1": [(64, 3)]}
WELCH = {"": [(255, 4096)]}   # (segment length, samples): the framed wave-level Bluestein


def child(group):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    import libtsd_amd as t

    def randn(seed, *shape):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))

    def show(name, y):
        y = y if isinstance(y, np.ndarray) else y.cpu().numpy()
        print("%-34s %s" % ((group + " " if group else "") + name, hashlib.sha256(y.tobytes()).hexdigest()), flush=True)

    for n, batch in GROUPS[group]:
        x = torch.view_as_complex(randn(n, batch, n, 2)).cuda()
        p = t.Fft(n)
        for forward in (True, False):
            show("fft n=%d x %d %s" % (n, batch, "fwd" if forward else "inv"), p.step(x, forward))
        p.close()
    for n, batch in RFFT.get(group, []):
        p = t.Rfft(n)
        show("rfft n=%d x %d" % (n, batch), p.step(randn(n, batch, n).cuda()))
        p.close()
    for N, samples in WELCH.get(group, []):
        S, nseg = t.welch(torch.view_as_complex(randn(N, samples, 2)).cuda(), N, np.hanning(N).astype(np.float32))
        show("welch N=%d of %d (%d segments)" % (N, samples, nseg), S)


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
