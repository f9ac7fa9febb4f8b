"""The polyphase banks (channelizer.hip, channelizer_os.hip, synthesizer.hip, synthesizer_os.hip) held to float64 per frame / per
output sample at high dynamic range, at every served branch length (the bounds and inputs of tests/poly_f64.py; they are shown to
discriminate, without a GPU, by tests/test_poly_f64_cpu.py).

The parity tests of the four banks measure max |y - ref| against the loudest output of a step, with a smooth prototype whose edge
taps are 1e-8 of its sum: a dropped or misplaced edge tap is invisible there.  Here the taps are standard normal (every tap
counts), the channelizer's input is a burst train (loud 1e4 / 1e6, quiet 1 / 1e-3, exact zeros) with lone samples of 1e6 inside
zero stretches (an impulse reads every tap back), the synthesizer's an (M, F) normal block under a per-frame envelope of the same
kinds with one row 1e4 louder, streamed in ragged steps (odd counts move the phase of an oversampled bank), and every frame /
sample is judged against its own bound; zero-bound ones must be exactly zero.

 1. the sweep: all four kernels, M in {8, 16, 32, 64, 128, 1024} (first radix 0, 16, 2, 4, 8 and two positions per thread), every
    served value of the kernels' template argument -- P = 1 ... 16 taps per position (OS = 1), P = 1 ... 16 / OS (the oversampled
    channelizer), Q = 1 ... 16 taps per hop sample (the oversampled synthesizer) -- each with a tap count inside the last row
    and one that fills it; 300 frames = 19 units.
 2. long steps: one call long enough that every sub-run takes `per` = 3 units of the persistent loop (the window then arrives
    by window_shift from the previous unit, and the LDS image is reused after store_rows); then the same stream in three ragged
    steps on a fresh handle: the same bits."""
import functools

import numpy as np
import pytest

import poly_f64 as PF

pytestmark = pytest.mark.gpu
MS = (8, 16, 32, 64, 128, 1024)
FRAMES = 300


@pytest.fixture(scope="module")
def tg():
    import libtsd_amd as t
    assert t.device_count() >= 1
    return t


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def served(bank, OS):
    """the values of the kernel's template argument, and the row length L its tap count is measured in"""
    if bank == "chan":
        return range(1, 16 // OS + 1), "M"
    return range(1, 17), "M" if OS == 1 else "D"


@functools.lru_cache(maxsize=None)
def chan_data(M, OS, frames=FRAMES):
    x = PF.chan_input(np.random.default_rng([1, M, OS, frames]), frames * (M // OS), M)
    return x, dev(x)


@functools.lru_cache(maxsize=None)
def syn_data(M, OS, frames=FRAMES):
    u = PF.syn_input(np.random.default_rng([2, M, OS, frames]), M, frames)
    return u, dev(u)


def run_and_judge(tg, bank, M, OS, h, data, steps, what):
    """one fresh handle over the stream in `steps`; -> (worst err / bound, the output)"""
    host, on_dev = data
    if bank == "chan":
        y64, bound = PF.chan(host, PF.chan_table(h, M), M, OS)
        y = PF.chan_stream(tg, h, M, OS, on_dev, steps)
        return PF.chan_judge(y, y64, bound, what), y
    x64, bound = PF.syn(host, PF.syn_table(h, M // OS), M, OS)
    x = PF.syn_stream(tg, h, M, OS, on_dev, steps)
    return PF.syn_judge(x, x64, bound, what), x


# ------------------------------------------------------------------------------------------------ 1. branch-length sweep
def _sweep():
    return [(bank, M, OS, P) for bank in ("chan", "syn") for OS in (1, 2, 4) for M in MS for P in served(bank, OS)[0]]


@pytest.mark.parametrize("bank,M,OS,P", _sweep())
def test_branch_length_sweep(tg, bank, M, OS, P):
    """P: the template argument (taps per position; per hop sample for the oversampled synthesizer).  K = (P - 1) L + 1 + a seeded
    offset < L - 1 (inside the last row: zero-padded taps), and K = P L (the row full)."""
    rng = np.random.default_rng([3, bank == "syn", M, OS, P])
    L = M if served(bank, OS)[1] == "M" else M // OS
    data = (chan_data if bank == "chan" else syn_data)(M, OS)
    for K in ((P - 1) * L + 1 + int(rng.integers(0, L - 1)), P * L):
        h = PF.taps(rng, K)
        what = f"{bank} M={M} OS={OS} P={P} K={K}"
        ratio, _ = run_and_judge(tg, bank, M, OS, h, data, PF.ragged(rng, FRAMES), what)
        print(f"{what}: worst err / bound {ratio:.3f}")
        assert ratio <= 1.0, what


# ------------------------------------------------------------------------------------------------ 2. long steps, per >= 2
def _long():
    out = []
    for bank in ("chan", "syn"):
        for M, OS in ((8, 1), (64, 1), (1024, 1), (64, 2)):
            # P in {3, 16}; the oversampled channelizer serves P <= 16 / OS: its largest
            out += [(bank, M, OS, P) for P in (3, 16 // OS if bank == "chan" else 16)]
    return out


@pytest.mark.parametrize("bank,M,OS,P", _long())
def test_long_step_second_iteration(tg, bank, M, OS, P):
    """F = 2 x 16 x R x grid + 17 frames (R = 512 / M sub-runs, grid = 2 CUs; M = 1024: R = 1, grid = CUs): 2 R grid + 2 units, so
    polybank_geometry hands every sub-run per = 3 units.  About 2^23 samples each way."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    F = 2 * 16 * cus + 17 if M == 1024 else 2 * 16 * (512 // M) * (2 * cus) + 17
    units, subruns = -(-F // 16), cus if M == 1024 else (512 // M) * 2 * cus
    assert -(-units // subruns) >= 2
    rng = np.random.default_rng([4, bank == "syn", M, OS, P])
    L = M if served(bank, OS)[1] == "M" else M // OS
    K = (P - 1) * L + 1 + int(rng.integers(0, L - 1))
    h = PF.taps(rng, K)
    data = (chan_data if bank == "chan" else syn_data)(M, OS, F)
    what = f"{bank} M={M} OS={OS} P={P} K={K} F={F}"
    ratio, one = run_and_judge(tg, bank, M, OS, h, data, [F], what)
    print(f"{what}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0, what
    a, b = sorted(int(v) for v in rng.choice(np.arange(1, F, 2), 2, replace=False))       # odd cuts: the phase moves
    stream = PF.chan_stream if bank == "chan" else PF.syn_stream
    three = stream(tg, h, M, OS, data[1], [a, b - a, F - b])
    assert np.array_equal(bits(one), bits(three)), what
    (chan_data if bank == "chan" else syn_data).cache_clear()                          # 64 MB a side: not kept for the session
