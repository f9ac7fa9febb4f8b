"""The per-frame float64 bounds of tests/poly_f64.py checked without a GPU: they discriminate.  On the inputs the GPU tests use
(random taps, burst trains with lone impulses / burst envelopes), for every shape below and both banks: a float32 emulation (a
float32 chain, oldest tap first, plus a scipy.fft complex64 transform) stays inside the bound, and three wrong banks -- h[0]
dropped, h[K-1] dropped, one branch's taps one frame late -- exceed it at least 100 times over.  Also: poly_f64's float64
statements are those of chan_os_ref / syn_os_ref, and exact zeros come out as exact zeros."""
import functools

import numpy as np
import pytest

import chan_os_ref
import poly_f64 as PF
import syn_os_ref

SHAPES = [(8, 4, 32), (16, 2, 45), (64, 1, 453), (64, 2, 353), (256, 4, 1024), (1024, 2, 1025), (1024, 1, 16384)]
FRAMES = 300
OVER = 100.0


@functools.lru_cache(maxsize=None)
def case(bank, M, OS, K):
    """the reference, the bound, and the float32 runs of the right table and of the three wrong ones, once per shape"""
    rng = np.random.default_rng([M, OS, K, bank == "syn"])
    D = M // OS
    h = PF.taps(rng, K)
    if bank == "chan":
        data, L, table, run = PF.chan_input(rng, FRAMES * D, M), M, PF.chan_table, PF.chan
    else:
        data, L, table, run = PF.syn_input(rng, M, FRAMES), D, PF.syn_table, PF.syn
    good = table(h, L)
    ref, bound, y = run(data, good, M, OS, emulate=good)
    wrong = {name: run(data, good, M, OS, emulate=tab)[2] for name, tab in PF.mutants(h, table, L, int(rng.integers(L))).items()}
    return h, data, ref, bound, y, wrong


def judge(bank):
    return PF.chan_judge if bank == "chan" else PF.syn_judge


@pytest.mark.parametrize("M,OS,K", SHAPES)
@pytest.mark.parametrize("bank", ["chan", "syn"])
def test_float32_emulation_is_inside_the_bound(bank, M, OS, K):
    h, data, ref, bound, y, _ = case(bank, M, OS, K)
    ratio = judge(bank)(y, ref, bound)
    print(f"{bank} M={M} OS={OS} K={K}: float32 emulation, worst err / bound {ratio:.3f}; zero-bound entries {int((bound == 0).sum())}")
    assert ratio <= 1.0


@pytest.mark.parametrize("M,OS,K", SHAPES)
@pytest.mark.parametrize("bank", ["chan", "syn"])
def test_wrong_banks_are_far_outside_the_bound(bank, M, OS, K):
    h, data, ref, bound, _, wrong = case(bank, M, OS, K)
    assert len(wrong) == 3
    for name, y in wrong.items():
        live = bound > 0
        err = np.abs(y.astype(np.complex128) - ref)
        err = err.max(axis=0) if bank == "chan" else err
        ratio = float((err[live] / bound[live]).max())
        print(f"{bank} M={M} OS={OS} K={K}: {name}, worst err / bound {ratio:.3g}")
        assert ratio >= OVER, (name, ratio)


@pytest.mark.parametrize("M,OS,K", SHAPES[:5])
def test_float64_statements_are_the_references(M, OS, K):
    h, x, ref, _, _, _ = case("chan", M, OS, K)
    want = chan_os_ref.polyphase64(x, h, M, OS)
    assert np.abs(ref - want).max() <= 1e-12 * np.abs(want).max()
    f, u, ref, _, _, _ = case("syn", M, OS, K)
    want = syn_os_ref.synth64(u, f, M, OS)
    assert np.abs(ref - want).max() <= 1e-12 * np.abs(want).max()


def test_bound_by_hand():
    """M = 8, OS = 2, K = 3, one impulse: frame m reads x[4 m - 4 .. 4 m + 3] against g_0[s] = h[7 - s]"""
    M, OS = 8, 2
    h = np.array([0.5, -2.0, 4.0], np.float32)
    x = np.zeros(16, np.complex64)
    x[5] = 3.0
    y64, bound = PF.chan(x, PF.chan_table(h, M), M, OS)
    # x[5] is position 5 of frame 1 (tap h[2]), position 1 of frame 2 (past the taps): one live frame
    A = 4.0 * 3.0
    assert np.allclose(bound, [0, PF.R.gamma(3) * A + 8 * PF.R.U * 3 * A, 0, 0], rtol=1e-12)
    assert np.allclose(np.abs(y64[:, 1]), A) and not y64[:, [0, 2, 3]].any()
    # the dual: D = 4, Q = 1, a lone channel-0 frame of 2.0 -> w = 2 at every r, x[4 q + s'] = f[s'] w
    f = np.array([1.0, -3.0, 0.25], np.float32)
    u = np.zeros((M, 3), np.complex64)
    u[0, 1] = 2.0
    x64, b = PF.syn(u, PF.syn_table(f, 4), M, OS)
    assert np.allclose(x64, [0, 0, 0, 0, 2.0, -6.0, 0.5, 0, 0, 0, 0, 0])
    assert np.allclose(b[4:8], np.abs([1.0, -3.0, 0.25, 0]) * (8 * PF.R.U * 3 * 2.0 + PF.R.gamma(3) * 2.0), rtol=1e-12)
    assert not b[:4].any() and not b[8:].any()


def test_inputs():
    rng = np.random.default_rng(3)
    for M, n in ((8, 600), (64, 19200), (1024, 76800)):
        x = PF.chan_input(rng, n, M)
        mag = np.abs(x)
        assert x.dtype == np.complex64 and len(x) == n
        lone = np.nonzero((mag == 1e6) & (np.roll(mag, 1) + np.roll(mag, -1) < 1e6))[0]
        assert len(lone) >= 2 and (mag == 0).sum() > n // 50
    u = PF.syn_input(rng, 16, 500)
    mag = np.abs(u)
    assert u.shape == (16, 500) and (mag.max(axis=0) == 0).any() and mag.max() > 1e9 and mag[mag > 0].min() < 1e-2
    for F in (1, 16, 300):
        steps = PF.ragged(rng, F)
        assert sum(steps) == F and min(steps) >= 1
