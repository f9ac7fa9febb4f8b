"""The float64 references of tests/f64ref.py checked without a GPU: against the CPU oracle on white noise (1e-5 of
the peak: the oracle's float32 rounding), and against the known answers of libtsd's own tests restated in
tests/test_oracle_pins.py.  What the dynamic-range tests compare the kernels with is only as good as this."""
import numpy as np
import pytest

import f64ref as R

TOL = 1e-5


def rand(n, cplx, seed):
    rng = np.random.default_rng(seed)
    if cplx:
        return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    return rng.standard_normal(n).astype(np.float32)


def relerr(y, ref):
    return float(np.abs(np.asarray(y) - ref).max() / max(np.abs(ref).max(), 1e-300))


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("K", [1, 15, 127, 300])
def test_fir(orc, K, cplx):
    h = orc.design_rif_fen(K, "lp", 0.1) if K > 1 else np.array([0.7], np.float32)
    x = rand(5000, cplx, K)
    assert relerr(orc.fir(h, x), R.fir(h, x)) <= TOL


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("Rr,K,kind", [(2, 15, 0), (3, 31, 0), (4, 64, 0), (8, 33, 0), (2, 15, 1), (2, 31, 1)])
def test_decim(orc, Rr, K, kind, cplx):
    rng = np.random.default_rng(K * Rr)
    c = rng.standard_normal(K).astype(np.float32)            # asymmetric: the un-reversed taps show
    x = rand(4001, cplx, Rr)
    y = orc.PolyDecim(c, Rr, kind).step(x)
    ref = R.decim(c, x, Rr, halfband=kind == 1)
    assert len(y) == len(ref) and relerr(y, ref) <= TOL


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("Rr,K", [(2, 15), (3, 31), (4, 17), (5, 64)])
def test_ups(orc, Rr, K, cplx):
    c = np.random.default_rng(K).standard_normal(K).astype(np.float32)
    x = rand(3001, cplx, Rr)
    y = orc.PolyUps(c, Rr).step(x)
    ref = R.ups(c, x, Rr)
    assert len(y) == len(ref) and relerr(y, ref) <= TOL


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("order,fc,forme", [(12, 0.25, 2), (5, 0.1, 2), (6, 0.05, 1), (3, 0.2, 1)])
def test_sos(orc, order, fc, forme, cplx):
    z, p, mn, md = orc.design_butter_lp(order, fc)
    ch = orc.SosChain(z, p, mn, md, forme=forme)
    co, gain, r1 = ch.coefs()
    x = rand(20000, cplx, order) + np.float32(0.5)           # offset: the first-sample seeds matter
    y = np.concatenate([ch.step(x[a:b]) for a, b in ((0, 777), (777, 5000), (5000, 20000))])
    assert relerr(y, R.sos(co, gain, r1, x, forme)) <= TOL


def test_sos_matches_oracle_double_run(orc):
    z, p, mn, md = orc.design_butter_lp(12, 0.25)
    ch = orc.SosChain(z, p, mn, md)
    co, gain, r1 = ch.coefs()
    x = rand(30000, False, 3)
    assert relerr(R.sos(co, gain, r1, x), ch.run_f64(x)) <= 1e-9


@pytest.mark.parametrize("numer,denom", [([0.1], [1.0, -0.9]), ([0.2, 0.3, -0.1], [1.0, -1.2, 0.5, -0.1]),
                                         ([1e-5, 0.0], [1.0, -(1.0 - 1e-5)])])
def test_rii(orc, numer, denom):
    x = rand(20000, False, len(denom))
    f = orc.Rii(np.array(numer, np.float32), np.array(denom, np.float32))
    y = np.concatenate([f.step(x[:5000]), f.step(x[5000:])])
    ref = R.rii(np.array(numer, np.float32), np.array(denom, np.float32), x)
    assert relerr(y, ref) <= TOL


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("which", ["butter4", "cheby"])
def test_rii_bound_holds_for_the_oracle(orc, which, cplx):
    """libtsd's float32 recursion (the oracle) on a burst train stays inside the first-order componentwise bound."""
    from scipy.signal import butter, cheby1
    b, a = butter(4, 0.1) if which == "butter4" else cheby1(5, 0.5, 0.3)
    nu, de = b.astype(np.float32), a.astype(np.float32)
    x, _, _ = R.burst_train(np.random.default_rng(5), 1 << 18, 2048, cplx)
    yo = (orc.RiiC(nu.astype(np.complex64), de.astype(np.complex64)) if cplx else orc.Rii(nu, de)).step(x)
    y64 = R.rii(nu, de, x)
    assert (np.abs(yo - y64) <= R.rii_bound(nu, de, x, y64)).all()


def test_rii_complex(orc):
    nu = np.array([0.3 + 0.1j, 0.2 - 0.05j], np.complex64)
    de = np.array([1.0, -0.6 + 0.3j], np.complex64)
    x = rand(10000, True, 4)
    assert relerr(orc.RiiC(nu, de).step(x), R.rii(nu, de, x)) <= TOL


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("ratio,K", [(160 / 147, 15), (0.7, 15), (1.9, 31), (0.55, 63)])
def test_resample(orc, ratio, K, cplx):
    r = orc.Resampler(ratio, K)
    x = rand(6000, cplx, K)
    s = orc.Resampler(ratio, K)
    n, idx, col = s.schedule(len(x))
    y = r.step(x)
    ref = R.resample(r.lut, idx, col, x)
    assert len(y) == n and relerr(y, ref) <= TOL
    assert np.all(np.abs(y - ref) <= R.gamma(K + 2) * R.resample_bound(r.lut, idx, col, x))


@pytest.mark.parametrize("n", [16, 1024, 1000, 17, 4096 * 3])
@pytest.mark.parametrize("fwd", [True, False])
def test_fft(orc, n, fwd):
    x = rand(n, True, n)
    # sizes whose odd part goes through the reference's float32-chirp Bluestein sit 2e-5 ... 1.5e-3 from float64
    # (INTEGRATION.md "Deliberate differences"); the power-of-two plans are float32 rounding away
    tol = TOL if n & (n - 1) == 0 else 1.5e-3
    assert relerr(orc.fft(x, fwd), R.fft(x, fwd)) <= tol


@pytest.mark.parametrize("Ne,M", [(512, 127), (1024, 300)])
def test_ola(orc, Ne, M):
    from oracle import ola_oracle
    h = orc.design_rif_fen(M, "lp", 0.05)
    o = ola_oracle.Ola(Ne, M, None, None)
    h2 = np.zeros(o.N, np.complex64)
    h2[o.N - M:] = h
    H = (orc.fft(h2, True) * np.float32(np.sqrt(o.N))).astype(np.complex64)
    o.cb = lambda X: X * H
    x = rand(20 * Ne + 17, True, Ne)
    y = np.concatenate([o.step(x[:3 * Ne + 5]), o.step(x[3 * Ne + 5:])])
    ref = R.ola(x, Ne, o.N, H)
    assert len(y) == len(ref) and relerr(y, ref) <= TOL
    # and the definition is the FIR delayed by Ne - M (fourier.cc:963-966, the pin of test_oracle_pins.py)
    d = Ne - M
    f = R.fir(h, x)
    assert relerr(ref[d:], f[:len(ref) - d]) <= 1e-6                 # (H itself is rounded to complex64)


@pytest.mark.parametrize("N", [64, 100, 1024])
def test_welch(orc, N):
    from oracle import ola_oracle
    x = rand(30 * N + 3, True, N)
    w = ola_oracle.fen_hann_periodique(N)
    S, k = ola_oracle.psd_welch_sum(x, N, w)
    ref, k2 = R.welch_sum(x, N, w)
    assert k == k2 and relerr(S, ref) <= 2e-5


# ---- the known answers of libtsd's tests (tests/test_oracle_pins.py), restated on the float64 definitions
def test_pin_fir_impulse():
    h = np.linspace(1, 31, 31).astype(np.float32)
    x = np.zeros(81, np.float32)
    x[0] = 1
    assert np.array_equal(R.fir(h, x), np.concatenate([h, np.zeros(50)]))


def test_pin_rii_smoother():
    a = np.float32(0.1)
    y = R.rii(np.array([a]), np.array([1.0, -(1 - a)], np.float32), np.ones(20, np.float32))
    ref = np.empty(20)
    ref[0] = a
    for i in range(1, 20):
        ref[i] = np.float64(a) + np.float64(np.float32(1 - a)) * ref[i - 1]
    assert np.abs(y - ref).max() <= 1e-12


def test_pin_decim_correlation():
    hh = np.array([1.0, 2.0, 3.0], np.float32)
    xx = np.arange(1, 13, dtype=np.float32)
    xp = np.concatenate([np.zeros(2), xx])
    ref = np.array([np.dot(hh, xp[a:a + 3]) for a in range(1, 12, 2)])
    assert np.array_equal(R.decim(hh, xx, 2), ref)


def test_pin_decimateur_is_pick():
    x = np.arange(90, dtype=np.float32)
    assert np.array_equal(R.decim(np.array([1.0], np.float32), x, 3), x[2::3])  # one tap: the last of every R
    # (Decimateur keeps x[0::R]: a one-tap decimator keeps the last input of every group, FiltreRIFDecim's phase)


@pytest.mark.parametrize("n", [16, 1, 2, 5, 17, 128])
def test_pin_fft_vs_dft(n):
    x = rand(n, True, n).astype(np.complex128)
    k = np.arange(n)
    D = np.exp(-2j * np.pi * np.outer(k, k) / n) / np.sqrt(n)
    assert np.abs(R.fft(x) - D @ x).max() <= 1e-12 * max(1, n)
    assert np.abs(R.fft(R.fft(x), False) - x).max() <= 1e-12 * max(1, n)


def test_pin_sos_first_sample_seed(orc):
    """Every section starts with its memories equal to its own first input (filtre-rt.cc:361-365): the first output
    of a DF2 section is b0 (x0 - a1 x0 - a2 x0) + b1 x0 + b2 x0, of a DF1 section (b0 + b1 + b2 - a1 - a2) x0."""
    z, p, mn, md = orc.design_butter_lp(4, 0.2)
    x = np.array([3.0, -1.0, 0.5], np.float32)
    for forme in (1, 2):
        co, gain, r1 = orc.SosChain(z, p, mn, md, forme=forme).coefs()
        v = 3.0
        for b0, b1, b2, a1, a2 in co.astype(np.float64):
            v = b0 * (v - a1 * v - a2 * v) + (b1 + b2) * v if forme == 2 else (b0 + b1 + b2 - a1 - a2) * v
        assert abs(R.sos(co, gain, r1, x, forme)[0] - v * np.float64(gain)) <= 1e-12 * abs(v)


def test_error_measures():
    e, m = R.region_err(np.array([1.0, 2, 3, 4]), np.array([1.0, 2.5, 3, 3]), [0, 2, 4])
    assert np.allclose(e, [0.5, 1.0]) and np.allclose(m, [2.5, 3.0])
    assert np.allclose(R.absconv([1, -1], [1, -2, 3]), [1, 3, 5])
    assert np.allclose(R.window_norm(np.array([3.0, 4.0, 0.0, 0.0]), 1), [5, 4, 0, 0])     # blocks [i, i + 1]
    v = np.random.default_rng(2).standard_normal(5000) * np.repeat([1e6, 1e-3, 0.0, 1.0, 1e-3], 1000)
    wn, N = R.window_norm(v, 256), 256
    exact = np.array([np.linalg.norm(v[max(i - N + 1, 0):i + N]) for i in range(len(v))])
    assert (wn >= exact * (1 - 1e-12)).all() and (wn[2303:2560] == 0).all() and (wn[1279:1792] < 1e-1).all()
    assert list(R.windows([0, 5000, 6000], 7000)) == [0, 2048, 4096, 5000, 6000, 7000]
    x, edges, kinds = R.burst_train(np.random.default_rng(1), 100000, 1000)
    assert edges[-1] == 100000 and {"loud", "quiet", "zero"} <= set(kinds)
