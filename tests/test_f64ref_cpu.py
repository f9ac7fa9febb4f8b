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


# ---- the spectral estimators, the correlations and the detector (tests/test_spectral_dynamic_range_gpu.py's references):
# each reference against the oracle on white noise, then each bound "on the reference alone" -- (a) libtsd's float32
# statements (the oracle) stay inside it on the inputs of the GPU tests, (b) a planted defect does not
def _oo():
    from oracle import ola_oracle
    return ola_oracle


def _G():
    import test_spectral_dynamic_range_gpu as G
    return G


@pytest.mark.parametrize("N", [64, 100, 1024])
def test_welch_parts(orc, N):
    x = rand(30 * N + 3, True, N)
    w = _oo().fen_hann_periodique(N)
    S, k = _oo().psd_welch_sum(x, N, w)
    P, B, k2 = R.welch_parts(x, N, w)
    ref, k3 = R.welch_sum(x, N, w)
    assert k == k2 == k3 and relerr(S, P) <= 2e-5 and relerr(P, ref) <= 1e-12
    assert (B > 0).all()


@pytest.mark.parametrize("down", [60, 100])
@pytest.mark.parametrize("N", [64, 1024, 4096, 1000])
def test_welch_bound_holds_for_the_oracle_and_catches_a_dropped_segment(orc, N, down):
    w = _oo().fen_hann_periodique(N)
    x = R.two_tone(N, 40 * N + 3, down)
    P, B, nseg = R.welch_parts(x, N, w)
    S, k = _oo().psd_welch_sum(x, N, w)
    assert k == nseg == 79
    ratio = float((np.abs(S - P) / B).max())
    print("welch oracle / bound", N, down, ratio)
    assert ratio <= (0.05 if N != 1000 else 0.6)              # (a): room to spare (1000: the float32-chirp Bluestein)
    kw = N // 2 + N // 3 + 1                                   # the weak line, fftshift-ed
    assert B[kw] <= 2e-3 * 1e-5 * P.max()                      # ... and the bound there is 500 times (at -100 dB 1e5 times) inside today's 1e-5 of the peak
    # (b) one segment dropped: 1/79 of every line is missing -- outside the bound on the strong line (on the weak one the
    # transform's own share of the bound is 1/85 of the line at -60 dB and 0.7 of it at -100 dB: float32 resolves no better)
    S2, k2 = _oo().psd_welch_sum(x[:-(N // 2)], N, w)
    ks = N // 2 + N // 8
    assert k2 == nseg - 1 and np.abs(S2 - P)[ks] > 100 * B[ks]


class _LeakySpectrum:
    """The oracle's Spectrum whose completed group leaves 2^-20 of its sums in the accumulator."""
    def __init__(self, *a, **k):
        self.o = _oo().Spectrum(*a, **k)

    def step(self, x):
        o = self.o
        if o.cntmag + 1 < o.nmeans:
            return o.step(x)
        nm, o.nmeans = o.nmeans, 1 << 30
        o.step(x)                                              # accumulates only
        o.nmeans, o.cntmag = nm, nm - 1
        acc = o.mag_moy.copy()
        y = o.step(np.zeros(o.BS, np.complex64))               # adds exact zeros, completes the group
        o.mag_moy += acc * np.float32(2.0 ** -20)
        return y


def _spectrum_case(BS, nsubs, nmeans, sweep, make=None):
    oo = _oo()
    Nf = BS // nsubs
    w = oo.fen_hann_periodique(Nf)
    ref = oo.Spectrum(BS, nmeans, nsubs, w, sweep=sweep)
    run = ref if make is None else make(BS, nmeans, nsubs, w, sweep=sweep)
    x = R.spectrum_train(BS, nmeans, BS + nsubs)
    rows = [run.step(x[b * BS:(b + 1) * BS]) for b in range(len(x) // BS)]
    y = np.stack([v for v in rows if len(v)])
    P, B = R.spectrum(x, BS, nsubs, nmeans, ref.f, None if sweep is None else sweep[0], ref.masque, getattr(ref, "mag_cnt", None))
    return y, P, B


def test_spectrum_matches_oracle_on_white_noise(orc):
    oo = _oo()
    for BS, nsubs, nmeans, sweep in [(1024, 1, 3, None), (4096, 4, 2, (700, 3, 20)), (4099, 4, 2, None), (1024, 1, 2, (300, 2, 20))]:
        Nf = BS // nsubs
        ref = oo.Spectrum(BS, nmeans, nsubs, oo.fen_hann_periodique(Nf), sweep=sweep)
        x = rand(2 * nmeans * BS, True, BS)
        y = np.stack([v for v in (ref.step(x[b * BS:(b + 1) * BS]) for b in range(2 * nmeans)) if len(v)])
        P, _ = R.spectrum(x, BS, nsubs, nmeans, ref.f, None if sweep is None else sweep[0], ref.masque, getattr(ref, "mag_cnt", None))
        assert P.shape == y.shape
        lin, _ = R.db_to_linear(y)
        assert relerr(lin, P) <= TOL
        assert np.array_equal(P == 0, y == y.min()) or (P > 0).all()


def test_spectrum_bound_holds_for_the_oracle_and_catches_a_leak(orc):
    floor = np.float32(10) * np.log10(np.float32(R.FLT_MIN), dtype=np.float32)
    for BS, nsubs, nmeans, sweep in _G().SPEC_SHAPES:
        y, P, B = _spectrum_case(BS, nsubs, nmeans, sweep)
        lin, lg = R.db_to_linear(y)
        ratio = float((np.abs(lin - P) / np.maximum(B + lg, 1e-300)).max())
        print("spectrum oracle / bound", BS, nsubs, nmeans, sweep, ratio, "rows dB", y.max(axis=1).round(1))
        assert ratio <= 0.5                                    # (a)
        assert (y[[2, 7]] == floor).all() and (y[P == 0] == floor).all()
        # (b) 2^-20 of a loud group's sums left behind: the quiet row after it is outside its bound
        yl, _, _ = _spectrum_case(BS, nsubs, nmeans, sweep, make=_LeakySpectrum)
        linl, lgl = R.db_to_linear(yl)
        bad = np.abs(linl - P) > B + lgl
        assert bad[1].any() and bad[7].any() and not bad[0].any()


@pytest.mark.parametrize("n,m", [(64, -1), (1000, 10), (777, 300), (512, 512)])
def test_xcorr(orc, n, m):
    oo = _oo()
    x, y = rand(n, True, 1), rand(n, True, 2)
    mm = n if m < 0 else m
    c = np.correlate(x.astype(np.complex128), y.astype(np.complex128), "full")
    want = c[::-1][n - 1 - (mm - 1): n - 1 + mm] / n
    assert np.abs(R.xcorr(x, y, m) - want).max() <= 1e-12
    L = n + 2 * mm
    tol = TOL if L & (L - 1) == 0 else 1.5e-3                  # (the oracle's float32-chirp Bluestein off the powers of two, as in test_fft)
    assert relerr(oo.xcorrb(x, y, m)[1], R.xcorr(x, y, m)) <= tol
    assert relerr(oo.xcorrb(x, None, m)[1], R.xcorr(x, None, m)) <= tol
    w = R.xcorr_weights(n, mm)
    assert np.abs(oo.xcorr(x, y, m)[1] - R.xcorr(x, y, m, True)).max() <= tol * np.abs(want).max() / w.min()


@pytest.mark.parametrize("kind", ["white", "half80", "quietloud"])
@pytest.mark.parametrize("n,m", [(1024, 512), (3072, 512), (65336, 100)])
def test_xcorr_flat_bound_at_power_of_two_sizes(orc, n, m, kind):
    """L = n + 2m a power of two: the oracle's radix-2 plan is within 3 C_FFT u log2(L) ||x|| ||y|| / n of the definition
    (two forward transforms and the inverse one, each normwise; ||X|| = ||x|| for the unitary transform)."""
    L = n + 2 * m
    assert L & (L - 1) == 0
    x, y = _G().xcorr_inputs(n, kind)
    r = _oo().xcorrb(x, y, m)[1]
    flat = _G().xcorr_flat_bound(x, y, n, m)
    e = np.abs(r - R.xcorr(x, y, m)).max()
    print("xcorr oracle / flat bound", n, m, kind, e / flat)
    assert e <= flat
    assert np.abs(np.roll(r, 1) - R.xcorr(x, y, m)).max() > flat          # lags off by one are outside it


def _det_emulation(orc, pu, x, late=0):
    """libtsd's float32 statements of the FIR-mode detector: FiltreRIF with the conjugated reversed pattern, the M-tap
    moving average of |x|^2 (late: that average taken `late` samples late), the score."""
    M = len(pu)
    c = orc.fir(np.conj(pu[::-1]).astype(np.complex64), x)
    a2 = (x.real * x.real + x.imag * x.imag).astype(np.float32)
    e = orc.fir(np.full(M, np.float32(1.0 / M), np.float32), a2)
    if late:
        e = np.concatenate([np.zeros(late, np.float32), e[:-late]])
    m2 = (c.real * c.real + c.imag * c.imag).astype(np.float32)
    m2 = np.where(m2 <= np.float32(1e-12), np.float32(0), m2)
    return (np.float32(1.0 / np.sqrt(np.float32(M))) * np.sqrt(m2 / (e + np.float32(1e-20)))).astype(np.float32)


@pytest.mark.parametrize("M", [31, 200, 513])
def test_detector_bound_holds_for_a_float32_run_and_catches_a_late_energy(orc, M):
    G = _G()
    pat, x, edges, kinds, starts = R.detector_stream(G.DET_SEED + M, M)
    pu = R.unit_pattern(pat)
    d = R.detector(pu, x, 1, threshold=G.DET_THRESHOLD)
    keep = G.det_keep(d)
    assert 1 - keep.mean() <= 1e-3                              # the leave-out share of the GPU test's seeds
    s32 = _det_emulation(orc, pu, x)
    ratio = np.abs(s32 - d["s"]) / np.maximum(d["bound"], 1e-300)
    print("detector M", M, "float32 run / bound", float(ratio[keep].max()), "left out", float(1 - keep.mean()),
          "peaks", len(d["peaks"]), "certain", int((d["margins"] > 2 * d["local"]).sum()))
    assert ratio[keep].max() <= 0.5
    assert (d["margins"] > 2 * d["local"]).sum() >= 20          # the planted patterns give peaks the test can insist on
    late = _det_emulation(orc, pu, x, late=1)
    assert (np.abs(late - d["s"])[keep] > d["bound"][keep]).any()
    # and on white noise the scores agree with the float32 run at the file's tolerance
    xw = rand(20000, True, M)
    dw = R.detector(pu, xw, 1)
    assert relerr(_det_emulation(orc, pu, xw), dw["s"]) <= TOL


def test_detector_ola_mode_is_the_fir_mode_delayed(orc):
    pat, x, _, _, _ = R.detector_stream(5, 31, n=1 << 14)
    pu = R.unit_pattern(pat)
    a, b = R.detector(pu, x, 1, threshold=0.7), R.detector(pu, x, 1024, Ne=512, threshold=0.7)
    D = 512 - 30
    keep = (a["m2"][:-D] > 4e-12 * 1024)
    assert np.abs(b["s"][D:] - a["s"][:-D])[keep].max() <= 1e-12 * (1 + a["s"].max()) and (b["s"][:D] == 0).all()
    assert list(b["peaks"]) == [i + D for i in a["peaks"] if i + D <= len(x) - 31]
    # the engine's own float32 run (the oracle's OLA with the oracle's transform of the pattern) is inside the bound
    oo = _oo()
    p2 = np.zeros(1024, np.complex64)
    p2[:31] = pu
    H = np.conj(orc.fft(p2, True))
    c = oo.Ola(512, 30, None, lambda X: X * H).step(x)
    cb = b["cb"]
    assert (np.abs(c - np.where(b["m2"] <= 1e-12, c, b["c"])) <= cb + 1e-30).all()


def _ola_w_float32(Ne, nz, win, H, x, defect=False):
    """ola_oracle.Ola's windowed branch; defect: `last`'s second half is not cleared (fourier.cc:902 left out)."""
    oo = _oo()
    o = oo.Ola(Ne, nz, win, lambda X: X * H)
    if not defect:
        return o.step(x)
    N, Nz, h = o.N, o.Nz, Ne // 2
    fc = o.fen.astype(np.complex64)
    out = []
    for b in range(len(x) // Ne):
        xb = x[b * Ne:(b + 1) * Ne]
        o.padded[N - h:] = xb[:h]
        o.padded[N - Ne:] *= fc
        x2 = o._tf(o.padded)
        o.svg[Ne - Nz:] += x2[:Nz]
        o.last[h:] += o.svg[:h] / np.float32(2)
        if b > 0:
            out.append(o.last.copy())
        o.last[:h] = o.svg[h:] / np.float32(2)                 # (o.last[h:] = 0 is the statement left out)
        o.svg = x2[N - Ne:].copy()
        o.padded[N - Ne:] = xb * fc
        x2 = o._tf(o.padded)
        o.svg[Ne - Nz:] += x2[:Nz]
        o.last += o.svg / np.float32(2)
        o.svg = x2[Nz:Nz + Ne].copy()
        o.padded[Nz:Nz + h] = xb[h:]
    return np.concatenate(out)


@pytest.mark.parametrize("Ne,nz", [(512, 127), (64, 64), (1000, 24), (4096, 0)])
def test_ola_windowed(orc, Ne, nz):
    G = _G()
    win = _oo().fen_hann_periodique(Ne)
    N = orc.next_pow2(Ne + nz)
    H = G.ola_response(orc, N)
    xw = rand(12 * Ne + 17, True, Ne)
    ref = R.ola_windowed(xw, Ne, N, H, win)
    yo = _ola_w_float32(Ne, nz, win, H, xw)
    assert len(ref) == len(yo) == 11 * Ne and relerr(yo, ref) <= TOL
    assert relerr(_ola_w_float32(Ne, nz, win, H, xw, defect=False), _ola_w_float32(Ne, nz, win, H, xw)) == 0
    # the bound on the GPU test's burst train: (a) the oracle inside, (b) `last` not cleared outside
    x = G.ola_w_input(Ne, N)
    ref = R.ola_windowed(x, Ne, N, H, win)
    bound = G.ola_w_bound(x, N, H, win)[: len(ref)]
    e = np.abs(_ola_w_float32(Ne, nz, win, H, x) - ref)
    print("windowed ola oracle / bound", Ne, nz, float((e / np.maximum(bound, 1e-300)).max()))
    assert (e <= 0.5 * bound).all()
    assert (np.abs(_ola_w_float32(Ne, nz, win, H, x, defect=True) - ref) > bound).any()


@pytest.mark.parametrize("n", [16, 1024, 1000, 6144])
def test_rfft(orc, n):
    x = rand(n, False, n)
    assert relerr(orc.rfft(x), R.rfft(x)) <= (TOL if n & (n - 1) == 0 else 1.5e-3)
