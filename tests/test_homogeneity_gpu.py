"""Exact homogeneity and run-to-run determinism of the linear operators.

A linear operator evaluated in float32 without absolute constants in its data path satisfies y(2^k x) = 2^k y(x) bit
for bit as long as nothing overflows or underflows: scaling by a power of two is exact, and every sum, product and
rounding of the scaled evaluation is the scaled image of the unscaled one.  At k = +-60 and the amplitudes below
(|x| ~ 1, taps ~ 1e-4 ... 1, sums of ~ 1e7 terms) nothing does.  A failure means an absolute constant (a guard such as
+1e-30, a clamp, a flush of small partial sums) or a data-dependent path inside a kernel.  Running the same input
twice through fresh handles must also give the same bits (dynamic work hand-out is allowed, non-deterministic
arithmetic is not).  The detector is left out: its 1e-12 floor is libtsd's own (detection.cc:239)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
KS = (60, -60)


@pytest.fixture(scope="module")
def tg():
    import libtsd_amd as t
    assert t.device_count() >= 1
    return t


def rand(n, cplx, seed):
    rng = np.random.default_rng(seed)
    if cplx:
        return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    return rng.standard_normal(n).astype(np.float32)


def run(make, x, cuts=None):
    """A fresh handle from make(), x streamed through it in the given calls (device tensors)."""
    import torch
    op = make()
    cuts = cuts or [(0, len(x))]
    out = [op.step(torch.from_numpy(np.ascontiguousarray(x[a:b])).cuda()).cpu().numpy() for a, b in cuts]
    torch.cuda.synchronize()
    return np.concatenate(out)


def check(make, x, cuts=None, power=1, ks=KS):
    """Determinism, then y(2^k x) == 2^(power k) y(x) for k in ks (+-60; power 2 for quadratic outputs)."""
    y = run(make, x, cuts)
    assert np.array_equal(run(make, x, cuts), y, equal_nan=True), "two runs differ"
    assert np.isfinite(y).all()
    for k in ks:
        s = np.float32(2.0 ** k)
        ys = run(make, (x * s).astype(x.dtype), cuts)
        want = (y * np.float32(2.0 ** (power * k))).astype(y.dtype)
        bad = np.nonzero(ys != want)[0]
        assert len(bad) == 0, (k, len(bad), int(bad[0]), ys[bad[0]], want[bad[0]])


CUTS = [(0, 1), (1, 65538), (65538, 65600), (65600, 300001), (300001, 1 << 19)]


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("K,method", [(7, 1), (33, 1), (127, 1), (127, 2), (900, 2), (3000, 2)])
def test_fir(tg, orc, K, method, cplx):
    h = orc.design_rif_fen(K, "lp", 0.1)
    check(lambda: tg.Fir(h, tg.C64 if cplx else tg.F32, method), rand(1 << 19, cplx, K), CUTS)


def test_fir_complex_taps(tg):
    h = rand(31, True, 3) * np.float32(0.1)
    check(lambda: tg.Fir(h, tg.C64, tg.FIR_DIRECT), rand(1 << 19, True, 4), CUTS)
    check(lambda: tg.Fir(h, tg.C64, tg.FIR_OVERLAP_SAVE), rand(1 << 19, True, 4), CUTS)


@pytest.mark.parametrize("no_direct", [False, True])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("kind,Rr,K", [("decim", 2, 15), ("decim", 4, 63), ("decim", 3, 31), ("half", 2, 31),
                                       ("ups", 2, 15), ("ups", 4, 63), ("ups", 3, 31)])
def test_polyphase(tg, orc, monkeypatch, kind, Rr, K, cplx, no_direct):
    if no_direct:
        monkeypatch.setenv("TSDGPU_POLY_NO_DIRECT", "1")
    c = orc.design_rif_fen(K, "lp", 0.5 / Rr)
    code = {"decim": tg.POLY_DECIM, "half": tg.POLY_HALFBAND, "ups": tg.POLY_UPS}[kind]
    check(lambda: tg.PolyFir(code, tg.C64 if cplx else tg.F32, c, Rr), rand((1 << 19) + 3, cplx, Rr * K), CUTS)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("ratio,K,extra", [(160 / 147, 15, None), (0.7, 31, None), (0.9, 127, None),
                                           (1.3, 0, ("lin", 0)), (0.8, 0, ("lagrange", 3))])
def test_resampler(tg, ratio, K, extra, cplx):
    dt = tg.C64 if cplx else tg.F32
    make = (lambda: tg.Resampler(ratio, dt, analytic=extra)) if extra else (lambda: tg.Resampler(ratio, dt, K=K))
    check(make, rand(1 << 19, cplx, K), CUTS)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("order,fc,forme", [(12, 0.25, 2), (5, 0.1, 2), (4, 0.02, 1), (2, 1e-4, 2)])
def test_sos(tg, orc, order, fc, forme, cplx):
    z, p, mn, md = orc.design_butter_lp(order, fc)
    co, gain, r1 = orc.SosChain(z, p, mn, md, forme=forme).coefs()
    check(lambda: tg.Sos(co, gain, tg.C64 if cplx else tg.F32, r1, forme=forme), rand(1 << 20, cplx, order),
          [(0, 5), (5, 300000), (300000, 1 << 20)])


@pytest.mark.parametrize("cplx", [False, True])
def test_rii(tg, cplx):
    from scipy.signal import butter
    b, a = butter(4, 0.1)
    nu, de = b.astype(np.float32), a.astype(np.float32)
    check(lambda: tg.Rii(nu, de, tg.C64 if cplx else tg.F32), rand(1 << 20, cplx, 9), [(0, 100000), (100000, 1 << 20)])
    nc = np.array([0.05 + 0.02j, 0.03 - 0.01j], np.complex64)
    dc = np.array([1.0, -0.95 * np.exp(0.3j), 0.2 + 0.1j], np.complex64)
    if cplx:
        check(lambda: tg.Rii(nc, dc, tg.C64), rand(1 << 20, True, 10), [(0, 100000), (100000, 1 << 20)])


class _Fft:
    def __init__(self, tg, n, fwd):
        self.p, self.n, self.fwd = tg.Fft(n, 1), n, fwd

    def step(self, x):
        return self.p.step(x.view(-1, self.n), self.fwd).view(-1)


@pytest.mark.parametrize("n", [1 << 10, 1 << 12, 1 << 16, 1 << 20, 1 << 24, 3 * 1024, 10000, 2187, 1000, 8191])
def test_fft(tg, n):
    B = max(1, (1 << 22) // n)
    for fwd in (True, False):
        check(lambda: _Fft(tg, n, fwd), rand(B * n, True, n))


class _Rfft:
    def __init__(self, tg, n):
        self.p, self.n = tg.Rfft(n), n

    def step(self, x):
        return self.p.step(x.view(-1, self.n)).view(-1)


@pytest.mark.parametrize("n", [1 << 10, 1 << 16, 1000])
def test_rfft(tg, n):
    check(lambda: _Rfft(tg, n), rand(max(1, (1 << 20) // n) * n, False, n))


@pytest.mark.parametrize("Ne,M", [(512, 127), (4096, 2000)])
def test_ola(tg, orc, Ne, M):
    h = orc.design_rif_fen(M, "lp", 0.05)

    def make():
        o = tg.Ola(Ne, M)
        h2 = np.zeros(o.N, np.complex64)
        h2[o.N - M:] = h
        o.set_response((orc.fft(h2, True) * np.float32(np.sqrt(o.N))).astype(np.complex64))
        return o
    check(make, rand(200 * Ne + 7, True, Ne), [(0, 3 * Ne + 1), (3 * Ne + 1, 200 * Ne + 7)])


@pytest.mark.parametrize("N", [256, 1000, 1024])
def test_welch(tg, N):
    """|.|^2 sums: quadratic, y(2^k x) = 2^(2k) y(x); k = +-30 keeps the powers inside float32's range."""
    import torch
    from oracle import ola_oracle
    w = ola_oracle.fen_hann_periodique(N)
    x = rand(1 << 20, True, N)

    def go(v):
        return tg.welch(torch.from_numpy(v).cuda(), N, w)[0]
    y = go(x)
    assert np.array_equal(go(x), y)
    for k in (30, -30):
        assert np.array_equal(go((x * np.float32(2.0 ** k)).astype(np.complex64)), (y * np.float32(2.0 ** (2 * k))).astype(np.float32)), k


@pytest.mark.parametrize("n,m", [(1024, 512), (1000, 300)])
def test_xcorr(tg, n, m):
    """Biased cross-correlation, L = n + 2m a power of two (2048) and not (1600): bilinear, so 2^k on EITHER input scales
    every lag by exactly 2^k."""
    x, y = rand(n, True, n), rand(n, True, n + 1)
    r = tg.xcorr(x, y, m, False)
    assert np.array_equal(tg.xcorr(x, y, m, False), r) and np.isfinite(r).all()
    for k in KS:
        s = np.float32(2.0 ** k)
        want = (r * s).astype(np.complex64)
        assert np.array_equal(tg.xcorr((x * s).astype(np.complex64), y, m, False), want), ("x", k)
        assert np.array_equal(tg.xcorr(x, (y * s).astype(np.complex64), m, False), want), ("y", k)


@pytest.mark.parametrize("BS,nsubs,nmeans,sweep", [(1024, 1, 3, None), (4096, 4, 2, None), (4096, 4, 2, (700, 3, 20)), (3000, 3, 2, None)])
def test_spectrum(tg, BS, nsubs, nmeans, sweep):
    """The sums of |X|^2 scale exactly with 4^k; the row is 10 log10f of them, so it moves by the float32 10 log10 of 4^k:
    within 2 ulp of the dB value (the two float32 logarithms).  |x| ~ 1 and k = +-10: FLT_MIN stays far below every bin."""
    from oracle import ola_oracle
    ref = ola_oracle.Spectrum(BS, nmeans, nsubs, ola_oracle.fen_hann_periodique(BS // nsubs), sweep=sweep)
    make = lambda: tg.Spectrum(BS, nsubs, nmeans, ref.f, sweep=None if sweep is None else (sweep[0], ref.masque))
    x = rand(2 * nmeans * BS, True, BS)
    y = make().step(x)
    assert np.array_equal(make().step(x), y) and y.shape[0] == 2
    live = y > -300                                              # (bins the sweep leaves unreached read 10 log10(FLT_MIN) at every k)
    for k in (10, -10):
        ys = make().step((x * np.float32(2.0 ** k)).astype(np.complex64))
        assert np.array_equal(ys[~live], y[~live])
        want = y.astype(np.float64) + 10 * np.log10(4.0) * k
        ulp = np.maximum(np.spacing(np.abs(ys)), np.spacing(np.abs(y))).astype(np.float64)
        bad = np.abs(ys.astype(np.float64) - want)[live] > 2 * ulp[live]
        assert not bad.any(), (k, int(bad.sum()), float((np.abs(ys - want) / ulp)[live].max()))


def test_sharded_sos(tg, orc):
    """The sharded SOS over every device present (several shards per device when there is one)."""
    z, p, mn, md = orc.design_butter_lp(12, 0.25)
    co, gain, r1 = orc.SosChain(z, p, mn, md).coefs()
    nd = tg.device_count()
    ns = max(nd, 4)
    devs = [g % nd for g in range(ns)]
    x = rand(1 << 20, False, 12)

    class _S:
        def __init__(self):
            self.s = tg.Sharded("sos", tg.F32, ns, devs, coefs=co, gain=gain, rii1=r1)

        def step(self, xd):
            import torch
            return torch.from_numpy(self.s.step_host(xd.cpu().numpy()))
    check(_S, x, [(0, 300001), (300001, 1 << 20)])


class _Syn:
    """the synthesizer over a frame-major stream: M samples = one frame of the (M, F) block"""
    def __init__(self, tg, f, M, OS):
        self.s, self.M = tg.Synthesizer(f, M, oversample=OS), M

    def step(self, x):
        return self.s.step(x.view(-1, self.M).t().contiguous())


@pytest.mark.parametrize("bank", ["chan", "syn"])
@pytest.mark.parametrize("M,OS,K", [(8, 1, 5 * 8), (64, 1, 4 * 64 - 3), (1024, 1, 3 * 1024 + 1), (16, 4, 13 * 4), (64, 2, 11 * 32 - 5),
                                    (1024, 2, 1025)])
def test_polyphase_banks(tg, bank, M, OS, K):
    """The four banks (channelizer / synthesizer, plain and oversampled), k in {-20, 7, 30}.  |x| ~ 1 and taps ~ 1/4: at k = 30 a
    product is ~ 1e9 and an output sums at most 16 M <= 2^14 of them, far below 2^128; at k = -20 a product of two small normal
    draws (1e-5 each, say) is 1e-16, far above 2^-126: nothing overflows or goes subnormal.  Ragged steps of odd frame counts:
    the phase of the oversampled banks moves."""
    f = rand(K, False, M + OS) * np.float32(0.25)
    D = M // OS
    frames = [0, 1, 18, 33, 150]
    per = D if bank == "chan" else M
    make = (lambda: tg.Channelizer(f, M, oversample=OS)) if bank == "chan" else (lambda: _Syn(tg, f, M, OS))

    class _Flat:
        def __init__(self):
            self.op = make()

        def step(self, x):
            return self.op.step(x).reshape(-1)
    check(_Flat, rand(150 * per, True, K), [(a * per, b * per) for a, b in zip(frames[:-1], frames[1:])], ks=(-20, 7, 30))
