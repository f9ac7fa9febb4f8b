"""Linear operators held to float64 per region, at high dynamic range (the references of tests/f64ref.py).

The parity tests elsewhere measure max|y - ref| against the loudest output of a call: an error confined to the quiet
part of a signal is invisible there.  Here the input is a seeded burst train -- loud segments (1e4, 1e6), quiet
segments (1, 1e-3), exact-zero stretches, lengths random between 300 and 3 W_max so that quiet segments start just
before every kind of tile / block / chunk boundary -- streamed in ragged calls, and every window of at most 2048
outputs (aligned to the segments) is judged on its own:

  direct paths       |y - y64|_i <= gamma_{K+2} (|h| * |x|)_i          (Wilkinson: any float32 evaluation order
                     passes, exact zeros stay exact)
  FFT-based paths    |e_i| <= 8 u log2(N) max|H| ||x[i-N+1 : i+N]||_2  (normwise; N the plan's transform size)
  inexact references max_R|y - y64| <= C max_R|y_orc - y64| + 8 u max_R|y64|
                     (the GPU at most C times as far from float64 as libtsd's own float32 run, per window)

u = 2^-24.  Every constant is fixed below with its derivation; none is tuned per case."""
import numpy as np
import pytest

import f64ref as R

pytestmark = pytest.mark.gpu
U = R.U
C_FFT = 8.0          # normwise FFT constant: the classical bound is ~ log2(N) u per stage with a constant <= 5 (radix-2,
                     # Higham 24.1) -- 8 covers radix-16 / mixed-radix butterflies with FMA contraction and twiddle rounding
# The recursions' per-window factor over libtsd's own float32 error.  Calibration: 0 dB runs of the same filters
# (white noise, no truncation anywhere: test_recursion_calibration_0db) gave worst per-window ratios
# max|y_gpu - y64| / max|y_orc - y64| of 2.52 (5th order 0.1), 2.37 (12th order 0.25, DF2), 2.25 (6th order 0.02),
# 2.16 (12th order complex), 2.02 (12th order DF1), 1.66 and 0.99 for the others: C = 2 x 2.52, rounded down.
C_REC = 5.0


@pytest.fixture(scope="module")
def tg():
    import libtsd_amd as t
    assert t.device_count() >= 1
    return t


def ragged(rng, n, big=False):
    """Cut points of a stream into ragged calls (test_fuzz_gpu.random_chunks' sizes, plus long calls so that the
    multi-chunk layouts of the block-parallel paths are reached)."""
    sizes = [1, 7, 63, 64, 65, 1023, 1024, 2047, 2048, 2049, 5000, 20000, 65537, 262143] + ([1 << 20] * 4 if big else [])
    cuts, o = [], 0
    while o < n:
        c = int(rng.choice(sizes))
        cuts.append((o, min(n, o + c)))
        o += c
    return cuts


def stream(step, x, cuts):
    import torch
    outs = []
    for a, b in cuts:
        y = step(torch.from_numpy(np.ascontiguousarray(x[a:b])).cuda())
        outs.append(y.cpu().numpy())
    torch.cuda.synchronize()
    return np.concatenate(outs)


def assert_componentwise(y, y64, scale, m, cplx_products=False, what=""):
    """|y - y64|_i <= gamma_m scale_i (x sqrt2 for complex x complex products)."""
    g = R.gamma(m) * (np.sqrt(2.0) if cplx_products else 1.0)
    e = np.abs(np.asarray(y).astype(np.complex128) - y64)
    bad = e > g * scale
    worst = float(np.max(e / np.maximum(g * scale, 1e-300)))
    print(what, "worst err / componentwise bound", worst)
    assert not bad.any(), (what, int(np.argmax(bad)), worst)


def assert_windows_vs_reference(y, y64, yorc, edges, C, x=None, what=""):
    """Windows whose input is all exact zeros hold nothing but the filter's decaying tail: libtsd follows it down into
    the subnormals, the block-parallel paths start a chunk from zero state once the tail is below their warm-up bound
     -- relative to a tail there is no float32 accuracy to keep, so those windows are not judged."""
    win = R.windows(edges, len(y64))
    eg, mag = R.region_err(y.astype(np.complex128), y64, win)
    eo = np.max([R.region_err(v.astype(np.complex128), y64, win)[0] for v in (yorc if isinstance(yorc, list) else [yorc])], axis=0)
    if x is not None:
        live = np.array([np.any(x[a:b] != 0) for a, b in zip(win[:-1], win[1:])])
        eg, eo, mag = eg[live], eo[live], mag[live]
        win = np.concatenate([win[:-1][live], [len(y64)]])
    lim = C * eo + 8 * U * mag
    ratio = eg / np.maximum(eo, 1e-300)
    print(what, "worst per-window ratio to libtsd's own error", float(ratio[mag > 0].max(initial=0)),
          "worst err / limit", float((eg / np.maximum(lim, 1e-300)).max()))
    bad = np.nonzero(eg > lim)[0]
    assert len(bad) == 0, (what, [(int(win[i]), float(eg[i]), float(eo[i]), float(mag[i])) for i in bad[:5]])


# ------------------------------------------------------------------------------------------------- direct paths
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("K", [7, 33, 127])
def test_fir_direct(tg, orc, K, cplx):
    rng = np.random.default_rng(K + 10 * cplx)
    h = orc.design_rif_fen(K, "lp", 0.1)
    n = 1 << 20
    x, edges, _ = R.burst_train(rng, n, 2048, cplx)
    f = tg.Fir(h, tg.C64 if cplx else tg.F32, tg.FIR_DIRECT)
    y = stream(f.step, x, ragged(rng, n))
    assert_componentwise(y, R.fir(h, x), R.absconv(h, x), K + 2, what=f"fir direct K={K}")


@pytest.mark.parametrize("no_direct", [False, True])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("Rr,K,kind", [(2, 15, 0), (4, 63, 0), (8, 64, 0), (3, 31, 0), (2, 31, 1)])
def test_decimators(tg, orc, monkeypatch, Rr, K, kind, cplx, no_direct):
    if no_direct:
        monkeypatch.setenv("TSDGPU_POLY_NO_DIRECT", "1")
    rng = np.random.default_rng(Rr * K + cplx)
    c = orc.design_rif_fen(K, "lp", 0.5 / Rr)
    n = (1 << 20) + 3
    x, edges, _ = R.burst_train(rng, n, 1024, cplx)
    f = tg.PolyFir(tg.POLY_HALFBAND if kind else tg.POLY_DECIM, tg.C64 if cplx else tg.F32, c, Rr)
    y = stream(f.step, x, ragged(rng, n))
    ref = R.decim(c, x, Rr, halfband=kind == 1)
    ca = np.abs(c.astype(np.float64))
    if kind:
        ca[1::2] = 0
        ca[K // 2] += 0.5
    scale = np.convolve(ca[::-1], np.abs(x.astype(np.complex128)))[:n][Rr - 1:: Rr]
    assert len(y) == len(ref)
    assert_componentwise(y, ref, scale, K + 2, what=f"decim R={Rr} K={K} kind={kind} nodirect={no_direct}")


@pytest.mark.parametrize("no_direct", [False, True])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("Rr,K", [(2, 15), (4, 63), (3, 31)])
def test_upsamplers(tg, orc, monkeypatch, Rr, K, cplx, no_direct):
    if no_direct:
        monkeypatch.setenv("TSDGPU_POLY_NO_DIRECT", "1")
    rng = np.random.default_rng(Rr * K + 7 * cplx)
    c = orc.design_rif_fen(K, "lp", 0.5 / Rr)
    n = (1 << 19) + 5
    x, edges, _ = R.burst_train(rng, n, 1024, cplx)
    f = tg.PolyFir(tg.POLY_UPS, tg.C64 if cplx else tg.F32, c, Rr)
    y = stream(f.step, x, ragged(rng, n))
    ref = R.ups(c, x, Rr)
    cp = np.abs(R.ups_taps(c, Rr).astype(np.float64))
    W = len(cp) // Rr
    scale = np.zeros(len(ref))
    for i in range(Rr):
        scale[i::Rr] = np.convolve(cp[Rr - 1 - i:: Rr][:W][::-1], np.abs(x.astype(np.complex128)))[:n]
    assert len(y) == len(ref)
    assert_componentwise(y, ref, scale, W + 2, what=f"ups R={Rr} K={K} nodirect={no_direct}")


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("ratio,K,env", [(160 / 147, 15, None), (0.7, 15, None), (1.3, 31, None), (0.9, 127, None),
                                         (0.9, 127, "0")])
def test_resampler(tg, orc, monkeypatch, ratio, K, env, cplx):
    """K = 15: the fused kernel; 31: the generic table-driven kernel; 127: the long interpolator (TSDGPU_RS_LONG=0:
    the generic kernel at the same K)."""
    if env is not None:
        monkeypatch.setenv("TSDGPU_RS_LONG", env)
    rng = np.random.default_rng(K + int(ratio * 100) + cplx)
    n = 1 << 20
    x, edges, _ = R.burst_train(rng, n, 1024, cplx)
    o = orc.Resampler(ratio, K)
    nout, idx, col = orc.Resampler(ratio, K).schedule(n)
    g = tg.Resampler(ratio, tg.C64 if cplx else tg.F32, K=K, lut=o.lut)
    y = stream(g.step, x, ragged(rng, n))
    assert len(y) == nout
    assert_componentwise(y, R.resample(o.lut, idx, col, x), R.resample_bound(o.lut, idx, col, x), K + 2,
                         what=f"resampler {ratio} K={K} env={env}")


# ------------------------------------------------------------------------------------------------- FFT-based paths
def ols_n(K):
    """The 1024-point overlap-save plan serves K < 514 (ols_long.hip's KMIN); above it an upper bound of the long plans'
    transform size."""
    return 1024 if K < 514 else 1 << int(np.ceil(np.log2(8 * K)))


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("K", [127, 900, 3000])
def test_fir_overlap_save(tg, orc, K, cplx):
    """ols.hip's 1024-point plan (K <= 961) and the long / partitioned plans above it.  N: the transform size of the
    1024-point plan, and for the long plans an upper bound (a larger N only widens the norm's window)."""
    rng = np.random.default_rng(K + 3 * cplx)
    h = orc.design_rif_fen(K, "lp", 0.1)
    n = 1 << 20
    N = ols_n(K)
    x, edges, kinds = R.burst_train(rng, n, N, cplx)
    f = tg.Fir(h, tg.C64 if cplx else tg.F32, tg.FIR_OVERLAP_SAVE)
    y = stream(f.step, x, ragged(rng, n))
    Hmax = np.abs(np.fft.fft(h.astype(np.float64), max(N, K))).max()
    # real data: two blocks share one complex transform, so the norm is taken over a half-width of 4N
    bound = C_FFT * U * np.log2(N) * Hmax * R.window_norm(x, N if cplx else 4 * N)
    e = np.abs(y.astype(np.complex128) - R.fir(h, x))
    print("ols K", K, "worst err / normwise bound", float((e / np.maximum(bound, 1e-300)).max()))
    assert (e <= bound).all(), (int(np.argmax(e > bound)), float((e / np.maximum(bound, 1e-300)).max()))


@pytest.mark.parametrize("Ne,M", [(512, 127), (1024, 600), (4096, 2000)])
def test_ola_engine(tg, orc, Ne, M):
    rng = np.random.default_rng(Ne + M)
    h = orc.design_rif_fen(M, "lp", 0.05)
    o = tg.Ola(Ne, M)
    N = o.N
    h2 = np.zeros(N, np.complex64)
    h2[N - M:] = h
    H = (orc.fft(h2, True) * np.float32(np.sqrt(N))).astype(np.complex64)
    o.set_response(H)
    n = 300 * Ne
    x, edges, _ = R.burst_train(rng, n, N, True)
    y = stream(o.step, x, ragged(rng, n))
    ref = R.ola(x, Ne, N, H)
    assert len(y) == len(ref)
    # output t reads the inputs [t - Ne - N, t]: the norm over a half-width of 2N covers them
    bound = C_FFT * U * np.log2(N) * np.abs(H.astype(np.complex128)).max() * R.window_norm(x, 2 * N)[: len(ref)]
    e = np.abs(y - ref)
    print("ola", Ne, M, "worst err / normwise bound", float((e / np.maximum(bound, 1e-300)).max()))
    assert (e <= bound).all(), (int(np.argmax(e > bound)), float((e / np.maximum(bound, 1e-300)).max()))


FFT_SIZES = [(1 << 10, {}), (1 << 12, {}), (1 << 16, {}), (1 << 16, {"TSDGPU_FFT_NO_1K_P1": "1"}), (1 << 20, {}),
             (1 << 22, {}), (3 * 1024, {}), (5 << 12, {}), (27 << 9, {}), (3 << 18, {}), (1 << 12, {"TSDGPU_FFT_GENERIC": "1"})]


@pytest.mark.parametrize("n,env", FFT_SIZES)
def test_fft_plans_rows_and_two_tone(tg, monkeypatch, n, env):
    """Radix-16, four-step / 1024 x C, mixed radix and smooth plans.  (a) A batch whose rows are loud, quiet or zero:
    each row is held to its own norm (a zero row stays exactly zero).  (b) Two tones 100 dB apart: the weak bin and its
    neighbours within the same normwise bound."""
    import torch
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(n)
    B = max(2, min(8, (1 << 23) // n))
    amps = np.array([1e6, 1.0, 0.0, 1e-3, 1e4, 1.0, 0.0, 1e-3])[:B]
    x = ((rng.standard_normal((B, n)) + 1j * rng.standard_normal((B, n))) * amps[:, None]).astype(np.complex64)
    p = tg.Fft(n, B)
    for fwd in (True, False):
        y = p.step(torch.from_numpy(x).cuda(), fwd).cpu().numpy()
        ref = R.fft(x, fwd)
        bound = C_FFT * U * np.log2(n) * np.linalg.norm(x.astype(np.complex128), axis=1)
        e = np.abs(y - ref).max(axis=1)
        print("fft", n, env, fwd, "worst row err / bound", float((e / np.maximum(bound, 1e-300)).max()))
        assert (e <= bound).all(), (e, bound)
    t = np.arange(n)
    k1, k2 = n // 7, n // 3 + 1
    xt = (np.exp(2j * np.pi * k1 * t / n) + 1e-5 * np.exp(2j * np.pi * k2 * t / n)).astype(np.complex64)[None, :]
    yt = tg.Fft(n, 1).step(torch.from_numpy(xt).cuda(), True).cpu().numpy()[0]
    rt = R.fft(xt)[0]
    bound = C_FFT * U * np.log2(n) * np.linalg.norm(xt.astype(np.complex128))
    sl = slice(k2 - 2, k2 + 3)
    assert np.abs(yt[sl] - rt[sl]).max() <= bound and np.abs(yt - rt).max() <= bound


def test_fft_three_pass_2_24(tg):
    import torch
    n = 1 << 24
    rng = np.random.default_rng(24)
    x = np.zeros(n, np.complex64)
    x[: n // 2] = (rng.standard_normal(n // 2) * 1e4).astype(np.float32)
    x[n // 2:] = (rng.standard_normal(n // 2) * 1e-3).astype(np.float32)
    y = tg.Fft(n, 1).step(torch.from_numpy(x).cuda(), True).cpu().numpy()
    e = np.abs(y - R.fft(x)).max()
    bound = C_FFT * U * np.log2(n) * np.linalg.norm(x.astype(np.complex128))
    print("fft 2^24 err / bound", e / bound)
    assert e <= bound


@pytest.mark.parametrize("n", [1000, 1001, 8191, 2187, 10000])
def test_fft_bluestein_two_tone(tg, orc, n):
    """Bluestein sizes carry libtsd's float32 chirp (2e-5 ... 1.5e-3 from float64): held to the
    reference's own error on the two-tone input, over the weak bin's neighbourhood and over the whole transform."""
    import torch
    t = np.arange(n)
    k1, k2 = n // 7, n // 3 + 1
    xt = (np.exp(2j * np.pi * k1 * t / n) + 1e-5 * np.exp(2j * np.pi * k2 * t / n)).astype(np.complex64)
    y = tg.Fft(n, 1).step(torch.from_numpy(xt[None, :].copy()).cuda(), True).cpu().numpy()[0]
    yo = orc.fft(xt)
    r = R.fft(xt)
    for sl in (slice(k2 - 2, k2 + 3), slice(0, n)):
        eg, eo = np.abs(y[sl] - r[sl]).max(), np.abs(yo[sl] - r[sl]).max()
        print("bluestein", n, sl, eg, eo)
        assert eg <= C_REC * eo + 8 * U * np.abs(r[sl]).max()


# ------------------------------------------------------------------------------------------------- recursions
def libtsd_builds(orc, run):
    """run() under both builds of the oracle: libtsd's statements compiled with FMA contraction (x86-64-v3) and without
    (baseline x86-64).  Both are libtsd's float32 run; on an ill-conditioned recursion they differ per window by up to
    15x (6th order at 0.02 on the burst train), so "libtsd's own error" in a window is the larger of the two."""
    import ctypes
    import os
    saved, outs = orc._LIB, []
    names = ["liborc_base.so"] + (["liborc_v3.so"] if orc._cpu_has_v3() else [])
    try:
        for name in names:
            L = ctypes.CDLL(os.path.join(os.path.dirname(orc.__file__), name))
            orc._declare(L)
            orc._LIB = L
            outs.append(run())
    finally:
        orc._LIB = saved
    return outs


def same_chain(orc, ch):
    """A fresh oracle chain (fresh state) on exactly ch's float32 coefficients."""
    c = orc.SosChain(np.zeros(0), np.zeros(0), 1.0)
    c.s = ch.s
    return c


def sos_case(orc, tg, order, fc, cplx, forme=2):
    z, p, mn, md = orc.design_butter_lp(order, fc)
    ch = orc.SosChain(z, p, mn, md, forme=forme)
    co, gain, r1 = ch.coefs()
    return ch, co, gain, r1, tg.Sos(co, gain, tg.C64 if cplx else tg.F32, r1, forme=forme)


SOS_CASES = [(12, 0.25, False, 2), (12, 0.25, True, 2), (6, 0.02, False, 2), (5, 0.1, False, 2), (3, 0.05, True, 2),
             (12, 0.25, False, 1), (4, 0.02, True, 1)]


@pytest.mark.parametrize("order,fc,cplx,forme", SOS_CASES)
def test_recursion_calibration_0db(tg, orc, order, fc, cplx, forme):
    """White noise at one amplitude (no quiet region anywhere): fixes C_REC."""
    rng = np.random.default_rng(order * 100 + forme)
    ch, co, gain, r1, g = sos_case(orc, tg, order, fc, cplx, forme)
    n = 1 << 20
    x = rng.standard_normal(n)
    if cplx:
        x = x + 1j * rng.standard_normal(n)
    x = x.astype(np.complex64 if cplx else np.float32)
    cuts = ragged(rng, n, big=True)
    y = stream(g.step, x, cuts)
    assert_windows_vs_reference(y, R.sos(co, gain, r1, x, forme), ch.step(x), np.array([0, n]), C_REC, x,
                                what=f"sos 0 dB {order} {fc} {cplx} DF{forme}")


# + the exact carry (memories far beyond a chunk: the cost model of sos.hip carries the state instead of warming up)
@pytest.mark.parametrize("order,fc,cplx,forme", SOS_CASES + [(2, 1e-4, False, 2), (3, 1e-3, True, 1)])
def test_sos_burst_train(tg, orc, order, fc, cplx, forme):
    rng = np.random.default_rng(order * 10 + forme + 5 * cplx)
    ch, co, gain, r1, g = sos_case(orc, tg, order, fc, cplx, forme)
    n = 1 << 21
    W = max(int(g.halo), 64)
    x, edges, _ = R.burst_train(rng, n, min(W, 20000), cplx)
    y = stream(g.step, x, ragged(rng, n, big=True))
    yo = libtsd_builds(orc, lambda: same_chain(orc, ch).step(x))
    assert_windows_vs_reference(y, R.sos(co, gain, r1, x, forme), yo, edges, C_REC, x,
                                what=f"sos burst {order} {fc} {cplx} DF{forme} W={g.halo}")


def test_sos_cfg4_2_24_one_call(tg, orc):
    """cfg 4's shape: 12th-order Butterworth at 0.25, 2^24 float samples in one call (the benchmark's chunk layout)."""
    import torch
    rng = np.random.default_rng(44)
    ch, co, gain, r1, g = sos_case(orc, tg, 12, 0.25, False)
    n = 1 << 24
    x, edges, _ = R.burst_train(rng, n, max(int(g.halo), 64))
    y = g.step(torch.from_numpy(x).cuda()).cpu().numpy()
    assert_windows_vs_reference(y, R.sos(co, gain, r1, x), ch.step(x), edges, C_REC, x, what="sos cfg4 2^24")


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("which", ["butter4", "cheby"])
def test_rii_burst_train(tg, orc, which, cplx):
    """FiltreRII, real coefficients, on the burst train.  butter(4, 0.1) fails the create-time cascade check and runs the
    literal recursion (path 2), an ill-conditioned direct form: two equally valid float32 evaluations of it (libtsd's order
    with and without FMA) sit up to 9x apart per window, so one realisation is no yardstick there.  The literal path is held
    to the first-order componentwise bound of any float32 evaluation instead (f64ref.rii_bound); the block-parallel
    sections (cheby1, path 1) to C_REC x libtsd's error."""
    from scipy.signal import butter, cheby1
    b, a = butter(4, 0.1) if which == "butter4" else cheby1(5, 0.5, 0.3)
    nu, de = b.astype(np.float32), a.astype(np.float32)
    rng = np.random.default_rng(len(a) + cplx)
    n = 1 << 20
    x, edges, _ = R.burst_train(rng, n, 2048, cplx)
    g = tg.Rii(nu, de, tg.C64 if cplx else tg.F32)
    y = stream(g.step, x, ragged(rng, n, big=True))
    yo = (orc.RiiC(nu.astype(np.complex64), de.astype(np.complex64)) if cplx else orc.Rii(nu, de)).step(x)
    y64 = R.rii(nu, de, x)
    assert g.path == (2 if which == "butter4" else 1)
    if g.path == 2:
        bnd = R.rii_bound(nu, de, x, y64)
        e = np.abs(y.astype(np.complex128) - y64)
        print("rii literal", which, cplx, "worst err / bound", float((e / np.maximum(bnd, 1e-300)).max()))
        assert (e <= bnd).all(), (int(np.argmax(e > bnd)), float((e / np.maximum(bnd, 1e-300)).max()))
    else:
        assert_windows_vs_reference(y, y64, yo, edges, C_REC, x, what=f"rii {which} {cplx} path {g.path}")


def test_rii_complex_coefficients(tg, orc):
    nu = np.array([0.05 + 0.02j, 0.03 - 0.01j], np.complex64)
    de = np.array([1.0, -0.95 * np.exp(0.3j), 0.2 + 0.1j], np.complex64)
    rng = np.random.default_rng(77)
    n = 1 << 20
    x, edges, _ = R.burst_train(rng, n, 2048, True)
    g = tg.Rii(nu, de, tg.C64)
    y = stream(g.step, x, ragged(rng, n, big=True))
    assert_windows_vs_reference(y, R.rii(nu, de, x), orc.RiiC(nu, de).step(x), edges, C_REC, x, what=f"rii complex path {g.path}")
