"""Seeded randomised parity sweep (GPU, through the C ABI, against the oracle): ragged sizes
around every tile / block / sub-tile boundary, random chunkings, unaligned device views."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 1e-5
# TSDGPU_FUZZ_SCALE=N multiplies the number of seeds of every sweep (default 1: seconds per sweep)
SCALE = int(os.environ.get("TSDGPU_FUZZ_SCALE", "1"))


def relerr(y, ref):
    return float(np.abs(y - ref).max() / max(np.abs(ref).max(), 1e-30))


def rand(rng, n, cplx):
    if cplx:
        return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    return rng.standard_normal(n).astype(np.float32)


def random_chunks(rng, n):
    cuts, o = [], 0
    while o < n:
        c = int(rng.choice([1, 7, 63, 64, 65, 895, 896, 897, 1023, 1024, 2047, 2048, 2049, 5000, 20000]))
        cuts.append((o, min(n, o + c)))
        o += c
    return cuts


@pytest.fixture(scope="module")
def tg():
    import libtsd_amd as t
    assert t.device_count() >= 1
    return t


@pytest.mark.parametrize("seed", range(12 * SCALE))
def test_fuzz_fir(tg, orc, seed):
    rng = np.random.default_rng(1000 + seed)
    cplx = bool(rng.integers(2))
    ctaps = cplx and bool(rng.integers(2))
    K = int(rng.choice([1, 3, 16, 39, 40, 47, 48, 63, 64, 65, 127, 129, 193, 257, 513, 514, 640, 897, 898, 1000, 1025, 2500, 4097, 5000]))
    n = int(rng.choice([1, 100, 895, 896, 897, 1791, 1792, 1793, 4096, 30000, 70001]))
    h = rand(rng, K, ctaps) / np.float32(max(1.0, np.sqrt(K)))
    x = rand(rng, n + 5000, cplx)
    ref = orc.fir(h, x)
    for method in (tg.FIR_AUTO, tg.FIR_DIRECT, tg.FIR_OVERLAP_SAVE):
        f = tg.Fir(h, tg.C64 if cplx else tg.F32, method)
        y = np.concatenate([f.step(x[a:b].copy()) for a, b in random_chunks(rng, len(x))])
        assert relerr(y, ref) <= TOL, (seed, method, K, n, cplx, ctaps)


@pytest.mark.parametrize("seed", range(8 * SCALE))
def test_fuzz_sos(tg, orc, seed):
    rng = np.random.default_rng(2000 + seed)
    cplx = bool(rng.integers(2))
    order = int(rng.choice([1, 2, 3, 6, 12]))
    fc = float(rng.choice([0.05, 0.1, 0.25, 0.4]))
    forme = int(rng.choice([1, 2]))
    z, p, mn, md = orc.design_butter_lp(order, fc)
    ref = orc.SosChain(z, p, mn, md, forme=forme)
    co, gain, r1 = ref.coefs()
    g = tg.Sos(co, gain, tg.C64 if cplx else tg.F32, r1, forme=forme)
    x = rand(rng, int(rng.choice([1, 2047, 2049, 40000, 100001])), cplx)
    yref = ref.step(x)
    y = np.concatenate([g.step(x[a:b].copy()) for a, b in random_chunks(rng, len(x))])
    assert relerr(y, yref) <= TOL, (seed, order, fc, forme, cplx)


@pytest.mark.parametrize("seed", range(3 * SCALE))
def test_fuzz_sos_long_memory(tg, orc, seed):
    """cut-offs of 1e-5 ... 1e-2: the warm-up scheme, the exact carry of the state from chunk to chunk and the
    sequential chunk, whichever the call's length selects; ragged calls; the float64 run of the chain arbitrates"""
    from scipy.signal import lfilter, lfiltic
    rng = np.random.default_rng(2500 + seed)
    cplx = bool(rng.integers(2))
    order = int(rng.choice([1, 2, 3, 4, 6]))
    fc = float(10.0 ** rng.uniform(-5, -2))
    forme = int(rng.choice([1, 2]))
    z, p, mn, md = orc.design_butter_lp(order, fc)
    ref = orc.SosChain(z, p, mn, md, forme=forme)
    co, gain, r1 = ref.coefs()
    g = tg.Sos(co, gain, tg.C64 if cplx else tg.F32, r1, forme=forme)
    x = rand(rng, int(rng.choice([16384, 70000, 300001])), cplx) + np.float32(rng.uniform(-1, 1))
    yref = ref.step(x)
    if forme == 2:
        # the oracle's own float64 run of the DF2 chain (real data; real coefficients: the two channels apart)
        v = ref.run_f64(x.real) + 1j * ref.run_f64(x.imag) if cplx else ref.run_f64(x)
    else:
        # FormeDirecte1: every memory of a section = its first input (filtre-rt.cc:361-365); the trailing first-order
        # section starts from zero and carries the gain (:407-437,567-570)
        v = x.astype(np.complex128 if cplx else np.float64)
        for b0, b1, b2, a1, a2 in np.asarray(co, np.float32).astype(np.float64).reshape(-1, 5):
            zi = lfiltic([b0, b1, b2], [1.0, a1, a2], y=[v[0], v[0]], x=[v[0], v[0]])
            v, _ = lfilter([b0, b1, b2], [1.0, a1, a2], v, zi=zi.astype(v.dtype))
        if r1 is not None:
            q = np.asarray(r1, np.float32).astype(np.float64)
            v = lfilter([q[0], q[1]], [1.0, q[2]], v)
        else:
            v = v * np.float64(np.float32(gain))
    y = np.concatenate([g.step(x[a:b].copy()) for a, b in random_chunks(rng, len(x))])
    bruit = relerr(yref, v)
    # (as close to the float64 answer as the reference's own float32 run is; where that run is itself 1e-4 or more off --
    # order 6 at fc = 1e-5: states of 1e8 whose ulp exceeds the input -- two float32 evaluations are two noise
    # realisations: factor 6, the band of test_sos_slow_decay -- 1 case in 4500 of a 1500x soak reached 4.02)
    assert relerr(y, v) <= max(2e-5, bruit if bruit < 1e-4 else 6 * bruit), (seed, order, fc, forme, cplx, len(x), relerr(y, v), bruit)


@pytest.mark.parametrize("seed", range(8 * SCALE))
def test_fuzz_resampler(tg, orc, seed):
    rng = np.random.default_rng(3000 + seed)
    cplx = bool(rng.integers(2))
    ratio = float(np.float32(rng.uniform(0.5, 1.999)))
    x = rand(rng, int(rng.choice([1, 15, 511, 512, 513, 2047, 2049, 33333])), cplx)
    K, nph = [(15, 256), (15, 256), (4, 256), (31, 128), (127, 256), (64, 1024)][int(rng.integers(6))]
    ref = orc.Resampler(ratio, K=K, nphases=nph, fcut=0.4)
    yref = ref.step(x)
    g = tg.Resampler(ratio, tg.C64 if cplx else tg.F32, K=K, nphases=nph, lut=ref.lut)
    parts = [g.step(x[a:b].copy()) for a, b in random_chunks(rng, len(x))]
    y = np.concatenate(parts) if parts else np.zeros(0, x.dtype)
    assert len(y) == len(yref), (seed, ratio)
    if len(y):
        assert relerr(y, yref) <= TOL, (seed, ratio, cplx, K, nph)


@pytest.mark.parametrize("seed", range(6 * SCALE))
def test_fuzz_fft(tg, orc, seed):
    rng = np.random.default_rng(4000 + seed)
    n = int(rng.choice([6, 12, 16, 30, 32, 48, 64, 96, 255, 256, 600, 1024, 1536, 2048, 3000, 4096, 5120, 8192, 16384, 15360, 32768, 65536,
                        1 << 17, 3 << 15]))
    batch = int(rng.integers(1, 4))
    x = rand(rng, batch * n, True).reshape(batch, n)
    p = tg.Fft(n)
    for fwd in (True, False):
        y = p.step(x, fwd)
        for b in range(batch):
            assert relerr(y[b], orc.fft(x[b], fwd)) <= TOL, (seed, n, fwd)


@pytest.mark.parametrize("seed", range(6 * SCALE))
def test_fuzz_polyphase(tg, orc, seed):
    rng = np.random.default_rng(6000 + seed)
    cplx = bool(rng.integers(2))
    kind = int(rng.integers(3))
    R = int(rng.choice([2, 3, 4, 7, 16, 33]))
    K = int(rng.choice([3, 15, 16, 31, 64, 101]))
    h = orc.design_rif_fen(K, "lp", 0.45 / R)
    x = rand(rng, int(rng.choice([1, 100, 4095, 4096, 4097, 30011])), cplx)
    dt = tg.C64 if cplx else tg.F32
    if kind == 0:
        ref, g = orc.PolyDecim(h, R, 0), tg.PolyFir(tg.POLY_DECIM, dt, h, R)
    elif kind == 1:
        ref, g = orc.PolyDecim(h, 2, 1), tg.PolyFir(tg.POLY_HALFBAND, dt, h)
    else:
        ref, g = orc.PolyUps(h, R), tg.PolyFir(tg.POLY_UPS, dt, h, R)
    yref = ref.step(x)
    parts = [g.step(x[a:b].copy()) for a, b in random_chunks(rng, len(x))]
    y = np.concatenate(parts) if parts else np.zeros(0, x.dtype)
    assert len(y) == len(yref), (seed, kind, R, K)
    if len(y):
        assert relerr(y, yref) <= TOL, (seed, kind, R, K, cplx)


def test_device_views_unaligned(tg, orc):
    """device tensors that are only 4- or 8-byte aligned (odd offsets into a larger buffer)"""
    import torch
    rng = np.random.default_rng(5)
    x = rand(rng, 50003, False)
    xd = torch.from_numpy(x).cuda()
    h = orc.design_rif_fen(127, "lp", 0.05)
    for off in (1, 2, 3):
        f = tg.Fir(h, tg.F32, tg.FIR_AUTO)
        y = f.step(xd[off:])
        torch.cuda.synchronize()
        assert relerr(y.cpu().numpy(), orc.fir(h, x[off:])) <= TOL
    z, p, mn, md = orc.design_butter_lp(6, 0.2)
    ref = orc.SosChain(z, p, mn, md)
    co, gain, r1 = ref.coefs()
    g = tg.Sos(co, gain, tg.F32, r1)
    y = g.step(xd[3:])
    torch.cuda.synchronize()
    assert relerr(y.cpu().numpy(), ref.step(x[3:])) <= TOL


# ---- round 2: the operators added since (FiltreRII paths, OLA engine, real FFT, correlations, sharded steps) ----------
@pytest.mark.parametrize("seed", range(8 * SCALE))
def test_fuzz_rii(tg, orc, seed):
    rng = np.random.default_rng(7000 + seed)
    order = int(rng.integers(1, 11))
    npair = order // 2
    rad = rng.uniform(0.2, 0.93, npair)
    ang = rng.uniform(0.05, 3.09, npair)
    poles = np.concatenate([rad * np.exp(1j * ang), rad * np.exp(-1j * ang), [rng.uniform(-0.9, 0.9)] if order & 1 else []])
    de = (np.real(np.poly(poles)) * rng.uniform(0.5, 2.0)).astype(np.float32)
    nu = rng.standard_normal(int(rng.integers(1, order + 3))).astype(np.float32)
    cplx = bool(rng.integers(2))
    n = int(rng.choice([1, 2, 63, 2047, 2048, 2049, 40000, 200001]))
    x = rand(rng, n, cplx)
    if cplx:
        ref = (orc.Rii(nu, de).step(x.real.copy()) + 1j * orc.Rii(nu, de).step(x.imag.copy())).astype(np.complex64)
    else:
        ref = orc.Rii(nu, de).step(x)
    f = tg.Rii(nu, de, tg.C64 if cplx else tg.F32)
    y = np.concatenate([f.step(x[a:b].copy()) for a, b in random_chunks(rng, n)])
    if relerr(y, ref) > TOL:
        # a direct form of order ~10 with poles near the circle amplifies its OWN float rounding past the band (the
        # create-time check sends exactly these to the literal kernel): then the float64 answer arbitrates -- the GPU
        # result must be as close to it as the reference recursion's float32 run is (within a small factor)
        from scipy.signal import lfilter
        exact = lfilter(nu.astype(np.float64), de.astype(np.float64), x.astype(np.complex128 if cplx else np.float64))
        # (factor 4: two float32 evaluation orders of such a recursion are two noise realisations -- 1 case in 12000 of a
        # 1500x soak reached 2.3x)
        assert relerr(y, exact) <= 4 * relerr(ref, exact), (seed, order, f.path, n, cplx, relerr(y, ref), relerr(ref, exact))


@pytest.mark.parametrize("seed", range(6 * SCALE))
def test_fuzz_ola(tg, orc, seed):
    from oracle import ola_oracle
    rng = np.random.default_rng(8000 + seed)
    Ne = int(rng.choice([2, 16, 100, 256, 512, 1000, 2048, 4096]))
    windowed = bool(rng.integers(2)) and Ne % 2 == 0
    nz = int(rng.choice([0, 1, Ne // 3, Ne, 2 * Ne + 5]))
    win = ola_oracle.fen_hann_periodique(Ne) if windowed else None
    N = 1 << int(np.ceil(np.log2(max(Ne + nz, 1))))
    if N - Ne > Ne:
        # more zeros than samples: the reference's svg.tail(N_zeros) leaves its Ne-sample vector (fourier.cc:866) -> error
        with pytest.raises(tg.TsdGpuError):
            tg.Ola(Ne, nz, win)
        return
    g = tg.Ola(Ne, nz, win)
    H = (rng.standard_normal(g.N) + 1j * rng.standard_normal(g.N)).astype(np.complex64)
    g.set_response(H)
    ref = ola_oracle.Ola(Ne, nz, win, lambda X: X * H)
    assert (g.N, g.Ne) == (ref.N, ref.Ne), (seed, Ne, nz)
    for _ in range(6):
        n = int(rng.choice([0, 1, Ne - 1, Ne, Ne + 1, 3 * Ne + 7, 10 * Ne]))
        x = rand(rng, n, True)
        y, yr = g.step(x), ref.step(x)
        assert y.shape == yr.shape, (seed, Ne, nz, windowed, n)
        if len(yr):
            assert np.abs(y - yr).max() <= TOL * max(np.abs(yr).max(), 1.0) * 4, (seed, Ne, nz, windowed, n)


@pytest.mark.parametrize("seed", range(3 * SCALE))
def test_fuzz_welch(tg, orc, seed):
    """psd_welch sums: the fused kernels (powers of two from 16 to 16384: runs of segments per transform, partial groups at
    the end of a call), the in-wave one (1024) and the framed-transform path (other sizes), on host and resident data"""
    from oracle import ola_oracle as oo
    import torch
    rng = np.random.default_rng(9200 + seed)
    N = int(rng.choice([2, 16, 32, 64, 100, 128, 256, 512, 1000, 1024, 2048, 4096, 8192, 16384]))
    nseg = int(rng.choice([0, 1, 2, 3, 17, 64, 65, 200]))
    n = max(0, nseg * (N // 2) + N + int(rng.integers(0, max(N // 2, 1)))) if nseg else int(rng.integers(0, N + 1))
    n = min(n, 3_000_000)
    x = rand(rng, n, True)
    w = oo.fen_hann_periodique(N) if N > 2 else np.ones(N, np.float32)
    ref, nref = oo.psd_welch_sum(x, N, w)
    S, ns = tg.welch(x, N, w)
    assert ns == nref, (seed, N, n)
    assert np.abs(S - ref).max() <= TOL * max(float(ref.max()), 1e-30), (seed, N, n)
    if n:
        S2, _ = tg.welch(torch.from_numpy(x).cuda(), N, w)
        assert np.abs(S2 - ref).max() <= TOL * max(float(ref.max()), 1e-30), (seed, N, n, "resident")


@pytest.mark.parametrize("seed", range(4 * SCALE))
def test_fuzz_rfft_and_correlations(tg, orc, seed):
    from oracle import ola_oracle as oo
    rng = np.random.default_rng(9000 + seed)
    n = int(rng.choice([2, 4, 30, 64, 100, 1024, 1000, 4096, 6144, 32768]))
    x = rand(rng, n, False)
    assert relerr(tg.rfft(x), orc.rfft(x)) <= TOL, (seed, n)
    nc = int(rng.choice([8, 100, 1000, 5000]))
    a, b = rand(rng, nc, True), rand(rng, nc, True)
    m = int(rng.choice([-1, 1, nc // 2, nc]))
    ref = oo.xcorrb(a, b, m)[1]
    got = tg.xcorr(a, b, m, False)
    assert got.shape == ref.shape
    # (the band is set by the scale of the correlation -- its zero lag bound sqrt(Ea Eb) / n -- not by the few lags asked for,
    # which may be small by cancellation: a 600x soak had a single lag at 1e-3 of that scale)
    echelle = max(float(np.abs(ref).max()), float(np.sqrt(np.mean(np.abs(a) ** 2) * np.mean(np.abs(b) ** 2))))
    assert np.abs(got - ref).max() <= 1e-5 * echelle, (seed, nc, m)


@pytest.mark.parametrize("seed", range(4 * SCALE))
def test_fuzz_sharded(tg, orc, seed):
    """N logical shards on the one device against the single handle, random call lengths (incl. shorter than the halo)"""
    rng = np.random.default_rng(9500 + seed)
    N = int(rng.integers(2, 9))
    kind = ["fir", "sos", "resampler"][int(rng.integers(3))]
    if kind == "fir":
        K = int(rng.choice([2, 31, 127, 600]))
        h = orc.design_rif_fen(K, "lp", 0.1) if K > 2 else np.array([0.5, 0.5], np.float32)
        method = tg.FIR_DIRECT
        sh, one = tg.Sharded("fir", tg.C64, N, taps=h, method=method), tg.Fir(h, tg.C64, method)
        exact = True
    elif kind == "sos":
        from scipy.signal import butter
        sos = butter(int(rng.choice([2, 6, 12])), float(rng.uniform(0.1, 0.6)), output="sos")
        co = np.array([[s[0], s[1], s[2], s[4], s[5]] for s in sos], np.float32)
        sh, one = tg.Sharded("sos", tg.C64, N, coefs=co), tg.Sos(co, 1.0, tg.C64)
        exact = False
    else:
        ratio = float(rng.choice([160 / 147, 0.75, 1.9, 0.51]))
        sh, one = tg.Sharded("resampler", tg.C64, N, ratio=ratio), tg.Resampler(ratio, tg.C64)
        exact = True
    crete = 1e-3                  # the stream's peak so far: float rounding scales with it, not with a one-sample call's own value
    for _ in range(4):
        n = int(rng.choice([1, 5, 100, 3000, 50001, 300000]))
        x = rand(rng, n, True)
        ys, y1 = sh.step_host(x), one.step(x)
        if len(y1):
            crete = max(crete, float(np.abs(y1).max()))
        assert ys.shape == y1.shape, (seed, kind, N, n)
        if not len(y1):
            continue
        if exact:
            assert np.array_equal(ys, y1), (seed, kind, N, n)
        else:
            # (shards shift the tiling and the warm-up of the cascade: float rounding, 2.1e-6 at worst in a 600x soak; the bar is 1e-5)
            assert np.abs(ys - y1).max() <= 5e-6 * crete, (seed, kind, N, n)


@pytest.mark.parametrize("seed", range(8 * SCALE))
def test_fuzz_resampler_wide(tg, orc, seed):
    """the whole accepted ratio range (1/64 .. 8), short and long tables, the analytic interpolators; a configuration the
    kernel cannot hold must be refused at CREATE time"""
    rng = np.random.default_rng(3500 + seed)
    cplx = bool(rng.integers(2))
    ratio = float(np.float32(np.exp(rng.uniform(np.log(1 / 64), np.log(8.0)))))
    n = int(rng.choice([1, 64, 511, 513, 4097, 33333]))
    x = rand(rng, n, cplx)
    dt = tg.C64 if cplx else tg.F32
    flavour = int(rng.integers(4))
    try:
        if flavour == 0:
            ref, g = orc.Resampler(ratio, analytic=("lin", 0)), tg.Resampler(ratio, dt, analytic=("lin", 0))
        elif flavour == 1:
            d = int(rng.choice([1, 2, 3, 5, 7]))
            ref, g = orc.Resampler(ratio, analytic=("lagrange", d)), tg.Resampler(ratio, dt, analytic=("lagrange", d))
        else:
            K, nph = [(2, 16), (7, 64), (15, 256), (31, 256), (24, 1000)][int(rng.integers(5))]
            ref = orc.Resampler(ratio, K=K, nphases=nph, fcut=float(min(0.4, ratio / 2)))
            g = tg.Resampler(ratio, dt, K=K, nphases=nph, lut=ref.lut)
    except tg.TsdGpuError as e:
        assert "LDS" in str(e) or "UNSUPPORTED" in str(e) or "needs" in str(e), str(e)
        return
    yref = ref.step(x)
    parts = [g.step(x[a:b].copy()) for a, b in random_chunks(rng, n)]
    y = np.concatenate(parts) if parts else np.zeros(0, x.dtype)
    assert len(y) == len(yref), (seed, ratio, flavour)
    if len(y):
        assert relerr(y, yref) <= TOL, (seed, ratio, cplx, flavour)


@pytest.mark.parametrize("seed", range(3 * SCALE))
def test_fuzz_detector(tg, orc, seed):
    """patterns planted at random places (block borders included) are all found, once, at their place"""
    rng = np.random.default_rng(9800 + seed)
    M = int(rng.choice([31, 64, 127, 200]))
    Ne = int(rng.choice([512, 1024, 4096]))
    mode = int(rng.integers(2))
    nblk = 8
    pat = rand(rng, M, True)
    x = (0.01 * rand(rng, Ne * nblk, True)).astype(np.complex64)
    starts, s = [], int(rng.integers(0, Ne))
    while s + 3 * M < Ne * (nblk - 2):
        starts.append(s)
        x[s:s + M] += np.complex64((0.5 + rng.uniform(0, 1)) * np.exp(1j * rng.uniform(0, 6.28))) * pat
        s += int(rng.integers(2 * M + 1, 2 * Ne))
    det = tg.Detector(pat, Ne, mode, threshold=0.8)
    found = []
    for b in range(nblk):
        _, pk = det.step(x[b * Ne:(b + 1) * Ne].copy())
        found += [b * Ne + p.index - det.delay for p in pk]
    assert found == starts, (seed, M, Ne, mode)


# ---- round 3: the polyphase banks (channelizer / synthesizer, plain and oversampled), per frame against float64 -----------
def _bank_stream(make, data, cut, steps, D, rows):
    """the stream through a handle in `steps` (frame counts); at frame `cut` its state and phase move to a fresh handle, and both
    go on: -> (the first handle's output, the two continuations)"""
    import torch
    part = (lambda a, b: data[:, a:b]) if rows else (lambda a, b: data[a * D:(b) * D])
    first, fresh, outs, tail, o = make(), None, [], [], 0
    for f in steps:
        if o == cut:
            fresh = make()
            fresh.set_state(first.get_state())
            fresh.phase = first.phase
        y = first.step(part(o, o + f))
        outs.append(y)
        if fresh is not None:
            tail.append((y, fresh.step(part(o, o + f))))
        o += f
    torch.cuda.synchronize()
    cat = (lambda v: torch.cat(v)) if rows else (lambda v: torch.cat(v, dim=1))
    return cat(outs).cpu().numpy(), cat([a for a, _ in tail]).cpu().numpy(), cat([b for _, b in tail]).cpu().numpy()


@pytest.mark.parametrize("pair", ["plain", "oversampled"])
@pytest.mark.parametrize("seed", range(40 * SCALE))
def test_fuzz_polyphase_banks(tg, pair, seed):
    """random (M, OS, K in [1, 16 D], frames, ragged steps) through the channelizer and the synthesizer of the pair: every frame /
    sample inside its float64 bound (tests/poly_f64.py), and a hand-over of state + phase to a fresh handle at a random cut gives
    the same bits"""
    import torch
    import poly_f64 as PF
    rng = np.random.default_rng([10000, pair == "oversampled", seed])
    M = int(rng.choice([8, 16, 32, 64, 128, 256, 512, 1024]))
    OS = 1 if pair == "plain" else int(rng.choice([2, 4]))
    D = M // OS
    F = int(rng.integers(1, 401))
    for bank in ("chan", "syn"):
        K = int(rng.integers(1, 16 * D + 1))
        h = PF.taps(rng, K)
        steps = PF.ragged(rng, F)
        cut = int(np.concatenate([[0], np.cumsum(steps)])[rng.integers(len(steps))])
        what = (seed, bank, M, OS, K, F, cut)
        if bank == "chan":
            x = PF.chan_input(rng, F * D, M)
            ref, bound = PF.chan(x, PF.chan_table(h, M), M, OS)
            y, ya, yb = _bank_stream(lambda: tg.Channelizer(h, M, oversample=OS), torch.from_numpy(x).cuda(), cut, steps, D, False)
            ratio = PF.chan_judge(y, ref, bound, what)
        else:
            u = PF.syn_input(rng, M, F)
            ref, bound = PF.syn(u, PF.syn_table(h, D), M, OS)
            y, ya, yb = _bank_stream(lambda: tg.Synthesizer(h, M, oversample=OS), torch.from_numpy(u).cuda(), cut, steps, D, True)
            ratio = PF.syn_judge(y, ref, bound, what)
        print(what, "worst err / bound", ratio)
        assert ratio <= 1.0, what
        assert np.array_equal(ya.view(np.uint32), yb.view(np.uint32)), what
