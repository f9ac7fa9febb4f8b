"""GPU parity of the SOS/biquad IIR path (C ABI tsdgpu_sos_*) against the CPU oracle
(restatement of ChaineSOIS/SOIS/RIIFoS, filtre-rt.cc:303-602).
Tolerance: max|y - y_ref| <= 1e-5 * max|y_ref| (the block-parallel recursion re-associates)."""
import numpy as np
import pytest

from conftest import perf_guard

pytestmark = pytest.mark.gpu
TOL = 1e-5


def relerr(y, ref):
    return float(np.abs(y - ref).max() / max(np.abs(ref).max(), 1e-30))


def rand(n, cplx, seed):
    rng = np.random.default_rng(seed)
    if cplx:
        return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    return rng.standard_normal(n).astype(np.float32)


@pytest.fixture(scope="module")
def tg():
    import libtsd_amd as t
    assert t.device_count() >= 1
    return t


def chains(orc, tg, order, fcut, cplx):
    z, p, mn, md = orc.design_butter_lp(order, fcut)
    ref = orc.SosChain(z, p, mn, md)
    co, gain, r1 = ref.coefs()
    return ref, tg.Sos(co, gain, tg.C64 if cplx else tg.F32, r1)


# BASELINE configs[3] design: 12th-order Butterworth lp 0.25 -> 6 DF2 sections (design_riia)
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("n", [1, 7, 2047, 2048, 2049, 100000, 300001])
def test_sos_butter12(tg, orc, cplx, n):
    ref, g = chains(orc, tg, 12, 0.25, cplx)
    assert 0 < g.halo <= 1024
    x = rand(n, cplx, n)
    assert relerr(g.step(x), ref.step(x)) <= TOL


# odd order -> trailing first-order section RIIFoS carrying the gain (filtre-rt.cc:530-556)
@pytest.mark.parametrize("order", [1, 3, 5])
def test_sos_odd_order(tg, orc, order):
    ref, g = chains(orc, tg, order, 0.1, False)
    x = rand(50000, False, order)
    assert relerr(g.step(x), ref.step(x)) <= TOL


# slowly decaying filter: long warm-up, few chunks (narrow-band low-pass)
@pytest.mark.parametrize("fc", [0.01, 0.001])
def test_sos_slow_decay(tg, orc, fc):
    ref, g = chains(orc, tg, 4, fc, False)
    assert g.halo > 1024
    x = rand(400000, False, 11)
    yref = ref.step(x)
    y = g.step(x)
    # A narrow-band DF2 cascade is ill-conditioned in float32: the reference's own rounding
    # noise (oracle vs the same recurrence in double) reaches 2e-4 at fc = 0.001, far above
    # 1e-5, so "parity" can only mean: as close to the exact result as the reference is,
    # within a small factor (any re-association, or -ffp-contract, moves it that much).
    y64 = ref.run_f64(x)
    noise = relerr(yref, y64)
    assert relerr(y, y64) <= max(TOL, 5 * noise)
    assert relerr(y, yref) <= max(TOL, 6 * noise)


# streaming: state (and the first-call seed) carried across ragged chunks
@pytest.mark.parametrize("bs", [100000, 4096, 1000, 311, 1])
def test_sos_streaming(tg, orc, bs):
    ref, g = chains(orc, tg, 12, 0.25, False)
    n = 250000 if bs > 1 else 200
    x = rand(n, False, 5)
    yref = ref.step(x)
    y = np.concatenate([g.step(x[o:o + bs].copy()) for o in range(0, n, bs)])
    assert relerr(y, yref) <= TOL


def test_sos_seed_is_first_sample(tg, orc):
    # constant input: with the d1 = d2 = x(0) seed of every section the response differs
    # from a zero-state start; the GPU path must reproduce the reference's quirk exactly
    ref, g = chains(orc, tg, 12, 0.25, False)
    x = np.full(5000, 3.0, np.float32)
    yref = ref.step(x)
    assert relerr(g.step(x), yref) <= TOL
    z, p, mn, md = orc.design_butter_lp(12, 0.25)
    co, gain, _ = orc.SosChain(z, p, mn, md).coefs()
    assert abs(yref[0]) > 10 * abs(3.0 * gain)     # not the zero-state value b0-product * x


def test_sos_device_inplace_reset(tg, orc):
    import torch
    ref, g = chains(orc, tg, 12, 0.25, True)
    x = rand(200000, True, 6)
    yref = ref.step(x)
    xd = torch.from_numpy(x).cuda()
    yd = g.step(xd)
    torch.cuda.synchronize()
    assert relerr(yd.cpu().numpy(), yref) <= TOL
    g.reset()
    g.step(xd, xd)
    torch.cuda.synchronize()
    assert relerr(xd.cpu().numpy(), yref) <= TOL
    with pytest.raises(tg.TsdGpuError):
        tg.Sos(np.zeros((1, 5), np.float32), 1.0, tg.F32, None, forme=3)


# FormeDirecte1 (filtre-rt.cc:384-393): same transfer function, different arithmetic and a
# four-value first-call seed x1 = x2 = y1 = y2 = x(0)
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("order,fc", [(12, 0.25), (5, 0.1), (4, 0.02)])
def test_sos_forme_directe_1(tg, orc, cplx, order, fc):
    z, p, mn, md = orc.design_butter_lp(order, fc)
    ref = orc.SosChain(z, p, mn, md, forme=1)
    co, gain, r1 = ref.coefs()
    g = tg.Sos(co, gain, tg.C64 if cplx else tg.F32, r1, forme=1)
    x = rand(150000, cplx, order)
    yref = ref.step(x)
    y = np.concatenate([g.step(x[o:o + 40000].copy()) for o in range(0, len(x), 40000)])
    assert relerr(y, yref) <= TOL
    # constant input exercises the seed
    g2 = tg.Sos(co, gain, tg.C64 if cplx else tg.F32, r1, forme=1)
    ref2 = orc.SosChain(z, p, mn, md, forme=1)
    xc = np.full(3000, 2.0, np.complex64 if cplx else np.float32)
    assert relerr(g2.step(xc), ref2.step(xc)) <= TOL


# BASELINE configs[3] at full size: 6 sections on 2^26 float samples, whole-vector oracle
def test_cfg4_full_size(tg, orc):
    import torch
    n = 1 << 26
    ref, g = chains(orc, tg, 12, 0.25, False)
    gen = torch.Generator(device="cuda:0").manual_seed(4)
    xd = torch.randn(n, device="cuda:0", generator=gen)
    yd = g.step(xd)
    torch.cuda.synchronize()
    yref = ref.step(xd.cpu().numpy())
    y = yd.cpu().numpy()
    assert relerr(y, yref) <= TOL
    # linearity over the whole vector
    g.reset()
    y2 = g.step(xd * 0.5)
    torch.cuda.synchronize()
    assert float((y2 - 0.5 * yd).abs().max()) <= 1e-5 * float(yd.abs().max())


# Multi-GPU sharding rule of SURVEY 8e as bench.py --workload sos applies it: a shard that does
# not start the stream is warmed on the last `halo` samples of its left neighbour (output
# discarded); `halo` is the library's bound for ||Phi^halo|| <= 1e-9, so the shard's output
# equals the one-pass result.
@pytest.mark.parametrize("cplx", [False, True])
def test_sos_shard_warmup_halo(tg, orc, cplx):
    n, cut = 200000, 77777
    ref, g = chains(orc, tg, 12, 0.25, cplx)
    x = rand(n, cplx, 21)
    yref = ref.step(x)
    W = int(g.halo)
    assert 0 < W < cut
    g.step(x[cut - W:cut])                      # warm-up: state after the halo, output dropped
    y1 = g.step(x[cut:])
    assert relerr(y1, yref[cut:]) <= TOL


# device views that are not 16-B aligned (x[1:], y[3:] ...): bounced through aligned buffers,
# same results, and no fall-back to the sequential tail kernel
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("ox,oy", [(1, 0), (0, 3), (1, 1), (2, 3)])
def test_sos_unaligned_device_views(tg, orc, cplx, ox, oy):
    import time
    import torch
    dev = torch.device("cuda", 0)
    ref, g = chains(orc, tg, 12, 0.25, cplx)
    n = 1 << 22
    x = rand(n + 8, cplx, 5)
    xd = torch.from_numpy(x).to(dev)
    yd = torch.zeros(n + 8, dtype=xd.dtype, device=dev)
    g.step(xd[ox:ox + 1000], yd[oy:oy + 1000])             # first call: ragged and short
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g.step(xd[ox + 1000:ox + n], yd[oy + 1000:oy + n])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert relerr(yd[oy:oy + n].cpu().numpy(), ref.step(x[ox:ox + n])) <= TOL
    perf_guard(dt < 0.5, f"unaligned views took {dt:.2f} s")      # the sequential kernel would need seconds
    # in place on an unaligned view
    ref2, g2 = chains(orc, tg, 12, 0.25, cplx)
    z = xd.clone()
    g2.step(z[1:1 + n], z[1:1 + n])
    assert relerr(z[1:1 + n].cpu().numpy(), ref2.step(x[1:1 + n])) <= TOL


# The GPU data path tied to what the reference's test_riia holds (test-filtres.cc:668-679,327-404): the
# magnitude template of design_riia(12, "lp", "butt", 0.25) measured THROUGH tsdgpu_sos by steady-state
# sinusoids at the template's bin frequencies (same check on the oracle: tests/test_oracle_pins.py)
@pytest.mark.parametrize("forme", [2, 1])
def test_sos_riia_template_through_the_gpu_recursion(tg, orc, forme):
    from test_oracle_pins import (RIIA_TEMPLATE_BINS_PASS, RIIA_TEMPLATE_BINS_STOP, butter12_gain, riia_template_gain)
    z, p, mn, md = orc.design_butter_lp(12, 0.25)
    co, gain, r1 = orc.SosChain(z, p, mn, md, forme).coefs()
    for k in RIIA_TEMPLATE_BINS_PASS + RIIA_TEMPLATE_BINS_STOP:
        g = riia_template_gain(lambda x: tg.Sos(co, gain, tg.C64, r1, forme).step(x), k, n=1 << 17)
        if k < 800:
            assert abs(g - 1.0) <= 0.1, (k, g)
        else:
            assert g <= 0.1, (k, g)
        assert abs(g - butter12_gain(0.5 * k / 2048.0)) <= 2e-3, (k, g)


def test_sos_small_and_ragged_blocks_are_not_a_cliff(tg, orc):
    """Blocks shorter than a 2048-float sub-tile, and the ragged end of any call, used to walk the samples one by one from
    global memory (0.9 us per sample of this chain: 466 us for a 512-sample block, up to 1.8 ms added to a 2^26 + 2047
    call).  They run as narrow parallel steps plus a systolic pipeline now: parity on every residue class (odd orders and
    DF1 included), state carried from one ragged end into the next call, and a loose bound on the time so that the cliff
    cannot come back unnoticed."""
    import time
    import torch
    for cplx in (False, True):
        for order in (12, 5):
            for n in (1, 2, 63, 64, 127, 128, 255, 256, 257, 511, 512, 1000, 2047, 2048 + 255, 4096 + 1023):
                ref, g = chains(orc, tg, order, 0.25, cplx)
                x = rand(2 * n + 3, cplx, n + order)
                y = np.concatenate([g.step(x[:n].copy()), g.step(x[n:].copy())])
                assert relerr(y, ref.step(x)) <= TOL, (cplx, order, n)
    z, p, mn, md = orc.design_butter_lp(6, 0.2)
    ref = orc.SosChain(z, p, mn, md, forme=1)
    co, gain, r1 = ref.coefs()
    g = tg.Sos(co, gain, tg.F32, r1, forme=1)
    x = rand(3 * 777, False, 5)
    y = np.concatenate([g.step(x[o:o + 777].copy()) for o in range(0, len(x), 777)])
    assert relerr(y, ref.step(x)) <= TOL
    _, g = chains(orc, tg, 12, 0.25, False)
    for n in (512, 2047, (1 << 20) + 2047):
        xd = torch.randn(n, device="cuda")
        yd = torch.empty_like(xd)
        for _ in range(5):
            g.step(xd, yd)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            g.step(xd, yd)
        torch.cuda.synchronize()
        us = (time.perf_counter() - t0) / 20 * 1e6
        perf_guard(us < 400, f"a {n}-float step takes {us:.0f} us")


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("order,fc", [(1, 1e-5), (1, 1e-4), (2, 1e-4), (3, 1e-4), (2, 1e-3), (4, 1e-3), (12, 0.002)])
def test_sos_long_memory_exact_carry(tg, orc, cplx, order, fc):
    """A memory that is long against the call (DC blocker / smoother cut-offs: warm-ups of 10^5 samples and more) used to leave
    the block-parallel scheme a handful of chunks, down to ONE wave walking the vector (3 ms per 2^22 samples).  Such calls
    carry the state exactly from chunk to chunk (end states of a zero-state pass, scanned with the powers of the
    cascade's transition matrix, second pass from the true start states).  Against the oracle with the conditioning
    criterion of test_sos_slow_decay (the float64 run of the same recurrence arbitrates), in several ragged calls, and
    within 0.5 ms per 2^22 samples."""
    import time
    import torch
    ref, g = chains(orc, tg, order, fc, cplx)
    n = (1 << 20) + 777
    x = rand(n, cplx, 5) + np.float32(0.5)           # a DC offset: what such filters are for
    yref = ref.step(x)
    y64 = ref.run_f64(x.real) + 1j * ref.run_f64(x.imag) if cplx else ref.run_f64(x)     # (real coefficients: two channels)
    noise = relerr(yref, y64)
    y = g.step(x)
    print("long memory", order, fc, cplx, "halo", g.halo, "err", relerr(y, y64), "reference's own", noise)
    # (in the scans' (level, slope) coordinates the GPU result is closer to the float64 answer than the reference's own
    # float32 recurrence is -- 4e-6 against 6e-3 at order 2, fc = 1e-4)
    assert relerr(y, y64) <= max(TOL, noise), (relerr(y, y64), noise)
    # the same stream in ragged calls: the carried stream state enters chunk 0 of every call
    _, g2 = chains(orc, tg, order, fc, cplx)
    cuts = [0, 300001, 300001 + 2048 * 130, 900000, n]
    y2 = np.concatenate([g2.step(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    assert relerr(y2, y64) <= max(TOL, noise)
    # resident data, 2^22 samples: the rate of the ordinary kernel within a small factor
    _, g3 = chains(orc, tg, order, fc, cplx)
    xd = torch.randn((1 << 22) * (2 if cplx else 1), device="cuda")
    xd = torch.view_as_complex(xd.view(-1, 2)) if cplx else xd
    yd = torch.empty_like(xd)
    g3.step(xd, yd)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        g3.step(xd, yd)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / 5 * 1e3
    print("long memory", order, fc, cplx, "ms per 2^22 samples", round(ms, 3))
    perf_guard(ms < 0.5, ms)                         # (1.5 - 3.2 ms on the sequential chunk)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("order,fc", [(2, 1e-4), (3, 1e-4), (12, 0.002)])
def test_sos_long_memory_forme_directe_1(tg, orc, cplx, order, fc):
    """The exact carry with FormeDirecte1 sections: the carried state of a section then includes its last two inputs."""
    import time
    import torch
    z, p, mn, md = orc.design_butter_lp(order, fc)
    ref = orc.SosChain(z, p, mn, md, forme=1)
    co, gain, r1 = ref.coefs()
    g = tg.Sos(co, gain, tg.C64 if cplx else tg.F32, r1, forme=1)
    n = (1 << 20) + 333
    x = rand(n, cplx, 6) + np.float32(0.5)
    yref = ref.step(x)
    y = g.step(x)
    # the float64 run of the same chain arbitrates (FormeDirecte1 seeds all four memories of a section with its first input,
    # filtre-rt.cc:361-365; the trailing first-order section starts from zero and carries the gain, :407-437,567-570)
    import f64ref
    v = f64ref.sos(co, gain, r1, x, forme=1)
    noise = relerr(yref, v)
    print("long memory DF1", order, fc, cplx, "err", relerr(y, v), "reference's own", noise)
    assert relerr(y, v) <= max(2e-5, noise), (relerr(y, v), noise)
    g2 = tg.Sos(co, gain, tg.C64 if cplx else tg.F32, r1, forme=1)
    cuts = [0, 300001, 300001 + 2048 * 130, 900000, n]
    y2 = np.concatenate([g2.step(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    assert relerr(y2, v) <= max(2e-5, noise)
    xd = torch.randn((1 << 22) * (2 if cplx else 1), device="cuda")
    xd = torch.view_as_complex(xd.view(-1, 2)) if cplx else xd
    yd = torch.empty_like(xd)
    g.step(xd, yd)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        g.step(xd, yd)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / 5 * 1e3
    print("long memory DF1", order, fc, cplx, "ms per 2^22 samples", round(ms, 3))
    perf_guard(ms < 0.6, ms)


@pytest.mark.parametrize("cplx", [False, True])
def test_exponential_smoother_and_dc_blocker_long_memory(tg, orc, cplx):
    """filtre_lexp(gamma) and filtre_dc(fc) (filtre-rt.cc:764-781) with time constants of 10^5 samples -- THE long-memory
    filters of everyday use -- through tsdgpu_rii: y_n = y_{n-1} + g (x_n - y_{n-1}) and y_n = a ((x_n - x_{n-1}) + y_{n-1})."""
    import time
    import torch
    n = (1 << 21) + 5
    x = rand(n, cplx, 9) + np.float32(3.0)
    for nu, de in (([1e-5, 0.0], [1.0, -(1.0 - 1e-5)]), ([1.0 - 2e-5, -(1.0 - 2e-5)], [1.0, -(1.0 - 2e-5)])):
        dt = tg.C64 if cplx else tg.F32
        g = tg.Rii(np.array(nu, np.float32), np.array(de, np.float32), dt)
        y = g.step(x)
        from scipy.signal import lfilter
        ex = lfilter(np.array(nu, np.float32).astype(np.float64), np.array(de, np.float32).astype(np.float64), x.astype(np.complex128 if cplx else np.float64))
        # the reference's float32 recursion (real data: FiltreRII<float, float>; the complex one on the real coefficients)
        yr = (orc.RiiC if cplx else orc.Rii)(np.array(nu, np.float32), np.array(de, np.float32)).step(x)
        bruit = relerr(yr, ex)
        assert relerr(y, ex) <= max(2e-5, bruit), (nu, relerr(y, ex), bruit)
        xd = torch.from_numpy(x[:1 << 21].copy()).cuda()
        yd = torch.empty_like(xd)
        g.step(xd, yd)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            g.step(xd, yd)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / 5 * 1e3
        print("lexp / dc", nu, cplx, "path", g.path, "ms per 2^21 samples", round(ms, 3))
        perf_guard(ms < 0.5, ms)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("order,fc,forme", [(12, 0.25, 2), (3, 1e-3, 1), (1, 1e-5, 2)])
def test_sos_state_vector_and_propagation(tg, orc, cplx, order, fc, forme):
    """tsdgpu_sos_get_state / set_state / propagate_state: the stream cut in two; the second half filtered from zero
    memories plus the first half's state propagated over its length (in double, on the host) = the second half filtered
    from that state = the whole stream in one handle.  (What the exact sharding exchanges.)"""
    z, p, mn, md = orc.design_butter_lp(order, fc)
    co, gain, r1 = orc.SosChain(z, p, mn, md, forme=forme).coefs()
    dt = tg.C64 if cplx else tg.F32
    x = rand(100000, cplx, 21) + np.float32(0.3)
    whole = tg.Sos(co, gain, dt, r1, forme=forme).step(x)
    a = tg.Sos(co, gain, dt, r1, forme=forme)
    ya = a.step(x[:40000].copy())
    st = a.get_state()
    assert st[0] == 1.0 and st.size == tg.lib().tsdgpu_sos_state_floats()
    b = tg.Sos(co, gain, dt, r1, forme=forme)
    b.set_state(st)
    yb = b.step(x[40000:].copy())
    y = np.concatenate([ya, yb])
    assert relerr(y, whole) <= 1e-5                       # the state vector IS the stream state (tilings shift: rounding)
    # end state of the second half two ways: from the carried state, and zero-state run + propagation
    zero = np.zeros_like(st)
    zero[0] = 1.0
    c = tg.Sos(co, gain, dt, r1, forme=forme)
    c.set_state(zero)
    c.step(x[40000:].copy())
    via = c.propagate_state(60000, st, c.get_state())
    direct = b.get_state()
    # (records of four floats per (section, channel); a FormeDirecte2 section carries the first two only)
    # and real data uses the records of channel 0 only (record = (section * 2 + channel))
    garde = np.ones(st.size - 1, bool)
    if forme == 2:
        garde[2::4] = garde[3::4] = False
    if not cplx:
        garde[(np.arange(st.size - 1) // 4) % 2 == 1] = False
    scale = max(float(np.abs(direct[1:][garde]).max()), 1e-6)
    assert np.abs(via[1:] - direct[1:])[garde].max() <= 5e-5 * scale, np.abs(via[1:] - direct[1:])[garde].max() / scale
    assert np.array_equal(a.propagate_state(0, st), st)   # zero samples: the identity


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("n,skip", [(300000, 256), (300000, 0), (5000, 256), (1500, 256), (2048 * 3 + 77, 2048 + 512), (300, 300), (70000, 4444)])
def test_sos_step_skip_filters_everything_and_stores_from_skip_on(tg, orc, n, skip, cplx):
    """tsdgpu_sos_step_skip (the interior of a sharded chunk: warm-up and interior in one launch): bit for bit step(x) from sample
    `skip` on, nothing written before it, the stream state afterwards the same -- whole sub-tiles, ragged ends, calls shorter than
    a sub-tile, skips inside / across / at the end of a sub-tile."""
    import torch
    z, p, mn, md = orc.design_butter_lp(6, 0.2)
    co, gain, r1 = orc.SosChain(z, p, mn, md).coefs()
    dt = tg.C64 if cplx else tg.F32
    x = rand(n + 1000, cplx, n + skip)
    xd = torch.from_numpy(x).cuda()
    a, b = tg.Sos(co, gain, dt, r1), tg.Sos(co, gain, dt, r1)
    ya = torch.full((n,), 7.0, dtype=xd.dtype, device="cuda")
    a.step_skip(xd[:n], ya, skip)
    yb = b.step(xd[:n])
    torch.cuda.synchronize()
    assert torch.equal(ya[skip:], yb[skip:])
    assert bool((ya[:skip] == 7.0).all())
    assert torch.equal(a.step(xd[n:]), b.step(xd[n:]))          # same stream state
    if cplx is False:
        with pytest.raises(tg.TsdGpuError):
            a.step_skip(xd[:n], ya, 3)                           # 3 floats: not a multiple of 4
