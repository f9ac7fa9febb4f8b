"""Oversampled polyphase synthesizer (include/tsdgpu.h: tsdgpu_synthesizer_create_oversampled; hop D = M / OS, OS in {2, 4})
against the float64 references of tests/syn_os_ref.py: parity over every radix split of the transform and the tap counts around
the hop and the frame length, many tiles and workgroups, chunk invariance and state + phase bit for bit, OS = 1 against the plain
bank, layouts, the argument checks, the non-finite horizon, the round trip through the oversampled channelizer on the device, and
the chain channelizer -> bank -> synthesizer.

Inputs and prototype: syn_ref.rows / chan_ref.prototype.  Bar: max |x - ref| <= 1e-5 max |ref| over the whole step (the samples
of a hop share a transform)."""
import ctypes

import numpy as np
import pytest

import chan_os_ref
import chan_ref
import syn_os_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-5
MS = (8, 16, 32, 64, 128, 256, 512, 1024)
OSS = (2, 4)


@pytest.fixture(scope="module")
def tg():
    import libtsd_amd as t
    assert t.device_count() >= 1
    return t


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(y):
    import torch
    torch.cuda.synchronize()
    return y.cpu().numpy()


def run(sy, ud, frames):
    """the rows through the handle in steps of the given frame counts (strided column blocks of ud); the stream (host)"""
    import torch
    outs, a = [], 0
    for f in frames:
        outs.append(sy.step(ud[:, a:a + f]))
        a += f
    return host(torch.cat(outs))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ 1. parity
# every M with K = 16 D and K = M + 1 at every F; the other tap counts at F = 2 and 17 (17 straddles a 16-frame unit, and is odd:
# the second step starts from a non-zero phase)
def _parity_cases():
    out = []
    for OS in OSS:
        for M in MS:
            D = M // OS
            for K in sorted({1, D, D + 1, M + 1, 16 * D}):
                if K > 16 * D:
                    continue
                for F in (1, 2, 17, 100):
                    if K in (16 * D, M + 1) or F in (2, 17):
                        out.append((M, OS, K, F))
    return out


@pytest.mark.parametrize("M,OS,K,F", _parity_cases())
def test_parity_two_steps(tg, M, OS, K, F):
    D = M // OS
    f = R.prototype(M, K)
    u = R.rows(M, 2 * F, seed=M + K + F + OS)
    ref = R.synth64(u, f, M, OS)
    sy = tg.Synthesizer(f, M, oversample=OS)
    assert sy.hop == D and sy.out_count(F) == F * D
    x = run(sy, dev(u), [F, F])                  # the second step starts from real history and, for odd F, a non-zero phase
    assert x.shape == (2 * F * D,)
    assert sy.phase == (2 * F) % OS
    err = R.rel_err(x, ref)
    print(f"M={M} OS={OS} K={K} F={F}: {err:.2e}")
    assert err <= TOL


def test_small_case_against_the_definition(tg):
    M, OS, K, F = 16, 2, 45, 12
    f = R.prototype(M, K)
    u = R.rows(M, F, seed=3)
    x = run(tg.Synthesizer(f, M, oversample=OS), dev(u), [F])
    assert R.rel_err(x, R.definition(u, f, M, OS)) <= TOL


@pytest.mark.parametrize("M,OS,F", [(8, 4, 40000), (1024, 2, 600)])
def test_many_tiles_and_workgroups(tg, M, OS, F):
    K = 8 * (M // OS)
    f = R.prototype(M, K)
    u = R.rows(M, F, seed=11)
    x = run(tg.Synthesizer(f, M, oversample=OS), dev(u), [F])
    err = R.rel_err(x, R.synth64(u, f, M, OS))
    print(f"M={M} OS={OS} F={F}: {err:.2e}")
    assert err <= TOL


# ----------------------------------------------------------------------------------- 2. chunk invariance and state, bit for bit
@pytest.mark.parametrize("OS", OSS)
@pytest.mark.parametrize("M", [8, 64, 1024])
@pytest.mark.parametrize("kk", ["M+1", "16D"])
def test_chunk_invariance_bit_for_bit(tg, M, OS, kk):
    K = M + 1 if kk == "M+1" else 16 * (M // OS)
    f = R.prototype(M, K)
    ud = dev(R.rows(M, 150, seed=5))
    one = run(tg.Synthesizer(f, M, oversample=OS), ud, [150])
    many = run(tg.Synthesizer(f, M, oversample=OS), ud, [1, 15, 16, 17, 101])
    assert np.array_equal(bits(one), bits(many))


@pytest.mark.parametrize("M,OS,K", [(8, 4, 16 * 2), (64, 2, 4 * 64 - 3), (1024, 2, 1025), (64, 4, 65)])
def test_state_and_phase_move_to_a_fresh_handle(tg, M, OS, K):
    import torch
    D = M // OS
    f = R.prototype(M, K)
    QW = -(-K // D) - 1
    u = R.rows(M, 60, seed=6)
    ud = dev(u)
    a = tg.Synthesizer(f, M, oversample=OS)
    assert a.history_len == QW * M and a.frames_kept == QW and a.phase == 0
    a.step(ud[:, :23])                                                   # 23 frames: odd
    assert a.phase == 23 % OS
    st = a.get_state()
    assert st.shape == (M, QW)
    assert np.array_equal(bits(st), bits(np.concatenate([np.zeros((M, QW), np.complex64), u[:, :23]], axis=1)[:, -QW:]))
    b, nophase = tg.Synthesizer(f, M, oversample=OS), tg.Synthesizer(f, M, oversample=OS)
    b.set_state(st)
    b.phase = 23                                                         # any hop count: taken modulo OS
    assert b.phase == 23 % OS
    nophase.set_state(st)
    xa, xb, xn = host(a.step(ud[:, 23:])), host(b.step(ud[:, 23:])), host(nophase.step(ud[:, 23:]))
    assert np.array_equal(bits(xa), bits(xb))
    assert not np.array_equal(bits(xa), bits(xn))                        # the history alone does not continue the stream
    with pytest.raises(tg.TsdGpuError, match="status 1"):
        b.phase = -1
    # a device-side state, and reset = a new handle
    sd = torch.empty((M, QW), dtype=torch.complex64, device="cuda")
    a.get_state(sd)
    c = tg.Synthesizer(f, M, oversample=OS)
    c.set_state(sd)
    c.phase = a.phase
    a.step(ud[:, :1])                                                    # leave a on a non-zero phase before the reset
    a.reset()
    assert a.phase == 0
    fresh = host(tg.Synthesizer(f, M, oversample=OS).step(ud[:, :17]))
    assert np.array_equal(bits(host(a.step(ud[:, :17]))), bits(fresh))
    xc, xb2 = host(c.step(ud[:, :17])), host(b.step(ud[:, :17]))
    assert np.array_equal(bits(xc), bits(xb2))


@pytest.mark.parametrize("M,K", [(8, 5 * 8), (16, 33), (32, 3 * 32), (64, 65), (128, 2 * 128), (1024, 1025)])
def test_oversample_one_is_the_plain_bank(tg, M, K):
    """one shape per radix split (dft8; first radix 16, 2, 4, 8; M = 1024's two positions per thread)"""
    import torch
    f = R.prototype(M, K)
    ud = dev(R.rows(M, 37, seed=7))
    a, b = tg.Synthesizer(f, M), tg.Synthesizer(f, M, oversample=1)
    assert b.hop == M and b.history_len == a.history_len and b.phase == 0
    xa, xb = run(a, ud, [20, 17]), run(b, ud, [20, 17])
    assert np.array_equal(bits(xa), bits(xb))
    assert b.phase == 0
    # the Python layer creates OS = 1 through tsdgpu_synthesizer_create: the new entry point itself, through the C ABI
    L, raw, got = tg.lib(), ctypes.c_void_p(), ctypes.c_int64(-1)
    assert L.tsdgpu_synthesizer_create_oversampled(ctypes.byref(raw), M, 1, f.ctypes.data, len(f)) == 0
    try:
        assert L.tsdgpu_synthesizer_hop(raw) == M and L.tsdgpu_synthesizer_history_len(raw) == a.history_len
        assert L.tsdgpu_synthesizer_out_count(raw, 20) == 20 * M
        xr = torch.empty(37 * M, dtype=torch.complex64, device="cuda")
        for f0, nf in ((0, 20), (20, 17)):
            assert L.tsdgpu_synthesizer_step(raw, ud[:, f0:].data_ptr(), 37, nf, xr[f0 * M:].data_ptr(), nf * M, ctypes.byref(got), None) == 0
            assert got.value == nf * M and L.tsdgpu_synthesizer_get_phase(raw) == 0
        assert np.array_equal(bits(host(xr)), bits(xa))
    finally:
        L.tsdgpu_synthesizer_destroy(raw)


# -------------------------------------------------------------------------------------------------------------- 3. layouts
@pytest.mark.parametrize("M,OS,K", [(16, 4, 4 * 16 - 3), (256, 2, 257)])
def test_layouts_give_the_same_bits(tg, M, OS, K):
    import torch
    F, D = 21, M // OS                                                   # odd: the second step starts on a non-zero phase
    n = F * D
    f = R.prototype(M, K)
    u = R.rows(M, 2 * F, seed=8)
    ud = dev(u)

    def two_steps(step):
        sy = tg.Synthesizer(f, M, oversample=OS)
        return [step(sy, 0), step(sy, 1)]

    def packed(i):
        return ud[:, i * F:(i + 1) * F].contiguous()

    base = two_steps(lambda sy, i: host(sy.step(ud[:, i * F:(i + 1) * F])).copy())      # ldu = 2 F: even
    assert R.rel_err(np.concatenate(base), R.synth64(u, f, M, OS)) <= TOL

    def strided(ld):
        def step(sy, i):
            buf = torch.zeros((M, ld), dtype=torch.complex64, device="cuda")
            buf[:, :F] = packed(i)
            out = torch.full((n + 8,), 7.0, dtype=torch.complex64, device="cuda")
            x = sy.step(buf[:, :F], out)
            assert x.data_ptr() == out.data_ptr() and tuple(x.shape) == (n,)
            assert bool((out[n:] == 7.0).all())                      # nothing written past F D
            return host(x).copy()
        return step

    def from_host(sy, i):
        x = sy.step(np.ascontiguousarray(u[:, i * F:(i + 1) * F]))
        assert isinstance(x, np.ndarray) and x.shape == (n,)
        return x

    def host_strided(sy, i):
        return sy.step(u[:, i * F:(i + 1) * F]).copy()

    def misaligned_rows(sy, i):
        buf = torch.zeros(M * (F + 1) + 1, dtype=torch.complex64, device="cuda")
        rows = buf[1:].view(M, F + 1)[:, :F]                             # ldu = F + 1 even, the base 8 B off
        rows.copy_(packed(i))
        assert rows.data_ptr() % 16 == 8
        return host(sy.step(rows)).copy()

    def misaligned_x(sy, i):
        out = torch.full((n + 9,), 7.0, dtype=torch.complex64, device="cuda")
        assert out[1:].data_ptr() % 16 == 8
        x = sy.step(packed(i), out[1:])
        assert bool((out[n + 1:] == 7.0).all()) and bool(out[0] == 7.0)
        return host(x).copy()

    for name, step in (("ldu odd", strided(F + 2)), ("ldu even", strided(F + 3)), ("ldu = F", strided(F)), ("host", from_host),
                       ("host strided", host_strided), ("rows 8-B aligned", misaligned_rows), ("x 8-B aligned", misaligned_x)):
        got = two_steps(step)
        for g, b in zip(got, base):
            assert np.array_equal(bits(g), bits(b)), name


# --------------------------------------------------------------------------------------------------------------- 4. errors
def test_step_errors_leave_history_and_phase_untouched(tg):
    import torch
    M, OS, K, F = 64, 2, 4 * 64 - 3, 11                                 # F odd: the failing steps meet a non-zero phase
    D = M // OS
    n = F * D
    f = R.prototype(M, K)
    ud = dev(R.rows(M, 3 * F, seed=9))
    a, b = tg.Synthesizer(f, M, oversample=OS), tg.Synthesizer(f, M, oversample=OS)
    a.step(ud[:, :F])
    b.step(ud[:, :F])
    seg = ud[:, F:2 * F].contiguous()
    with pytest.raises(tg.TsdGpuError, match="status 1"):              # x_capacity below F D
        a.step(seg, torch.empty(n - 1, dtype=torch.complex64, device="cuda"))
    big = torch.zeros(2 * F * M, dtype=torch.complex64, device="cuda")
    big[:F * M] = seg.reshape(-1)
    with pytest.raises(tg.TsdGpuError, match="status 1"):              # u and x share addresses: x's footprint is F D samples
        a.step(big[:F * M].view(M, F), big[F * M - 1:F * M - 1 + n])
    a.step(big[:F * M].view(M, F), big[F * M:F * M + n])               # next to each other is fine (and keeps the twins in step)
    b.step(seg)
    with pytest.raises(tg.TsdGpuError, match="row stride"):            # ldu below a channel's inputs: the Python layer's check
        a.step(torch.as_strided(big, (M, F), (F - 1, 1)))
    xbuf, got = torch.empty(n, dtype=torch.complex64, device="cuda"), ctypes.c_int64(-1)
    rc = tg.lib().tsdgpu_synthesizer_step(a._h, seg.data_ptr(), F - 1, F, xbuf.data_ptr(), n, ctypes.byref(got), None)
    assert rc == 1 and got.value == 0 and "ldu" in tg.lib().tsdgpu_last_error().decode()     # the C ABI's check
    rc = tg.lib().tsdgpu_synthesizer_step(a._h, seg.data_ptr(), F, F, xbuf.data_ptr(), n - 1, ctypes.byref(got), None)
    assert rc == 1 and got.value == 0 and "x_capacity" in tg.lib().tsdgpu_last_error().decode()
    assert a.step(ud[:, :0]).shape == (0,)                              # frames = 0: a no-op
    assert a.phase == b.phase == (2 * F) % OS
    a.step(ud[:, :1])                                                   # onto a non-zero phase, then the errors once more
    b.step(ud[:, :1])
    with pytest.raises(tg.TsdGpuError, match="status 1"):
        a.step(seg, torch.empty(n - 1, dtype=torch.complex64, device="cuda"))
    assert a.step(ud[:, :0]).shape == (0,)
    assert a.phase == b.phase == 1
    last = ud[:, 2 * F:].contiguous()
    xa, xb = host(a.step(last)), host(b.step(last))
    assert np.array_equal(bits(xa), bits(xb))
    assert a.phase == b.phase == (1 + F) % OS


def test_create_errors(tg):
    def fails(channels, OS, K, status, *words):
        with pytest.raises(tg.TsdGpuError, match=f"status {status}"):
            tg.Synthesizer(np.ones(K, np.float32), channels, oversample=OS)
        msg = tg.lib().tsdgpu_last_error().decode()
        for w in words:
            assert w in msg, msg
    fails(64, 3, 64, 3, "oversample")          # UNSUPPORTED, with the limit
    fails(64, 8, 64, 3, "oversample")
    fails(64, 0, 64, 1)                        # INVALID
    fails(64, -2, 64, 1)
    fails(64, 2, 16 * 32 + 1, 3, "16")
    fails(64, 4, 16 * 16 + 1, 3, "16")
    fails(12, 2, 24, 3, "8", "1024")
    tg.Synthesizer(np.ones(16 * 32, np.float32), 64, oversample=2).close()
    tg.Synthesizer(np.ones(16 * 16, np.float32), 64, oversample=4).close()


# ---------------------------------------------------------------------------------------------------- 5. non-finite horizon
@pytest.mark.parametrize("what", [np.nan, np.inf])
@pytest.mark.parametrize("c", [1, 40])
def test_non_finite_horizon(tg, what, c):
    M, OS, F = 64, 2, 40
    D = M // OS
    K = 4 * M - 3                                                       # Q = 8: the last row has zero-padded taps
    Q = -(-K // D)
    f = R.prototype(M, K)
    u = R.rows(M, F, seed=10)
    clean = run(tg.Synthesizer(f, M, oversample=OS), dev(u), [F]).reshape(F, D)
    ub = u.copy()
    ub[c, 9] = what
    x = run(tg.Synthesizer(f, M, oversample=OS), dev(ub), [F]).reshape(F, D)
    bad = x[9:9 + Q]                                                    # every sample of hops 9 .. 9 + Q - 1
    assert not (np.isfinite(bad.real) & np.isfinite(bad.imag)).any()
    keep = np.r_[0:9, 9 + Q:F]
    assert np.array_equal(bits(x[keep]), bits(clean[keep]))


# ------------------------------------------------------------------------------------------- 6. round trip on the device
def _sine_window(M):
    h = np.sin(np.pi * (np.arange(M) + 0.5) / M).astype(np.float32)
    return h, np.ascontiguousarray(h[::-1])


@pytest.mark.parametrize("OS", OSS)
@pytest.mark.parametrize("M", [16, 256])
def test_round_trip_on_the_device(tg, M, OS):
    """Channelizer(h, M, OS) -> its rows delayed by one frame -> Synthesizer(f, M, OS), h the sine window of length M and f = h
    reversed: x comes back as (M OS / 2) x[p - M] (tests/test_synthesizer_os_cpu.py has the float64 pair at 5e-8).
    (a) the synthesizer against synth64 of the same device rows at the file's bar; (b) the round trip at 2e-5 of the peak, the two
    stages' bars added."""
    import torch
    F, D = 200, M // OS
    h, f = _sine_window(M)
    rng = np.random.default_rng(100 + M + OS)
    x = ((rng.standard_normal(F * D) + 1j * rng.standard_normal(F * D)) / np.sqrt(2)).astype(np.complex64)     # unit variance
    buf = torch.zeros((M, F + 1), dtype=torch.complex64, device="cuda")
    yd = tg.Channelizer(h, M, oversample=OS).step(dev(x), buf[:, 1:])   # columns 1 ..: column 0 stays zero
    assert yd.data_ptr() == buf[:, 1:].data_ptr() and tuple(yd.shape) == (M, F)
    out = tg.Synthesizer(f, M, oversample=OS).step(buf[:, :F])
    assert out.is_cuda and tuple(out.shape) == (F * D,)
    got = host(out)
    ea = R.rel_err(got, R.synth64(host(buf[:, :F]), f, M, OS))
    want = (M * OS / 2) * np.concatenate([np.zeros(M, np.complex128), x.astype(np.complex128)])[:F * D]
    eb = np.abs(got - want)[2 * M:].max() / np.abs(want).max()
    print(f"M={M} OS={OS}: against synth64 of the device rows {ea:.2e}; round trip {eb:.2e} of the peak")
    assert ea <= TOL
    assert eb <= 2e-5


# ------------------------------------------------------------------------------ 7. channelizer -> bank -> synthesizer on device
def test_banks_in_between(tg):
    import torch
    M, OS, F = 64, 2, 200
    D = M // OS
    K = 8 * D
    h = R.prototype(M, K)
    x = chan_ref.stream(F * D, M, seed=12)
    rng = np.random.default_rng(13)
    h2 = (rng.standard_normal(31) / 8).astype(np.float32)
    ybuf = torch.empty((M, F), dtype=torch.complex64, device="cuda")
    zbuf = torch.empty((M, F), dtype=torch.complex64, device="cuda")
    yd = tg.Channelizer(h, M, oversample=OS).step(dev(x), ybuf)
    assert yd.data_ptr() == ybuf.data_ptr() and tuple(yd.shape) == (M, F)          # a view of the caller's block: no copy
    zd = tg.FirBank(h2, tg.C64, M).step(yd, zbuf)
    assert zd.data_ptr() == zbuf.data_ptr() and tuple(zd.shape) == (M, F)
    out = tg.Synthesizer(h, M, oversample=OS).step(zd)
    assert out.is_cuda and tuple(out.shape) == (F * D,)
    y64 = chan_os_ref.polyphase64(x, h, M, OS)
    z64 = np.stack([np.convolve(r, h2.astype(np.float64))[:F] for r in y64])
    ref = R.synth64(z64, h, M, OS)
    err = R.rel_err(host(out), ref)
    print(f"channelizer -> FirBank -> synthesizer against the float64 composition: {err:.2e}")
    assert err <= TOL
