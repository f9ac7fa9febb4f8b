"""Oversampled polyphase channelizer (include/tsdgpu.h: tsdgpu_channelizer_create_oversampled; hop D = M / OS, OS in {2, 4})
against the float64 references of tests/chan_os_ref.py: parity over every radix split of the transform and the tap counts around
the hop and the branch length, many tiles and workgroups, chunk invariance and state + phase bit for bit, OS = 1 against the plain
bank, layouts, the argument checks, the non-finite horizon, and its (M, F) output handed to the channel banks without a copy.

Inputs and prototype: chan_ref.stream / chan_ref.prototype.  Bar: max |y - ref| <= 1e-5 max |ref| over the whole step (the
channels share a transform)."""
import ctypes

import numpy as np
import pytest

import chan_os_ref as O
import chan_ref as R

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


def run(ch, xd, hops):
    """the stream through the handle in steps of the given hop counts; the (M, sum(hops)) outputs side by side (host)"""
    import torch
    D = ch.hop
    outs, a = [], 0
    for f in hops:
        outs.append(ch.step(xd[a * D:(a + f) * D]))
        a += f
    return host(torch.cat(outs, dim=1))


def bits(y):
    return np.ascontiguousarray(y).view(np.uint32)


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
    h = R.prototype(M, K)
    x = R.stream(2 * F * D, M, seed=M + K + F + OS)
    ref = O.polyphase64(x, h, M, OS)
    ch = tg.Channelizer(h, M, oversample=OS)
    assert ch.hop == D and ch.out_count(F * D) == F
    y = run(ch, dev(x), [F, F])                  # the second step starts from real history and, for odd F, a non-zero phase
    assert y.shape == (M, 2 * F)
    assert ch.phase == (2 * F) % OS
    err = R.rel_err(y, ref)
    print(f"M={M} OS={OS} K={K} F={F}: {err:.2e}")
    assert err <= TOL


def test_small_case_against_the_definition(tg):
    M, OS, K, F = 16, 2, 45, 12
    h = R.prototype(M, K)
    x = R.stream(F * (M // OS), M, seed=3)
    y = run(tg.Channelizer(h, M, oversample=OS), dev(x), [F])
    assert R.rel_err(y, O.definition(x, h, M, OS)) <= TOL


@pytest.mark.parametrize("M,OS,F", [(8, 4, 40000), (1024, 2, 600)])
def test_many_tiles_and_workgroups(tg, M, OS, F):
    D = M // OS
    K = 8 * D
    h = R.prototype(M, K)
    x = R.stream(F * D, M, seed=11)
    y = run(tg.Channelizer(h, M, oversample=OS), dev(x), [F])
    err = R.rel_err(y, O.polyphase64(x, h, M, OS))
    print(f"M={M} OS={OS} F={F}: {err:.2e}")
    assert err <= TOL


# ----------------------------------------------------------------------------------- 2. chunk invariance and state, bit for bit
@pytest.mark.parametrize("OS", OSS)
@pytest.mark.parametrize("M", [8, 64, 1024])
@pytest.mark.parametrize("kk", ["M+1", "16D"])
def test_chunk_invariance_bit_for_bit(tg, M, OS, kk):
    D = M // OS
    K = M + 1 if kk == "M+1" else 16 * D
    h = R.prototype(M, K)
    xd = dev(R.stream(150 * D, M, seed=5))
    one = run(tg.Channelizer(h, M, oversample=OS), xd, [150])
    many = run(tg.Channelizer(h, M, oversample=OS), xd, [1, 15, 16, 17, 101])
    assert np.array_equal(bits(one), bits(many))


@pytest.mark.parametrize("M,OS,K", [(8, 4, 16 * 2), (64, 2, 4 * 64 - 3), (1024, 2, 1025), (64, 4, 65)])
def test_state_and_phase_move_to_a_fresh_handle(tg, M, OS, K):
    import torch
    D = M // OS
    h = R.prototype(M, K)
    P = -(-K // M)
    H = P * M - D
    xd = dev(R.stream(60 * D, M, seed=6))
    a = tg.Channelizer(h, M, oversample=OS)
    assert a.history_len == H and a.phase == 0
    a.step(xd[:23 * D])                                                  # 23 hops: odd
    assert a.phase == 23 % OS
    st = a.get_state()
    assert st.shape == (H,)
    assert np.array_equal(st, np.concatenate([np.zeros(H, np.complex64), host(xd)[:23 * D]])[-H:])    # the last inputs, oldest first
    b, nophase = tg.Channelizer(h, M, oversample=OS), tg.Channelizer(h, M, oversample=OS)
    b.set_state(st)
    b.phase = 23                                                         # any hop count: taken modulo OS
    assert b.phase == 23 % OS
    nophase.set_state(st)
    ya, yb, yn = host(a.step(xd[23 * D:])), host(b.step(xd[23 * D:])), host(nophase.step(xd[23 * D:]))
    assert np.array_equal(bits(ya), bits(yb))
    assert not np.array_equal(bits(ya), bits(yn))                        # the history alone does not continue the stream
    with pytest.raises(tg.TsdGpuError, match="status 1"):
        b.phase = -1
    # a device-side state, and reset = a new handle
    sd = torch.empty(H, dtype=torch.complex64, device="cuda")
    a.get_state(sd)
    c = tg.Channelizer(h, M, oversample=OS)
    c.set_state(sd)
    c.phase = a.phase
    a.step(xd[:D])                                                       # leave a on a non-zero phase before the reset
    a.reset()
    assert a.phase == 0
    fresh = host(tg.Channelizer(h, M, oversample=OS).step(xd[:17 * D]))
    assert np.array_equal(bits(host(a.step(xd[:17 * D]))), bits(fresh))
    yc, yb2 = host(c.step(xd[:17 * D])), host(b.step(xd[:17 * D]))
    assert np.array_equal(bits(yc), bits(yb2))


@pytest.mark.parametrize("M,K", [(8, 5 * 8), (16, 33), (32, 3 * 32), (64, 65), (128, 2 * 128), (1024, 1025)])
def test_oversample_one_is_the_plain_bank(tg, M, K):
    """one shape per radix split (dft8; first radix 16, 2, 4, 8; M = 1024's two positions per thread)"""
    h = R.prototype(M, K)
    xd = dev(R.stream(37 * M, M, seed=7))
    import torch
    a, b = tg.Channelizer(h, M), tg.Channelizer(h, M, oversample=1)
    assert b.hop == M and b.history_len == a.history_len and b.phase == 0
    ya, yb = run(a, xd, [20, 17]), run(b, xd, [20, 17])
    assert np.array_equal(bits(ya), bits(yb))
    assert b.phase == 0
    # the Python layer creates OS = 1 through tsdgpu_channelizer_create: the new entry point itself, through the C ABI
    L, raw, got = tg.lib(), ctypes.c_void_p(), ctypes.c_int64(-1)
    assert L.tsdgpu_channelizer_create_oversampled(ctypes.byref(raw), M, 1, h.ctypes.data, len(h)) == 0
    try:
        assert L.tsdgpu_channelizer_hop(raw) == M and L.tsdgpu_channelizer_history_len(raw) == a.history_len
        yr = torch.empty((M, 37), dtype=torch.complex64, device="cuda")
        for f0, f in ((0, 20), (20, 17)):
            assert L.tsdgpu_channelizer_step(raw, xd[f0 * M:].data_ptr(), f * M, yr[:, f0:].data_ptr(), 37, f, ctypes.byref(got), None) == 0
            assert got.value == f and L.tsdgpu_channelizer_get_phase(raw) == 0
        assert np.array_equal(bits(host(yr)), bits(ya))
    finally:
        L.tsdgpu_channelizer_destroy(raw)


# -------------------------------------------------------------------------------------------------------------- 3. layouts
@pytest.mark.parametrize("M,OS,K", [(16, 4, 4 * 16 - 3), (256, 2, 257)])
def test_layouts_give_the_same_bits(tg, M, OS, K):
    import torch
    F, D = 21, M // OS                                                   # odd: the second step starts on a non-zero phase
    n = F * D
    h = R.prototype(M, K)
    x = R.stream(2 * n, M, seed=8)
    xd = dev(x)

    def two_steps(step):
        ch = tg.Channelizer(h, M, oversample=OS)
        return [step(ch, 0), step(ch, 1)]

    base = two_steps(lambda ch, i: host(ch.step(xd[i * n:(i + 1) * n])).copy())
    assert R.rel_err(np.concatenate(base, axis=1), O.polyphase64(x, h, M, OS)) <= TOL

    def strided(ld):
        def step(ch, i):
            buf = torch.full((M, ld), 7.0, dtype=torch.complex64, device="cuda")
            y = ch.step(xd[i * n:(i + 1) * n], buf[:, :F])
            assert y.data_ptr() == buf.data_ptr() and tuple(y.shape) == (M, F)
            assert ld == F or bool((buf[:, F:] == 7.0).all())       # nothing written past a row
            return host(y).copy()
        return step

    def from_host(ch, i):
        y = ch.step(x[i * n:(i + 1) * n])
        assert isinstance(y, np.ndarray)
        return y

    def host_strided(ch, i):
        buf = np.full((M, F + 5), 7.0, np.complex64)
        y = ch.step(x[i * n:(i + 1) * n], buf[:, :F]).copy()
        assert (buf[:, F:] == 7.0).all()
        return y

    def misaligned(ch, i):
        xb = torch.empty(n + 1, dtype=torch.complex64, device="cuda")
        xb[1:] = xd[i * n:(i + 1) * n]
        assert xb[1:].data_ptr() % 16 == 8
        return host(ch.step(xb[1:])).copy()

    for name, step in (("ldy odd", strided(F + 4)), ("ldy even", strided(F + 3)), ("ldy = F", strided(F)), ("host", from_host),
                       ("host strided", host_strided), ("x 8-B aligned", misaligned)):
        got = two_steps(step)
        for g, b in zip(got, base):
            assert np.array_equal(bits(g), bits(b)), name


# --------------------------------------------------------------------------------------------------------------- 4. errors
def test_step_errors_leave_history_and_phase_untouched(tg):
    import torch
    M, OS, K, F = 64, 2, 4 * 64 - 3, 11                                 # F odd: the failing steps meet a non-zero phase
    D = M // OS
    n = F * D
    h = R.prototype(M, K)
    xd = dev(R.stream(3 * n, M, seed=9))
    a, b = tg.Channelizer(h, M, oversample=OS), tg.Channelizer(h, M, oversample=OS)
    a.step(xd[:n])
    b.step(xd[:n])
    seg = xd[n:2 * n]
    with pytest.raises(tg.TsdGpuError, match="status 1"):              # not whole hops
        a.step(xd[n:2 * n - 1])
    with pytest.raises(tg.TsdGpuError, match="status 1"):              # a whole number of frames' worth is not asked for: M / 2 is a hop
        a.step(xd[n:n + D + 1])
    with pytest.raises(tg.TsdGpuError, match="status 1"):              # y_capacity too small
        a.step(seg, torch.empty((M, F - 1), dtype=torch.complex64, device="cuda"))
    big = torch.zeros(2 * F * M, dtype=torch.complex64, device="cuda")
    big[:n] = seg
    with pytest.raises(tg.TsdGpuError, match="status 1"):              # x and y share addresses: y's footprint is M rows of F = n / D
        a.step(big[:n], big[n - 1:n - 1 + F * M].view(M, F))
    with pytest.raises(tg.TsdGpuError, match="row stride"):            # ldy below a channel's outputs: the Python layer's check
        a.step(seg, torch.as_strided(big, (M, F), (F - 1, 1), n))
    ybuf, got = torch.empty((M, F), dtype=torch.complex64, device="cuda"), ctypes.c_int64(-1)
    rc = tg.lib().tsdgpu_channelizer_step(a._h, seg.data_ptr(), n, ybuf.data_ptr(), F - 1, F, ctypes.byref(got), None)
    assert rc == 1 and got.value == 0 and "ldy" in tg.lib().tsdgpu_last_error().decode()     # the C ABI's check
    assert a.step(xd[:0]).shape == (M, 0)                               # n = 0: a no-op
    assert a.phase == b.phase == F % OS
    ya, yb = host(a.step(seg)), host(b.step(seg))
    assert np.array_equal(bits(ya), bits(yb))
    assert a.phase == b.phase == 0


def test_create_errors(tg):
    def fails(channels, OS, K, status, *words):
        with pytest.raises(tg.TsdGpuError, match=f"status {status}"):
            tg.Channelizer(np.ones(K, np.float32), channels, oversample=OS)
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
    tg.Channelizer(np.ones(16 * 32, np.float32), 64, oversample=2).close()
    tg.Channelizer(np.ones(16 * 16, np.float32), 64, oversample=4).close()


# ---------------------------------------------------------------------------------------------------- 5. non-finite horizon
@pytest.mark.parametrize("what", [np.nan, np.inf])
@pytest.mark.parametrize("s", [1, 20])                                  # s = 1 meets a zero-padded tap of the last branch
def test_non_finite_horizon(tg, what, s):
    M, OS, F = 64, 2, 40
    D = M // OS
    K = 4 * M - 3                                                       # P = 4
    P = 4
    h = R.prototype(M, K)
    x = R.stream(F * D, M, seed=10)
    clean = run(tg.Channelizer(h, M, oversample=OS), dev(x), [F])
    q = 9 * D + s
    xb = x.copy()
    xb[q] = what
    y = run(tg.Channelizer(h, M, oversample=OS), dev(xb), [F])
    lo, hi = q // D, (q + P * M) // D                                   # P OS frames
    assert hi - lo == P * OS
    assert not np.isfinite(y[:, lo:hi]).any()                           # every channel of those frames
    keep = np.r_[0:lo, hi:F]
    yb, cb = bits(y).reshape(M, F, 2), bits(clean).reshape(M, F, 2)
    assert np.array_equal(yb[:, keep], cb[:, keep])


# -------------------------------------------------------------------------------------------- 6. feeds a bank without a copy
def _rows_within_the_bar(z, ref, name):
    """every row within the file's bar: 1e-5 of the peak of the step.  The rows of a channelizer share a transform, so a weak row
    carries the strong one's rounding (tsdgpu.h: the channelizer's error bound) and a bank only passes that on: the bar is not
    1e-5 of a weak row's own peak (printed: with the 1e3 tone of chan_ref.stream next door, the weakest rows sit at that figure)."""
    peak = np.abs(ref).max()
    err = np.abs(np.asarray(z, np.complex128) - ref).max(axis=1)
    own = (err / np.abs(ref).max(axis=1)).max()
    print(f"{name}: worst row {err.max() / peak:.2e} of the step's peak; {own:.2e} of its own peak")
    assert z.shape == ref.shape
    for c in range(len(ref)):
        assert err[c] <= TOL * peak, (name, c)


def test_output_feeds_the_banks(tg):
    M, OS, K, F = 64, 2, 8 * 32, 200
    D = M // OS
    h = R.prototype(M, K)
    x = R.stream(F * D, M, seed=12)
    rng = np.random.default_rng(13)
    h2 = (rng.standard_normal(31) / 8).astype(np.float32)
    yd = tg.Channelizer(h, M, oversample=OS).step(dev(x))               # the (M, F) device block
    assert tuple(yd.shape) == (M, F)
    ref = O.polyphase64(x, h, M, OS)
    fir_ref = np.stack([np.convolve(r, h2.astype(np.float64))[:F] for r in ref])
    z = host(tg.FirBank(h2, tg.C64, M).step(yd))
    _rows_within_the_bar(z, fir_ref, "FirBank")
    d = host(tg.PolyFirBank(tg.POLY_DECIM, tg.C64, M, h2, 2).step(yd))
    assert d.shape == (M, F // 2)
    # the decimator applies its taps in forward order against the oldest -> newest window (tsdgpu.h; f64ref.decim): h2 reversed
    dec_ref = np.stack([np.convolve(r, h2[::-1].astype(np.float64))[:F] for r in ref])[:, 1::2]
    _rows_within_the_bar(d, dec_ref, "PolyFirBank")
