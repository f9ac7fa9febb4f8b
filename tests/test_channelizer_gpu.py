"""Polyphase channelizer (include/tsdgpu.h: tsdgpu_channelizer) against the float64 references of tests/chan_ref.py: parity over
every radix split of the transform and the tap counts around its branch lengths, many tiles and workgroups, chunk invariance
and state bit for bit, layouts (strided rows, host arrays, an 8-B aligned base), the argument checks, the non-finite horizon,
and its (M, F) output handed to the channel banks without a copy.

Inputs: seeded complex normal samples plus a tone of amplitude 1e3 between two channels; prototype: Hann-windowed sinc of cutoff
1 / M.  Bar: max |y - ref| <= 1e-5 max |ref| over the whole step (the channels share a transform)."""
import ctypes

import numpy as np
import pytest

import chan_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-5
MS = (8, 16, 32, 64, 128, 256, 512, 1024)


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


def run(ch, xd, M, frames):
    """the stream through the handle in steps of the given frame counts; the (M, sum(frames)) outputs side by side (host)"""
    import torch
    outs, a = [], 0
    for f in frames:
        outs.append(ch.step(xd[a * M:(a + f) * M]))
        a += f
    return host(torch.cat(outs, dim=1))


# ------------------------------------------------------------------------------------------------------------ 1. parity
# every M with K = 16 M and K = M + 1 at every F; the other tap counts at F = 2 and 17 (17 straddles a 16-frame unit)
def _parity_cases():
    out = []
    for M in MS:
        for K in (1, M - 1, M, M + 1, 4 * M - 3, 16 * M):
            for F in (1, 2, 17, 100):
                if K in (16 * M, M + 1) or F in (2, 17):
                    out.append((M, K, F))
    return out


@pytest.mark.parametrize("M,K,F", _parity_cases())
def test_parity_two_steps(tg, M, K, F):
    h = R.prototype(M, K)
    x = R.stream(2 * F * M, M, seed=M + K + F)
    ref = R.polyphase64(x, h, M)
    ch = tg.Channelizer(h, M)
    assert ch.out_count(F * M) == F
    y = run(ch, dev(x), M, [F, F])               # the second step starts from real history
    assert y.shape == (M, 2 * F)
    err = R.rel_err(y, ref)
    print(f"M={M} K={K} F={F}: {err:.2e}")
    assert err <= TOL


def test_small_case_against_the_definition(tg):
    M, K, F = 16, 3 * 16 - 3, 12
    h = R.prototype(M, K)
    x = R.stream(F * M, M, seed=3)
    y = run(tg.Channelizer(h, M), dev(x), M, [F])
    assert R.rel_err(y, R.definition(x, h, M)) <= TOL


@pytest.mark.parametrize("M,F", [(8, 40000), (1024, 600)])
def test_many_tiles_and_workgroups(tg, M, F):
    K = 8 * M
    h = R.prototype(M, K)
    x = R.stream(F * M, M, seed=11)
    y = run(tg.Channelizer(h, M), dev(x), M, [F])
    err = R.rel_err(y, R.polyphase64(x, h, M))
    print(f"M={M} F={F}: {err:.2e}")
    assert err <= TOL


# ----------------------------------------------------------------------------------- 2. chunk invariance and state, bit for bit
@pytest.mark.parametrize("M", [8, 64, 1024])
@pytest.mark.parametrize("kk", ["M+1", "16M"])
def test_chunk_invariance_bit_for_bit(tg, M, kk):
    K = M + 1 if kk == "M+1" else 16 * M
    h = R.prototype(M, K)
    xd = dev(R.stream(150 * M, M, seed=5))
    one = run(tg.Channelizer(h, M), xd, M, [150])
    many = run(tg.Channelizer(h, M), xd, M, [1, 15, 16, 17, 101])
    assert np.array_equal(one.view(np.uint32), many.view(np.uint32))


@pytest.mark.parametrize("M,K", [(8, 16 * 8), (64, 4 * 64 - 3), (1024, 1025)])
def test_state_moves_to_a_fresh_handle(tg, M, K):
    h = R.prototype(M, K)
    P = -(-K // M)
    xd = dev(R.stream(60 * M, M, seed=6))
    a = tg.Channelizer(h, M)
    assert a.history_len == (P - 1) * M
    a.step(xd[:23 * M])
    st = a.get_state()
    assert st.shape == ((P - 1) * M,)
    assert np.array_equal(st, host(xd)[23 * M - (P - 1) * M:23 * M])     # the last inputs, oldest first
    b = tg.Channelizer(h, M)
    b.set_state(st)
    ya, yb = host(a.step(xd[23 * M:])), host(b.step(xd[23 * M:]))
    assert np.array_equal(ya.view(np.uint32), yb.view(np.uint32))
    # a device-side state, and reset = a new handle
    import torch
    sd = torch.empty((P - 1) * M, dtype=torch.complex64, device="cuda")
    a.get_state(sd)
    c = tg.Channelizer(h, M)
    c.set_state(sd)
    a.reset()
    fresh = host(tg.Channelizer(h, M).step(xd[:17 * M]))
    assert np.array_equal(host(a.step(xd[:17 * M])).view(np.uint32), fresh.view(np.uint32))
    yc, yb2 = host(c.step(xd[:17 * M])), host(b.step(xd[:17 * M]))
    assert np.array_equal(yc.view(np.uint32), yb2.view(np.uint32))


def test_no_history_below_one_branch_tap(tg):
    M = 32
    for K in (1, M - 1, M):
        ch = tg.Channelizer(R.prototype(M, K), M)
        assert ch.history_len == 0
        assert ch.get_state().shape == (0,)
        ch.set_state(None)                       # a null buffer is accepted
        ch.reset()


# -------------------------------------------------------------------------------------------------------------- 3. layouts
@pytest.mark.parametrize("M,K", [(16, 4 * 16 - 3), (256, 257)])
def test_layouts_give_the_same_bits(tg, M, K):
    import torch
    F = 20
    h = R.prototype(M, K)
    x = R.stream(2 * F * M, M, seed=8)
    xd = dev(x)

    def two_steps(step):
        ch = tg.Channelizer(h, M)
        return [step(ch, 0), step(ch, 1)]

    base = two_steps(lambda ch, i: host(ch.step(xd[i * F * M:(i + 1) * F * M])).copy())
    assert R.rel_err(np.concatenate(base, axis=1), R.polyphase64(x, h, M)) <= TOL

    def strided(ld):
        def step(ch, i):
            buf = torch.full((M, ld), 7.0, dtype=torch.complex64, device="cuda")
            y = ch.step(xd[i * F * M:(i + 1) * F * M], buf[:, :F])
            assert y.data_ptr() == buf.data_ptr() and tuple(y.shape) == (M, F)
            assert ld == F or bool((buf[:, F:] == 7.0).all())       # nothing written past a row
            return host(y).copy()
        return step

    def from_host(ch, i):
        y = ch.step(x[i * F * M:(i + 1) * F * M])
        assert isinstance(y, np.ndarray)
        return y

    def host_strided(ch, i):
        buf = np.zeros((M, F + 5), np.complex64)
        return ch.step(x[i * F * M:(i + 1) * F * M], buf[:, :F]).copy()

    def misaligned(ch, i):
        xb = torch.empty(F * M + 1, dtype=torch.complex64, device="cuda")
        xb[1:] = xd[i * F * M:(i + 1) * F * M]
        assert xb[1:].data_ptr() % 16 == 8
        return host(ch.step(xb[1:])).copy()

    for name, step in (("ldy odd", strided(F + 3)), ("ldy = F", strided(F)), ("host", from_host), ("host strided", host_strided),
                       ("x 8-B aligned", misaligned)):
        got = two_steps(step)
        for g, b in zip(got, base):
            assert np.array_equal(g.view(np.uint32), b.view(np.uint32)), name


# --------------------------------------------------------------------------------------------------------------- 4. errors
def test_step_errors_leave_the_stream_untouched(tg):
    import torch
    M, K, F = 64, 4 * 64 - 3, 10
    h = R.prototype(M, K)
    xd = dev(R.stream(3 * F * M, M, seed=9))
    a, b = tg.Channelizer(h, M), tg.Channelizer(h, M)
    a.step(xd[:F * M])
    b.step(xd[:F * M])
    seg = xd[F * M:2 * F * M]
    with pytest.raises(tg.TsdGpuError, match="status 1"):              # not whole frames
        a.step(xd[F * M:2 * F * M - 1])
    with pytest.raises(tg.TsdGpuError, match="status 1"):              # y_capacity too small
        a.step(seg, torch.empty((M, F - 1), dtype=torch.complex64, device="cuda"))
    big = torch.zeros(2 * F * M, dtype=torch.complex64, device="cuda")
    big[:F * M] = seg
    with pytest.raises(tg.TsdGpuError, match="status 1"):              # x and y share addresses
        a.step(big[:F * M], big[F * M // 2:F * M // 2 + F * M].view(M, F))
    with pytest.raises(tg.TsdGpuError, match="row stride"):            # ldy below a channel's outputs: the Python layer's check
        a.step(seg, torch.as_strided(big, (M, F), (F - 1, 1), F * M))
    ybuf, got = torch.empty((M, F), dtype=torch.complex64, device="cuda"), ctypes.c_int64(-1)
    rc = tg.lib().tsdgpu_channelizer_step(a._h, seg.data_ptr(), F * M, ybuf.data_ptr(), F - 1, F, ctypes.byref(got), None)
    assert rc == 1 and got.value == 0 and "ldy" in tg.lib().tsdgpu_last_error().decode()     # the C ABI's check
    assert a.step(xd[:0]).shape == (M, 0)                               # n = 0: a no-op
    ya, yb = host(a.step(seg)), host(b.step(seg))
    assert np.array_equal(ya.view(np.uint32), yb.view(np.uint32))


def test_create_errors(tg):
    def fails(channels, K, status, *words):
        with pytest.raises(tg.TsdGpuError, match=f"status {status}"):
            tg.Channelizer(np.ones(K, np.float32), channels)
        msg = tg.lib().tsdgpu_last_error().decode()
        for w in words:
            assert w in msg, msg
    fails(12, 24, 3, "8", "1024")              # UNSUPPORTED, with the limit
    fails(4, 8, 3, "8", "1024")
    fails(2048, 2048, 3, "8", "1024")
    fails(64, 16 * 64 + 1, 3, "16")
    fails(64, 0, 1)                            # INVALID
    fails(0, 8, 1)
    tg.Channelizer(np.ones(16 * 64, np.float32), 64).close()


# ---------------------------------------------------------------------------------------------------- 5. non-finite horizon
@pytest.mark.parametrize("what", [np.nan, np.inf])
@pytest.mark.parametrize("s", [1, 40])                                  # s = 1 meets a zero-padded tap of the last branch
def test_non_finite_horizon(tg, what, s):
    M, F = 64, 40
    K = 4 * M - 3                                                       # P = 4
    h = R.prototype(M, K)
    x = R.stream(F * M, M, seed=10)
    clean = run(tg.Channelizer(h, M), dev(x), M, [F])
    xb = x.copy()
    xb[9 * M + s] = what
    y = run(tg.Channelizer(h, M), dev(xb), M, [F])
    assert not np.isfinite(y[:, 9:13]).any()                            # every channel of frames 9 .. 12
    keep = np.r_[0:9, 13:F]
    yb, cb = y.view(np.uint32).reshape(M, F, 2), clean.view(np.uint32).reshape(M, F, 2)
    assert np.array_equal(yb[:, keep], cb[:, keep])


# -------------------------------------------------------------------------------------------- 6. feeds a bank without a copy
def test_output_feeds_the_banks(tg):
    M, K, F = 64, 8 * 64, 200
    h = R.prototype(M, K)
    x = R.stream(F * M, M, seed=12)
    rng = np.random.default_rng(13)
    h2 = (rng.standard_normal(31) / 8).astype(np.float32)
    yd = tg.Channelizer(h, M).step(dev(x))                              # the (M, F) device block
    ref = R.polyphase64(x, h, M)
    fir_ref = np.stack([np.convolve(r, h2.astype(np.float64))[:F] for r in ref])
    z = host(tg.FirBank(h2, tg.C64, M).step(yd))
    assert R.rel_err(z, fir_ref) <= TOL
    d = host(tg.PolyFirBank(tg.POLY_DECIM, tg.C64, M, h2, 2).step(yd))
    assert d.shape == (M, F // 2)
    # the decimator applies its taps in forward order against the oldest -> newest window (tsdgpu.h; f64ref.decim): h2 reversed
    dec_ref = np.stack([np.convolve(r, h2[::-1].astype(np.float64))[:F] for r in ref])[:, 1::2]
    assert R.rel_err(d, dec_ref) <= TOL
