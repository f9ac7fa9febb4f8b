"""Polyphase synthesizer (include/tsdgpu.h: tsdgpu_synthesizer) against the float64 references of tests/syn_ref.py: parity over
every radix split of the transform and the tap counts around its branch lengths, many tiles and workgroups, chunk invariance
and state bit for bit, layouts (strided rows, host arrays, an 8-B aligned base), the argument checks, the non-finite horizon,
and the chain channelizer -> bank -> synthesizer on the device without a copy.

Inputs: seeded complex normal rows plus a constant 1e3 in row 3; prototype: Hann-windowed sinc of cutoff 1 / M.
Bar: max |x - ref| <= 1e-5 max |ref| over the whole step (the samples of a frame share a transform)."""
import ctypes

import numpy as np
import pytest

import chan_ref
import syn_ref as R

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
    f = R.prototype(M, K)
    u = R.rows(M, 2 * F, seed=M + K + F)
    ref = R.synth64(u, f)
    sy = tg.Synthesizer(f, M)
    assert sy.out_count(F) == F * M
    x = run(sy, dev(u), [F, F])                  # the second step starts from real history
    assert x.shape == (2 * F * M,)
    err = R.rel_err(x, ref)
    print(f"M={M} K={K} F={F}: {err:.2e}")
    assert err <= TOL


def test_small_case_against_the_definition(tg):
    M, K, F = 16, 3 * 16 - 3, 12
    f = R.prototype(M, K)
    u = R.rows(M, F, seed=3)
    x = run(tg.Synthesizer(f, M), dev(u), [F])
    assert R.rel_err(x, R.definition(u, f)) <= TOL


@pytest.mark.parametrize("M,F", [(8, 40000), (1024, 600)])
def test_many_tiles_and_workgroups(tg, M, F):
    K = 8 * M
    f = R.prototype(M, K)
    u = R.rows(M, F, seed=11)
    x = run(tg.Synthesizer(f, M), dev(u), [F])
    err = R.rel_err(x, R.synth64(u, f))
    print(f"M={M} F={F}: {err:.2e}")
    assert err <= TOL


# ----------------------------------------------------------------------------------- 2. chunk invariance and state, bit for bit
@pytest.mark.parametrize("M", [8, 64, 1024])
@pytest.mark.parametrize("kk", ["M+1", "16M"])
def test_chunk_invariance_bit_for_bit(tg, M, kk):
    K = M + 1 if kk == "M+1" else 16 * M
    f = R.prototype(M, K)
    ud = dev(R.rows(M, 150, seed=5))
    one = run(tg.Synthesizer(f, M), ud, [150])
    many = run(tg.Synthesizer(f, M), ud, [1, 15, 16, 17, 101])
    assert np.array_equal(bits(one), bits(many))


@pytest.mark.parametrize("M,K", [(8, 16 * 8), (64, 4 * 64 - 3), (1024, 1025)])
def test_state_moves_to_a_fresh_handle(tg, M, K):
    import torch
    f = R.prototype(M, K)
    P = -(-K // M)
    u = R.rows(M, 60, seed=6)
    ud = dev(u)
    a = tg.Synthesizer(f, M)
    assert a.history_len == (P - 1) * M
    a.step(ud[:, :23])
    st = a.get_state()
    assert st.shape == (M, P - 1)
    assert np.array_equal(bits(st), bits(u[:, 23 - (P - 1):23]))          # the last input columns, oldest first
    b = tg.Synthesizer(f, M)
    b.set_state(st)
    xa, xb = host(a.step(ud[:, 23:])), host(b.step(ud[:, 23:]))
    assert np.array_equal(bits(xa), bits(xb))
    # a device-side state, and reset = a new handle
    sd = torch.empty((M, P - 1), dtype=torch.complex64, device="cuda")
    a.get_state(sd)
    c = tg.Synthesizer(f, M)
    c.set_state(sd)
    a.reset()
    fresh = host(tg.Synthesizer(f, M).step(ud[:, :17]))
    assert np.array_equal(bits(host(a.step(ud[:, :17]))), bits(fresh))
    xc, xb2 = host(c.step(ud[:, :17])), host(b.step(ud[:, :17]))
    assert np.array_equal(bits(xc), bits(xb2))


def test_no_history_below_one_branch_tap(tg):
    M = 32
    for K in (1, M - 1, M):
        sy = tg.Synthesizer(R.prototype(M, K), M)
        assert sy.history_len == 0
        assert sy.get_state().shape == (M, 0)
        sy.set_state(None)                       # a null buffer is accepted
        sy.reset()


# -------------------------------------------------------------------------------------------------------------- 3. layouts
@pytest.mark.parametrize("M,K", [(16, 4 * 16 - 3), (256, 257)])
def test_layouts_give_the_same_bits(tg, M, K):
    import torch
    F = 20
    f = R.prototype(M, K)
    u = R.rows(M, 2 * F, seed=8)
    ud = dev(u)

    def two_steps(step):
        sy = tg.Synthesizer(f, M)
        return [step(sy, 0), step(sy, 1)]

    def packed(i):
        return ud[:, i * F:(i + 1) * F].contiguous()

    base = two_steps(lambda sy, i: host(sy.step(ud[:, i * F:(i + 1) * F])).copy())      # ldu = 2 F: even, 16-B aligned rows
    assert R.rel_err(np.concatenate(base), R.synth64(u, f)) <= TOL

    def strided(ld):
        def step(sy, i):
            buf = torch.zeros((M, ld), dtype=torch.complex64, device="cuda")
            buf[:, :F] = packed(i)
            out = torch.full((F * M + 8,), 7.0, dtype=torch.complex64, device="cuda")
            x = sy.step(buf[:, :F], out)
            assert x.data_ptr() == out.data_ptr() and tuple(x.shape) == (F * M,)
            assert bool((out[F * M:] == 7.0).all())                 # nothing written past F M
            return host(x).copy()
        return step

    def from_host(sy, i):
        x = sy.step(np.ascontiguousarray(u[:, i * F:(i + 1) * F]))
        assert isinstance(x, np.ndarray)
        return x

    def host_strided(sy, i):
        return sy.step(u[:, i * F:(i + 1) * F]).copy()

    def misaligned_rows(sy, i):
        buf = torch.zeros(M * F + 1, dtype=torch.complex64, device="cuda")
        rows = buf[1:].view(M, F)
        rows.copy_(packed(i))
        assert rows.data_ptr() % 16 == 8
        return host(sy.step(rows)).copy()

    def misaligned_x(sy, i):
        out = torch.full((F * M + 9,), 7.0, dtype=torch.complex64, device="cuda")
        assert out[1:].data_ptr() % 16 == 8
        x = sy.step(packed(i), out[1:])
        assert bool((out[F * M + 1:] == 7.0).all()) and bool(out[0] == 7.0)
        return host(x).copy()

    for name, step in (("ldu odd", strided(F + 3)), ("ldu = F", strided(F)), ("host", from_host), ("host strided", host_strided),
                       ("rows 8-B aligned", misaligned_rows), ("x 8-B aligned", misaligned_x)):
        got = two_steps(step)
        for g, b in zip(got, base):
            assert np.array_equal(bits(g), bits(b)), name


# --------------------------------------------------------------------------------------------------------------- 4. errors
def test_step_errors_leave_the_stream_untouched(tg):
    import torch
    M, K, F = 64, 4 * 64 - 3, 10
    f = R.prototype(M, K)
    ud = dev(R.rows(M, 3 * F, seed=9))
    a, b = tg.Synthesizer(f, M), tg.Synthesizer(f, M)
    a.step(ud[:, :F])
    b.step(ud[:, :F])
    seg = ud[:, F:2 * F].contiguous()
    with pytest.raises(tg.TsdGpuError, match="status 1"):              # x_capacity too small
        a.step(seg, torch.empty(F * M - 1, dtype=torch.complex64, device="cuda"))
    big = torch.zeros(2 * F * M, dtype=torch.complex64, device="cuda")
    big[:F * M] = seg.reshape(-1)
    with pytest.raises(tg.TsdGpuError, match="status 1"):              # u and x share addresses
        a.step(big[:F * M].view(M, F), big[F * M // 2:F * M // 2 + F * M])
    with pytest.raises(tg.TsdGpuError, match="row stride"):            # ldu below a channel's inputs: the Python layer's check
        a.step(torch.as_strided(big, (M, F), (F - 1, 1)))
    xbuf, got = torch.empty(F * M, dtype=torch.complex64, device="cuda"), ctypes.c_int64(-1)
    rc = tg.lib().tsdgpu_synthesizer_step(a._h, seg.data_ptr(), F - 1, F, xbuf.data_ptr(), F * M, ctypes.byref(got), None)
    assert rc == 1 and got.value == 0 and "ldu" in tg.lib().tsdgpu_last_error().decode()     # the C ABI's check
    with pytest.raises(tg.TsdGpuError):                                 # wrong dtype, wrong ndim
        a.step(seg.real.contiguous())
    with pytest.raises(tg.TsdGpuError):
        a.step(seg.reshape(-1))
    assert a.step(ud[:, :0]).shape == (0,)                              # frames = 0: a no-op
    xa, xb = host(a.step(seg)), host(b.step(seg))
    assert np.array_equal(bits(xa), bits(xb))


def test_create_errors(tg):
    def fails(channels, K, status, *words):
        with pytest.raises(tg.TsdGpuError, match=f"status {status}"):
            tg.Synthesizer(np.ones(K, np.float32), channels)
        msg = tg.lib().tsdgpu_last_error().decode()
        for w in words:
            assert w in msg, msg
    fails(12, 24, 3, "8", "1024")              # UNSUPPORTED, with the limit
    fails(4, 8, 3, "8", "1024")
    fails(2048, 2048, 3, "8", "1024")
    fails(64, 16 * 64 + 1, 3, "16")
    fails(64, 0, 1)                            # INVALID
    fails(0, 8, 1)
    tg.Synthesizer(np.ones(16 * 64, np.float32), 64).close()


# ---------------------------------------------------------------------------------------------------- 5. non-finite horizon
@pytest.mark.parametrize("what", [np.nan, np.inf])
@pytest.mark.parametrize("c", [1, 40])
def test_non_finite_horizon(tg, what, c):
    M, F = 64, 40
    K = 4 * M - 3                                                       # P = 4: the last branch has zero-padded taps
    f = R.prototype(M, K)
    u = R.rows(M, F, seed=10)
    clean = run(tg.Synthesizer(f, M), dev(u), [F]).reshape(F, M)
    ub = u.copy()
    ub[c, 9] = what
    x = run(tg.Synthesizer(f, M), dev(ub), [F]).reshape(F, M)
    bad = x[9:13]                                                       # every sample of frames 9 .. 12
    assert not (np.isfinite(bad.real) & np.isfinite(bad.imag)).any()
    keep = np.r_[0:9, 13:F]
    assert np.array_equal(bits(x[keep]), bits(clean[keep]))


# ------------------------------------------------------------------------------ 6. channelizer -> bank -> synthesizer on device
def test_chain_on_the_device(tg):
    M, K, F = 64, 8 * 64, 200
    h = R.prototype(M, K)
    x = chan_ref.stream(F * M, M, seed=12)
    rng = np.random.default_rng(13)
    h2 = (rng.standard_normal(31) / 8).astype(np.float32)
    yd = tg.Channelizer(h, M).step(dev(x))                              # the (M, F) device block
    zd = tg.FirBank(h2, tg.C64, M).step(yd)
    assert zd.is_cuda and tuple(zd.shape) == (M, F)
    out = tg.Synthesizer(h, M).step(zd)
    assert out.is_cuda and tuple(out.shape) == (F * M,)
    z = host(zd)
    assert R.rel_err(host(out), R.synth64(z, h)) <= TOL


def test_synthesis_undoes_analysis_on_the_device(tg):
    """K = M, f[s] = 1 / (M h[M - 1 - s]): the synthesizer gives the channelizer's input back.  The prototype is a ramp from 1 / M to
    2 / M: not symmetric, so the reversal of the taps shows, and with a ratio of 2 between its extremes, so the inverse taps stay at
    1/2 .. 1 and the 1e-5 bar is about the two kernels.  (The Hann-windowed sinc of the other tests has edge taps of 2e-5 against
    1.6e-2 at its centre: its inverse taps, up to 700, multiply the first bank's float32 rounding -- 2.2e-4 of the peak when tried.)
    What is left is the channelizer's rounding of y, up to 5e-7 of its peak in tests/test_channelizer_gpu.py, summed over the M
    bins of the inverse transform: a float64 run with noise of that size added to y gives 2.5e-6 at M = 16."""
    M, F = 16, 200
    h = ((1.0 + np.arange(M) / M) / M).astype(np.float32)
    f = (1.0 / (M * h[::-1].astype(np.float64))).astype(np.float32)
    x = chan_ref.stream(F * M, M, seed=14)
    out = host(tg.Synthesizer(f, M).step(tg.Channelizer(h, M).step(dev(x))))
    ref = R.synth64(chan_ref.polyphase64(x, h, M), f)                   # the float64 composition: x up to the taps' rounding
    assert R.rel_err(ref, x.astype(np.complex128)) <= 1e-6
    e_ref, e_x = R.rel_err(out, ref), R.rel_err(out, x.astype(np.complex128))
    print(f"against the float64 composition {e_ref:.2e}, against x {e_x:.2e}")
    assert e_ref <= TOL and e_x <= TOL
