"""Real-input polyphase channelizer (include/tsdgpu.h: tsdgpu_channelizer_create_real; channelizer_real.hip) through the C ABI via
RealChannelizer, against the float64 references of tests/rchan_ref.py: the definition, parity over every first radix of the
M / 2-point transform and the tap counts around its branch lengths, the complex Channelizer on the widened stream, exactly real
rows 0 and M / 2, chunk invariance and restart bit for bit, the per-frame float64 bound at every branch length (its inputs and
bound are shown to discriminate, without a GPU, by tests/test_rchannelizer_cpu.py), long steps, layouts, exact homogeneity, the
non-finite horizon, the argument checks, and its (M / 2 + 1, F) output handed to a channel bank without a copy.

Parity inputs: the real part of chan_ref.stream (normal samples plus a cosine of amplitude 1e3 between two channels: row order and
the sign of the exponent show); prototype: Hann-windowed sinc of cutoff 1 / M.  Bar: max |y - ref| <= 1e-5 max |ref| over the step.
Per-frame inputs: the real part of poly_f64.chan_input, standard normal taps; bar: worst err / bound <= 1, poly_f64.chan's bound
with M the real frame length, no constant added."""
import ctypes
import functools

import numpy as np
import pytest

import chan_ref
import poly_f64 as PF
import rchan_ref as R
from rchan_ref import bits, dev, host, run

pytestmark = pytest.mark.gpu
TOL = 1e-5
MS = (16, 32, 64, 128, 256, 512, 1024)
FRAMES = 300


@pytest.fixture(scope="module")
def tg():
    import libtsd_amd as t
    assert t.device_count() >= 1
    return t


# --------------------------------------------------------------------------------------------------------- 1. definition
def test_small_case_against_the_definition(tg):
    M, K, F = 16, 40, 5
    h = chan_ref.prototype(M, K)
    x = R.stream(F * M, M, seed=3)
    ch = tg.RealChannelizer(h, M)
    assert (ch.rows, ch.hop, ch.history_len) == (M // 2 + 1, M, 2 * M)
    assert tg.lib().tsdgpu_channelizer_is_real(ch._h) == 1 and ch.out_count(F * M) == F
    y = run(ch, dev(x), M, [F])
    assert y.shape == (M // 2 + 1, F) and y.dtype == np.complex64
    assert R.rel_err(y, R.definition(x, h, M)) <= TOL
    other = tg.Channelizer(h, M)
    assert tg.lib().tsdgpu_channelizer_is_real(other._h) == 0 and tg.lib().tsdgpu_channelizer_rows(other._h) == M


# ------------------------------------------------------------------------------------------------------------- 2. parity
@functools.lru_cache(maxsize=None)
def parity_stream(M, F):
    x = R.stream(2 * F * M, M, seed=M + F)
    return x, dev(x)


@pytest.mark.parametrize("F", [1, 15, 16, 17, 50])
@pytest.mark.parametrize("kk", ["1", "M-3", "4M", "16M-5"])
@pytest.mark.parametrize("M", MS)
def test_parity_two_steps(tg, M, kk, F):
    K = {"1": 1, "M-3": M - 3, "4M": 4 * M, "16M-5": 16 * M - 5}[kk]
    h = chan_ref.prototype(M, K)
    x, xd = parity_stream(M, F)
    ref = R.polyphase64(x, h, M)
    ch = tg.RealChannelizer(h, M)
    assert ch.out_count(F * M) == F
    y = run(ch, xd, M, [F, F])                   # the second step starts from real history
    assert y.shape == (M // 2 + 1, 2 * F)
    err = R.rel_err(y, ref)
    print(f"M={M} K={K} F={F}: {err:.2e}")
    assert err <= TOL


# --------------------------------------------------------------------------------- 3. the complex bank, 4. exactly real rows
@pytest.mark.parametrize("M", MS)
def test_rows_agree_with_the_complex_channelizer(tg, M):
    K, F = 4 * M - 3, 33
    h = chan_ref.prototype(M, K)
    x = R.stream(F * M, M, seed=4)
    y = R.fresh_run(tg, h, M, dev(x), [F])
    yc = host(tg.Channelizer(h, M).step(dev(R.widen(x))))
    assert R.rel_err(y, yc[: M // 2 + 1].astype(np.complex128)) <= TOL
    # the rows that are not produced are conjugates, to the complex bank's own accuracy
    assert np.abs(yc[M // 2 + 1:] - np.conj(yc[M // 2 - 1:0:-1])).max() <= 2 * TOL * np.abs(yc).max()


@pytest.mark.parametrize("M", MS)
def test_rows_0_and_nyquist_are_exactly_real(tg, M):
    K, F = 3 * M + 1, 37
    x = R.stream(F * M, M, seed=5)
    y = R.fresh_run(tg, chan_ref.prototype(M, K), M, dev(x), [20, 17])
    assert y[[1, M // 2 - 1]].imag.any()
    assert (y[0].imag == 0).all() and (y[M // 2].imag == 0).all()
    assert y[0].real.any() and y[M // 2].real.any()


# ----------------------------------------------------------------------------------- 5. chunk invariance and restart, bit for bit
@pytest.mark.parametrize("kk", ["M+1", "16M"])
@pytest.mark.parametrize("M", [16, 64, 1024])
def test_chunk_invariance_and_restart_bit_for_bit(tg, M, kk):
    K = M + 1 if kk == "M+1" else 16 * M
    P = -(-K // M)
    h = chan_ref.prototype(M, K)
    F = 150
    x = R.stream(F * M, M, seed=6)
    xd = dev(x)
    one = R.fresh_run(tg, h, M, xd, [F])
    steps = PF.ragged(np.random.default_rng([5, M, K]), F)
    assert len(steps) > 2
    many = R.fresh_run(tg, h, M, xd, steps)
    assert np.array_equal(bits(one), bits(many))
    # get_state -> a fresh handle -> set_state
    cut = steps[0] + steps[1]
    a = tg.RealChannelizer(h, M)
    assert a.history_len == (P - 1) * M
    first = run(a, xd, M, steps[:2])
    st = a.get_state()
    assert st.dtype == np.float32 and st.shape == ((P - 1) * M,)
    want = np.concatenate([np.zeros((P - 1) * M, np.float32), x[:cut * M]])[cut * M:]
    assert np.array_equal(st, want)                                     # the last input floats, oldest first
    b = tg.RealChannelizer(h, M)
    b.set_state(st)
    rest = run(b, xd[cut * M:], M, [F - cut])
    assert np.array_equal(bits(np.concatenate([first, rest], axis=1)), bits(one))
    # a device-side state, and reset = a new handle
    import torch
    sd = torch.empty((P - 1) * M, dtype=torch.float32, device="cuda")
    a.get_state(sd)
    c = tg.RealChannelizer(h, M)
    c.set_state(sd)
    assert np.array_equal(bits(run(c, xd[cut * M:], M, [F - cut])), bits(rest))
    a.reset()
    assert np.array_equal(bits(run(a, xd, M, [17])), bits(one[:, :17]))


def test_no_history_below_one_branch_tap(tg):
    M = 32
    for K in (1, M - 1, M):
        ch = tg.RealChannelizer(chan_ref.prototype(M, K), M)
        assert ch.history_len == 0
        assert ch.get_state().shape == (0,)
        ch.set_state(None)                       # a null buffer is accepted
        ch.reset()


# ------------------------------------------------------------------------------------------------ 6. per-frame float64 sweep
@functools.lru_cache(maxsize=None)
def f64_data(M, frames=FRAMES):
    x = R.f64_input(np.random.default_rng([1, M, frames]), frames * M, M)
    return x, dev(x)


def run_and_judge(tg, M, h, data, steps, what):
    x, xd = data
    y64, bound = R.f64_case(x, h, M)
    y = R.fresh_run(tg, h, M, xd, steps)
    return PF.chan_judge(y, y64, bound, what), y


@pytest.mark.parametrize("P", range(1, 17))
@pytest.mark.parametrize("M", MS)
def test_branch_length_sweep(tg, M, P):
    """P: the kernel's template argument.  Two tap counts: inside the last row (zero-padded taps), and the row full.  Frames whose
    bound is 0 must come out exactly 0 (chan_judge)."""
    rng = np.random.default_rng([3, M, P])
    for K in R.two_tap_counts(rng, M, P):
        h = PF.taps(rng, K)
        what = f"rchan M={M} P={P} K={K}"
        ratio, _ = run_and_judge(tg, M, h, f64_data(M), PF.ragged(rng, FRAMES), what)
        print(f"{what}: worst err / bound {ratio:.3f}")
        assert ratio <= 1.0, what


# ------------------------------------------------------------------------------------------------------------ 7. long step
@pytest.mark.parametrize("P", [3, 16])
@pytest.mark.parametrize("M", [16, 128, 1024])
def test_long_step_second_iteration(tg, M, P):
    """F = 2 x 16 x R x grid + 17 frames (R = 512 / (M / 2) sub-runs of the M / 2-point tile, grid = 2 CUs): 2 R grid + 2 units,
    so every sub-run takes per = 3 units of the persistent loop.  Then the same stream in three odd-cut steps: the same bits."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    subruns = (1024 // M) * 2 * cus
    F = 2 * 16 * subruns + 17
    assert -(-(-(-F // 16)) // subruns) == 3                            # ceil(ceil(F / 16) / subruns)
    rng = np.random.default_rng([4, M, P])
    K = R.two_tap_counts(rng, M, P)[0]
    h = PF.taps(rng, K)
    data = f64_data(M, F)
    what = f"rchan M={M} P={P} K={K} F={F}"
    ratio, one = run_and_judge(tg, M, h, data, [F], what)
    print(f"{what}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0, what
    a, b = sorted(int(v) for v in rng.choice(np.arange(1, F, 2), 2, replace=False))
    three = R.fresh_run(tg, h, M, data[1], [a, b - a, F - b])
    assert np.array_equal(bits(one), bits(three)), what
    f64_data.cache_clear()                                              # 64 MB a side: not kept for the session


# -------------------------------------------------------------------------------------------------------------- 8. layouts
@pytest.mark.parametrize("M,K", [(16, 4 * 16 - 3), (256, 257)])
def test_layouts_give_the_same_bits(tg, M, K):
    import torch
    F, C = 20, M // 2 + 1
    h = chan_ref.prototype(M, K)
    x = R.stream(2 * F * M, M, seed=8)
    xd = dev(x)

    def two_steps(step):
        ch = tg.RealChannelizer(h, M)
        return [step(ch, 0), step(ch, 1)]

    def seg(v, i):
        return v[i * F * M:(i + 1) * F * M]

    base = two_steps(lambda ch, i: host(ch.step(seg(xd, i))).copy())
    assert R.rel_err(np.concatenate(base, axis=1), R.polyphase64(x, h, M)) <= TOL

    def strided(ld, shift):
        """rows of pitch ld from a base `shift` samples (8 B each) into an allocation"""
        def step(ch, i):
            flat = torch.full((C * ld + shift,), 7.0, dtype=torch.complex64, device="cuda")
            buf = flat[shift:].view(C, ld)
            assert buf.data_ptr() % 16 == 8 * (shift % 2)
            y = ch.step(seg(xd, i), buf[:, :F])
            assert y.data_ptr() == buf.data_ptr() and tuple(y.shape) == (C, F)
            assert ld == F or bool((buf[:, F:] == 7.0).all())           # nothing written past a row
            return host(y).copy()
        return step

    def from_host(ch, i):
        y = ch.step(seg(x, i))
        assert isinstance(y, np.ndarray) and y.dtype == np.complex64
        return y

    def host_strided(ch, i):
        buf = np.zeros((C, F + 5), np.complex64)
        return ch.step(seg(x, i), buf[:, :F]).copy()

    def host_in_device_out(ch, i):
        buf = torch.empty((C, F), dtype=torch.complex64, device="cuda")
        y = ch.step(seg(x, i), buf)
        assert y.data_ptr() == buf.data_ptr()
        return host(y).copy()

    def x_4_byte_aligned(ch, i):
        xb = torch.empty(F * M + 1, dtype=torch.float32, device="cuda")
        xb[1:] = seg(xd, i)
        assert xb[1:].data_ptr() % 8 == 4
        return host(ch.step(xb[1:])).copy()

    for name, step in (("ldy odd, base 8-B aligned", strided(F + 3, 1)), ("ldy odd", strided(F + 3, 0)),
                       ("ldy even, base 8-B aligned", strided(F + 4, 1)), ("ldy > F", strided(F + 4, 0)), ("ldy = F", strided(F, 0)),
                       ("host", from_host), ("host strided", host_strided), ("host in, device out", host_in_device_out),
                       ("x 4-B aligned", x_4_byte_aligned)):
        got = two_steps(step)
        for g, b in zip(got, base):
            assert np.array_equal(bits(g), bits(b)), name


# ---------------------------------------------------------------------------------------------------- 9. exact homogeneity
@pytest.mark.parametrize("M", [16, 64, 1024])
def test_power_of_two_scaling_is_exact(tg, M):
    K, F = 5 * M - 2, 40
    h = chan_ref.prototype(M, K)
    x = R.stream(F * M, M, seed=9)
    y = R.fresh_run(tg, h, M, dev(x), [F])
    y2 = R.fresh_run(tg, h, M, dev(x * np.float32(128.0)), [F])
    assert np.array_equal(bits(y * np.float32(128.0)), bits(y2))


# ------------------------------------------------------------------------------------------------------ 10. non-finite horizon
@pytest.mark.parametrize("what", [np.nan, np.inf])
@pytest.mark.parametrize("s", [1, 40])                                  # s = 1 meets a zero-padded tap of the last branch
def test_non_finite_horizon(tg, what, s):
    M, F = 64, 40
    K = 4 * M - 3                                                       # P = 4
    h = chan_ref.prototype(M, K)
    x = R.stream(F * M, M, seed=10)
    clean = R.fresh_run(tg, h, M, dev(x), [F])
    xb = x.copy()
    xb[9 * M + s] = what
    y = R.fresh_run(tg, h, M, dev(xb), [F])
    assert not np.isfinite(y[:, 9:13]).any()                            # every row of frames 9 .. 12
    keep = np.r_[0:9, 13:F]
    C = M // 2 + 1
    yb, cb = bits(y).reshape(C, F, 2), bits(clean).reshape(C, F, 2)
    assert np.array_equal(yb[:, keep], cb[:, keep])


# --------------------------------------------------------------------------------------------------------------- 11. errors
def test_step_errors_leave_the_stream_untouched(tg):
    import torch
    M, K, F = 64, 4 * 64 - 3, 10
    C = M // 2 + 1
    h = chan_ref.prototype(M, K)
    xd = dev(R.stream(3 * F * M, M, seed=9))
    a, b = tg.RealChannelizer(h, M), tg.RealChannelizer(h, M)
    a.step(xd[:F * M])
    b.step(xd[:F * M])
    seg = xd[F * M:2 * F * M]
    with pytest.raises(tg.TsdGpuError, match="status 1"):              # not whole frames
        a.step(xd[F * M:2 * F * M - 1])
    with pytest.raises(tg.TsdGpuError, match="status 1"):              # y_capacity too small
        a.step(seg, torch.empty((C, F - 1), dtype=torch.complex64, device="cuda"))
    # x and y share addresses, by 8 bytes: the end of x in the first sample of row 0, the start of x in the last sample of row M / 2
    flat = torch.zeros(F * M + 2 * C * F, dtype=torch.float32, device="cuda")

    def rows_at(o):
        return torch.view_as_complex(flat[o:o + 2 * C * F].view(-1, 2)).view(C, F)
    for xo, yo in ((0, F * M - 2), (2 * C * F - 2, 0)):
        flat[xo:xo + F * M] = seg
        with pytest.raises(tg.TsdGpuError, match="status 1"):
            a.step(flat[xo:xo + F * M], rows_at(yo))
        assert "overlap" in tg.lib().tsdgpu_last_error().decode()
    with pytest.raises(tg.TsdGpuError, match="row stride"):            # ldy below a row's outputs: the Python layer's check
        a.step(seg, torch.as_strided(torch.empty(C * F, dtype=torch.complex64, device="cuda"), (C, F), (F - 1, 1)))
    ybuf, got = torch.empty((C, F), dtype=torch.complex64, device="cuda"), ctypes.c_int64(-1)
    rc = tg.lib().tsdgpu_channelizer_step(a._h, seg.data_ptr(), F * M, ybuf.data_ptr(), F - 1, F, ctypes.byref(got), None)
    assert rc == 1 and got.value == 0 and "ldy" in tg.lib().tsdgpu_last_error().decode()     # the C ABI's check
    with pytest.raises(tg.TsdGpuError, match="float32"):               # a complex x
        a.step(seg.to(torch.complex64))
    with pytest.raises(tg.TsdGpuError, match="complex64"):             # a float y
        a.step(seg, torch.empty((C, F), dtype=torch.float32, device="cuda"))
    with pytest.raises(tg.TsdGpuError, match="rows"):                  # M rows, as for the complex bank
        a.step(seg, torch.empty((M, F), dtype=torch.complex64, device="cuda"))
    assert a.step(xd[:0]).shape == (C, 0)                               # n = 0: a no-op
    # rows that start where the 4-B samples of x end are no overlap
    flat[:F * M] = seg
    ya, yb = host(a.step(flat[:F * M], rows_at(F * M))), host(b.step(seg))
    assert np.array_equal(bits(ya), bits(yb))


def test_create_errors(tg):
    def fails(channels, K, status, *words, oversample=1):
        with pytest.raises(tg.TsdGpuError, match=f"status {status}"):
            tg.RealChannelizer(np.ones(K, np.float32), channels, oversample=oversample)
        msg = tg.lib().tsdgpu_last_error().decode()
        for w in words:
            assert w in msg, msg
    fails(8, 16, 3, "16", "1024")              # UNSUPPORTED, with the limit
    fails(48, 96, 3, "16", "1024")
    fails(4096, 4096, 3, "16", "1024")
    fails(2048, 2048, 3, "16", "1024")         # two positions per thread: not served
    fails(64, 16 * 64 + 1, 3, "16")
    fails(64, 128, 3, "oversample", oversample=2)
    fails(64, 128, 1, oversample=0)            # INVALID
    fails(64, 0, 1)
    fails(0, 8, 1)
    ch = tg.RealChannelizer(np.ones(16 * 64, np.float32), 64)           # the handle after the refusals is usable
    assert ch.step(dev(np.ones(64, np.float32))).shape == (33, 1)
    ch.close()


# ---------------------------------------------------------------------------------------------- 12. feeds a bank without a copy
def test_output_feeds_a_bank(tg):
    M, K, F = 64, 8 * 64, 200
    C = M // 2 + 1
    h = chan_ref.prototype(M, K)
    x = R.stream(F * M, M, seed=12)
    h2 = (np.random.default_rng(13).standard_normal(31) / 8).astype(np.float32)
    yd = tg.RealChannelizer(h, M).step(dev(x))                          # the (33, F) device block
    assert tuple(yd.shape) == (C, F) and yd.is_cuda
    ref = R.polyphase64(x, h, M)
    fir_ref = np.stack([np.convolve(r, h2.astype(np.float64))[:F] for r in ref])
    z = host(tg.FirBank(h2, tg.C64, C).step(yd))
    assert R.rel_err(z, fir_ref) <= TOL
