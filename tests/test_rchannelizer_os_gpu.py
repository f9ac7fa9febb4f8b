"""Oversampled real-input polyphase channelizer (include/tsdgpu.h: tsdgpu_channelizer_create_real_oversampled;
channelizer_real_os.hip) through the C ABI via RealChannelizer.oversampled, against the float64 references of
tests/rchan_os_ref.py: the definition from a non-zero history and phase, parity over every first radix of the M / 2-point
transform and the tap counts around the hop, the complex oversampled Channelizer on the widened stream, exactly real rows 0 and
M / 2, chunk invariance with the phase checked after every step, state + phase to a fresh handle bit for bit, OS = 1 against the
plain real bank, the per-frame float64 bound at every branch length (shown to discriminate, without a GPU, by
tests/test_rchannelizer_os_cpu.py), long steps, layouts, exact homogeneity, the non-finite horizon, the argument checks, its
(M / 2 + 1, F) output handed to a channel bank without a copy, and the round trip through the oversampled Synthesizer.

Parity inputs: rchan_ref.stream (normal samples plus a cosine of amplitude 1e3 between two channels); prototype: Hann-windowed sinc
of cutoff 1 / M.  Bar: max |y - ref| <= 1e-5 max |ref| over the step.  Per-frame inputs: rchan_ref.f64_input, standard normal
taps; bar: worst err / bound <= 1, poly_f64.chan's bound with M the real frame length, no constant added."""
import ctypes
import functools

import numpy as np
import pytest

import chan_ref
import poly_f64 as PF
import rchan_os_ref as RO
import rchan_ref as R
from rchan_os_ref import bits, dev, host, run

pytestmark = pytest.mark.gpu
TOL = 1e-5
MS = (16, 32, 64, 128, 256, 512, 1024)
OSS = (2, 4)
HOPS = 300


@pytest.fixture(scope="module")
def tg():
    import libtsd_amd as t
    assert t.device_count() >= 1
    return t


def make(tg, h, M, OS):
    return tg.RealChannelizer.oversampled(h, M, OS)


# --------------------------------------------------------------------------------------------------------- 1. definition
@pytest.mark.parametrize("OS", OSS)
def test_small_case_against_the_definition(tg, OS):
    M, F, F0 = 16, 5, 3
    D = M // OS
    K = 2 * D - 1
    P = -(-K // M)
    H = P * M - D
    h = chan_ref.prototype(M, K)
    x = R.stream((F0 + F) * D, M, seed=3)
    ch = make(tg, h, M, OS)
    assert (ch.rows, ch.hop, ch.history_len, ch.oversample, ch.phase) == (M // 2 + 1, D, H, OS, 0)
    assert tg.lib().tsdgpu_channelizer_is_real(ch._h) == 1 and ch.out_count(F * D) == F
    xd = dev(x)
    ch.step(xd[:F0 * D])                                                # an odd number of hops: a history and a phase
    assert ch.phase == F0 % OS
    y = host(ch.step(xd[F0 * D:]))
    assert y.shape == (M // 2 + 1, F) and y.dtype == np.complex64
    hist = np.concatenate([np.zeros(H, np.float32), x[:F0 * D]])[-H:]
    assert hist.any()
    assert R.rel_err(y, RO.definition(x[F0 * D:], h, M, OS, F0, hist)) <= TOL


# ------------------------------------------------------------------------------------------------------------- 2. parity
@functools.lru_cache(maxsize=None)
def parity_stream(M, OS, F):
    x = R.stream(2 * F * (M // OS), M, seed=M + F + OS)
    return x, dev(x)


@pytest.mark.parametrize("F", [1, 15, 16, 17, 50])
@pytest.mark.parametrize("kk", ["1", "D-3", "4D", "16D-5"])
@pytest.mark.parametrize("OS", OSS)
@pytest.mark.parametrize("M", MS)
def test_parity_two_steps(tg, M, OS, kk, F):
    D = M // OS
    K = {"1": 1, "D-3": D - 3, "4D": 4 * D, "16D-5": 16 * D - 5}[kk]
    h = chan_ref.prototype(M, K)
    x, xd = parity_stream(M, OS, F)
    ref = RO.polyphase64(x, h, M, OS)
    ch = make(tg, h, M, OS)
    assert ch.hop == D and ch.out_count(F * D) == F
    y = run(ch, xd, [F, F])                      # the second step starts from real history and, for odd F, a non-zero phase
    assert y.shape == (M // 2 + 1, 2 * F)
    err = R.rel_err(y, ref)
    print(f"M={M} OS={OS} K={K} F={F}: {err:.2e}")
    assert err <= TOL


# --------------------------------------------------------------------------------- 3. the complex bank, 4. exactly real rows
@pytest.mark.parametrize("OS", OSS)
@pytest.mark.parametrize("M", MS)
def test_rows_agree_with_the_complex_channelizer(tg, M, OS):
    """two banks at the 1e-5 bar each: 2e-5 of the peak between them"""
    D = M // OS
    K, F = 4 * D - 3, 33
    h = chan_ref.prototype(M, K)
    x = R.stream(F * D, M, seed=4)
    y = RO.fresh_run(tg, h, M, OS, dev(x), [F])
    yc = host(tg.Channelizer(h, M, oversample=OS).step(dev(R.widen(x))))
    assert R.rel_err(y, yc[: M // 2 + 1].astype(np.complex128)) <= 2 * TOL


@pytest.mark.parametrize("OS", OSS)
@pytest.mark.parametrize("M", MS)
def test_rows_0_and_nyquist_are_exactly_real(tg, M, OS):
    D = M // OS
    K, F = 3 * D + 1, 37
    x = R.stream(F * D, M, seed=5)
    y = RO.fresh_run(tg, chan_ref.prototype(M, K), M, OS, dev(x), [19, 18])
    assert y[[1, M // 2 - 1]].imag.any()
    assert (y[0].imag == 0).all() and (y[M // 2].imag == 0).all()
    assert y[0].real.any() and y[M // 2].real.any()


# ----------------------------------------------------------------------------------- 5. chunk invariance and state, bit for bit
@pytest.mark.parametrize("kk", ["D+1", "16D"])
@pytest.mark.parametrize("OS", OSS)
@pytest.mark.parametrize("M", [16, 64, 1024])
def test_chunk_invariance_bit_for_bit(tg, M, OS, kk):
    D = M // OS
    K = D + 1 if kk == "D+1" else 16 * D
    h = chan_ref.prototype(M, K)
    F = 150
    xd = dev(R.stream(F * D, M, seed=6))
    one = RO.fresh_run(tg, h, M, OS, xd, [F])
    steps = PF.ragged(np.random.default_rng([5, M, OS, K]), F)
    assert len(steps) > 2 and any(sum(steps[:i]) % OS for i in range(1, len(steps)))      # a step starts on a non-zero phase
    many = RO.fresh_run(tg, h, M, OS, xd, steps)                        # (run checks the phase after every step)
    assert np.array_equal(bits(one), bits(many))


@pytest.mark.parametrize("M,OS,K", [(16, 4, 16 * 4), (64, 2, 4 * 64 - 3), (1024, 2, 1025), (64, 4, 65)])
def test_state_and_phase_move_to_a_fresh_handle(tg, M, OS, K):
    import torch
    D = M // OS
    h = chan_ref.prototype(M, K)
    P = -(-K // M)
    H = P * M - D
    x = R.stream(60 * D, M, seed=6)
    xd = dev(x)
    a = make(tg, h, M, OS)
    assert a.history_len == H and a.phase == 0
    a.step(xd[:23 * D])                                                  # 23 hops: odd
    assert a.phase == 23 % OS
    st = a.get_state()
    assert st.dtype == np.float32 and st.shape == (H,)
    assert np.array_equal(st, np.concatenate([np.zeros(H, np.float32), x[:23 * D]])[-H:])    # the last input floats, oldest first
    b, nophase = make(tg, h, M, OS), make(tg, h, M, OS)
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
    sd = torch.empty(H, dtype=torch.float32, device="cuda")
    a.get_state(sd)
    c = make(tg, h, M, OS)
    c.set_state(sd)
    c.phase = a.phase
    a.step(xd[:D])                                                       # leave a on a non-zero phase before the reset
    a.reset()
    assert a.phase == 0
    fresh = host(make(tg, h, M, OS).step(xd[:17 * D]))
    assert np.array_equal(bits(host(a.step(xd[:17 * D]))), bits(fresh))
    yc, yb2 = host(c.step(xd[:17 * D])), host(b.step(xd[:17 * D]))
    assert np.array_equal(bits(yc), bits(yb2))


@pytest.mark.parametrize("M,K", [(16, 33), (32, 3 * 32), (64, 65), (128, 2 * 128), (256, 257), (1024, 1025)])
def test_oversample_one_is_the_plain_real_bank(tg, M, K):
    """one shape per first radix of the M / 2-point transform (dft8; 16, 2, 4, 8; 512 points)"""
    h = chan_ref.prototype(M, K)
    xd = dev(R.stream(37 * M, M, seed=7))
    a, b = tg.RealChannelizer(h, M), make(tg, h, M, 1)
    assert (b.hop, b.history_len, b.rows, b.phase, b.oversample) == (M, a.history_len, a.rows, 0, 1)
    assert a.phase == 0
    ya, yb = R.run(a, xd, M, [20, 17]), run(b, xd, [20, 17])
    assert np.array_equal(bits(ya), bits(yb))
    assert a.phase == b.phase == 0


# ------------------------------------------------------------------------------------------------ 6. per-frame float64 sweep
@functools.lru_cache(maxsize=None)
def f64_data(M, OS, hops=HOPS):
    x = R.f64_input(np.random.default_rng([1, M, OS, hops]), hops * (M // OS), M)
    return x, dev(x)


def run_and_judge(tg, M, OS, h, data, steps, what):
    x, xd = data
    y64, bound = RO.f64_case(x, h, M, OS)
    y = RO.fresh_run(tg, h, M, OS, xd, steps)
    return PF.chan_judge(y, y64, bound, what), y


def _sweep_cases():
    return [(M, OS, P) for M in MS for OS in OSS for P in range(1, 16 // OS + 1)]


@pytest.mark.parametrize("M,OS,P", _sweep_cases())
def test_branch_length_sweep(tg, M, OS, P):
    """P: the kernel's template argument.  Two tap counts: inside the last row (zero-padded taps), and the row full.  Frames whose
    bound is 0 must come out exactly 0 (chan_judge)."""
    rng = np.random.default_rng([3, M, OS, P])
    for K in R.two_tap_counts(rng, M, P):
        h = PF.taps(rng, K)
        what = f"rchan_os M={M} OS={OS} P={P} K={K}"
        ratio, _ = run_and_judge(tg, M, OS, h, f64_data(M, OS), PF.ragged(rng, HOPS), what)
        print(f"{what}: worst err / bound {ratio:.3f}")
        assert ratio <= 1.0, what


# ------------------------------------------------------------------------------------------------------------ 7. long step
@pytest.mark.parametrize("P", [3, 8])
@pytest.mark.parametrize("M", [16, 128, 1024])
def test_long_step_third_iteration(tg, M, P):
    """F = 2 x 16 x R x grid + 17 hops (R = 512 / (M / 2) sub-runs of the M / 2-point tile, grid = 2 CUs): 2 R grid + 2 units, so
    every sub-run takes per = 3 units of the persistent loop.  Then the same stream in three odd-cut steps: the same bits."""
    import torch
    OS = 2
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    subruns = (1024 // M) * 2 * cus
    F = 2 * 16 * subruns + 17
    assert -(-(-(-F // 16)) // subruns) == 3                            # ceil(ceil(F / 16) / subruns)
    rng = np.random.default_rng([4, M, P])
    K = R.two_tap_counts(rng, M, P)[0]
    h = PF.taps(rng, K)
    data = f64_data(M, OS, F)
    what = f"rchan_os M={M} OS={OS} P={P} K={K} F={F}"
    ratio, one = run_and_judge(tg, M, OS, h, data, [F], what)
    print(f"{what}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0, what
    a, b = sorted(int(v) for v in rng.choice(np.arange(1, F, 2), 2, replace=False))
    three = RO.fresh_run(tg, h, M, OS, data[1], [a, b - a, F - b])
    assert np.array_equal(bits(one), bits(three)), what
    f64_data.cache_clear()                                              # tens of MB a side: not kept for the session


# -------------------------------------------------------------------------------------------------------------- 8. layouts
@pytest.mark.parametrize("M,OS,K", [(16, 4, 4 * 16 - 3), (256, 2, 257)])
def test_layouts_give_the_same_bits(tg, M, OS, K):
    import torch
    F, C, D = 21, M // 2 + 1, M // OS                                   # F odd: the second step starts on a non-zero phase
    n = F * D
    h = chan_ref.prototype(M, K)
    x = R.stream(2 * n, M, seed=8)
    xd = dev(x)

    def two_steps(step):
        ch = make(tg, h, M, OS)
        return [step(ch, 0), step(ch, 1)]

    def seg(v, i):
        return v[i * n:(i + 1) * n]

    base = two_steps(lambda ch, i: host(ch.step(seg(xd, i))).copy())
    assert R.rel_err(np.concatenate(base, axis=1), RO.polyphase64(x, h, M, OS)) <= TOL

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
        buf = np.full((C, F + 5), 7.0, np.complex64)
        y = ch.step(seg(x, i), buf[:, :F]).copy()
        assert (buf[:, F:] == 7.0).all()
        return y

    def host_in_device_out(ch, i):
        buf = torch.empty((C, F), dtype=torch.complex64, device="cuda")
        y = ch.step(seg(x, i), buf)
        assert y.data_ptr() == buf.data_ptr()
        return host(y).copy()

    def x_4_byte_aligned(ch, i):
        xb = torch.empty(n + 1, dtype=torch.float32, device="cuda")
        xb[1:] = seg(xd, i)
        assert xb[1:].data_ptr() % 8 == 4
        return host(ch.step(xb[1:])).copy()

    for name, step in (("ldy odd, base 8-B aligned", strided(F + 2, 1)), ("ldy even", strided(F + 3, 0)),
                       ("ldy even, base 8-B aligned", strided(F + 3, 1)), ("ldy odd", strided(F + 4, 0)), ("ldy = F", strided(F, 0)),
                       ("host", from_host), ("host strided", host_strided), ("host in, device out", host_in_device_out),
                       ("x 4-B aligned", x_4_byte_aligned)):
        got = two_steps(step)
        for g, b in zip(got, base):
            assert np.array_equal(bits(g), bits(b)), name


# ---------------------------------------------------------------------------------------------------- 9. exact homogeneity
@pytest.mark.parametrize("OS", OSS)
@pytest.mark.parametrize("M", [16, 64, 1024])
def test_power_of_two_scaling_is_exact(tg, M, OS):
    D = M // OS
    K, F = 5 * D - 2, 41
    h = chan_ref.prototype(M, K)
    x = R.stream(F * D, M, seed=9)
    y = RO.fresh_run(tg, h, M, OS, dev(x), [F])
    y2 = RO.fresh_run(tg, h, M, OS, dev(x * np.float32(128.0)), [F])
    assert np.array_equal(bits(y * np.float32(128.0)), bits(y2))


# ------------------------------------------------------------------------------------------------------ 10. non-finite horizon
@pytest.mark.parametrize("what", [np.nan, np.inf])
@pytest.mark.parametrize("OS", OSS)
@pytest.mark.parametrize("s", [1, 12])                                  # s = 1 meets only a zero-padded tap of the last branch in its last frame
def test_non_finite_horizon(tg, what, OS, s):
    M, F, P = 64, 40, 4
    D = M // OS
    K = P * M - 3
    h = chan_ref.prototype(M, K)
    x = R.stream(F * D, M, seed=10)
    clean = RO.fresh_run(tg, h, M, OS, dev(x), [F])
    q = 9 * D + s
    assert (q // D + P * OS - 1) * D + D - 1 - q >= K if s == 1 else True        # the last frame's tap on q is a padded one
    xb = x.copy()
    xb[q] = what
    y = RO.fresh_run(tg, h, M, OS, dev(xb), [F])
    lo, hi = q // D, (q + P * M) // D
    assert hi - lo == P * OS
    assert not np.isfinite(y[:, lo:hi]).any()                           # every row of those frames
    keep = np.r_[0:lo, hi:F]
    C = M // 2 + 1
    yb, cb = bits(y).reshape(C, F, 2), bits(clean).reshape(C, F, 2)
    assert np.array_equal(yb[:, keep], cb[:, keep])


# --------------------------------------------------------------------------------------------------------------- 11. errors
def test_step_errors_leave_history_and_phase_untouched(tg):
    import torch
    M, OS, K, F = 64, 2, 4 * 64 - 3, 11                                 # F odd: the failing steps meet a non-zero phase
    D, C = M // OS, M // 2 + 1
    n = F * D
    h = chan_ref.prototype(M, K)
    xd = dev(R.stream(3 * n, M, seed=9))
    a, b = make(tg, h, M, OS), make(tg, h, M, OS)
    a.step(xd[:n])
    b.step(xd[:n])
    seg = xd[n:2 * n]
    with pytest.raises(tg.TsdGpuError, match="status 1"):              # not whole hops
        a.step(xd[n:2 * n - 1])
    assert "hops" in tg.lib().tsdgpu_last_error().decode()
    with pytest.raises(tg.TsdGpuError, match="status 1"):              # y_capacity too small
        a.step(seg, torch.empty((C, F - 1), dtype=torch.complex64, device="cuda"))
    # x and y share addresses, by 8 bytes: the end of x in the first sample of row 0, the start of x in the last sample of row M / 2
    flat = torch.zeros(n + 2 * C * F, dtype=torch.float32, device="cuda")

    def rows_at(o):
        return torch.view_as_complex(flat[o:o + 2 * C * F].view(-1, 2)).view(C, F)
    for xo, yo in ((0, n - 2), (2 * C * F - 2, 0)):
        flat[xo:xo + n] = seg
        with pytest.raises(tg.TsdGpuError, match="status 1"):
            a.step(flat[xo:xo + n], rows_at(yo))
        assert "overlap" in tg.lib().tsdgpu_last_error().decode()
    with pytest.raises(tg.TsdGpuError, match="row stride"):            # ldy below a row's outputs: the Python layer's check
        a.step(seg, torch.as_strided(torch.empty(C * F, dtype=torch.complex64, device="cuda"), (C, F), (F - 1, 1)))
    ybuf, got = torch.empty((C, F), dtype=torch.complex64, device="cuda"), ctypes.c_int64(-1)
    rc = tg.lib().tsdgpu_channelizer_step(a._h, seg.data_ptr(), n, ybuf.data_ptr(), F - 1, F, ctypes.byref(got), None)
    assert rc == 1 and got.value == 0 and "ldy" in tg.lib().tsdgpu_last_error().decode()     # the C ABI's check
    with pytest.raises(tg.TsdGpuError, match="float32"):               # a complex x
        a.step(seg.to(torch.complex64))
    with pytest.raises(tg.TsdGpuError, match="rows"):                  # M rows, as for the complex bank
        a.step(seg, torch.empty((M, F), dtype=torch.complex64, device="cuda"))
    assert a.step(xd[:0]).shape == (C, 0)                               # n = 0: a no-op
    assert a.phase == b.phase == F % OS
    # rows that start where the 4-B samples of x end are no overlap
    flat[:n] = seg
    ya, yb = host(a.step(flat[:n], rows_at(n))), host(b.step(seg))
    assert np.array_equal(bits(ya), bits(yb))
    assert a.phase == b.phase == 0
    assert np.array_equal(a.get_state(), b.get_state())


def test_create_errors(tg):
    def fails(channels, OS, K, status, *words):
        with pytest.raises(tg.TsdGpuError, match=f"status {status}"):
            make(tg, np.ones(K, np.float32), channels, OS)
        msg = tg.lib().tsdgpu_last_error().decode()
        for w in words:
            assert w in msg, msg
    for OS in OSS:
        fails(8, OS, 16, 3, "16", "1024")          # UNSUPPORTED, with the limit
        fails(48, OS, 96, 3, "16", "1024")
        fails(2048, OS, 2048, 3, "16", "1024")     # two positions per thread: not served
        fails(4096, OS, 4096, 3, "16", "1024")
        fails(64, OS, 16 * (64 // OS) + 1, 3, "16", str(16 * (64 // OS)))
        fails(64, OS, 0, 1)
    fails(64, 3, 64, 3, "oversample", "1, 2 and 4")
    fails(64, 8, 64, 3, "oversample", "1, 2 and 4")
    fails(64, 0, 64, 1)                            # INVALID
    fails(0, 2, 8, 1)
    for OS in OSS:                                 # the handle after the refusals is usable, at the limit
        ch = make(tg, np.ones(16 * (64 // OS), np.float32), 64, OS)
        assert ch.step(dev(np.ones(64 // OS, np.float32))).shape == (33, 1)
        ch.close()


# ---------------------------------------------------------------------------------------------- 12. feeds a bank without a copy
def test_output_feeds_a_bank(tg):
    M, OS, K, F = 64, 2, 8 * 32, 200
    C, D = M // 2 + 1, M // OS
    h = chan_ref.prototype(M, K)
    x = R.stream(F * D, M, seed=12)
    h2 = (np.random.default_rng(13).standard_normal(31) / 8).astype(np.float32)
    yd = make(tg, h, M, OS).step(dev(x))                                # the (33, F) device block
    assert tuple(yd.shape) == (C, F) and yd.is_cuda
    ref = RO.polyphase64(x, h, M, OS)
    fir_ref = np.stack([np.convolve(r, h2.astype(np.float64))[:F] for r in ref])
    z = host(tg.FirBank(h2, tg.C64, C).step(yd))
    assert R.rel_err(z, fir_ref) <= TOL


# ------------------------------------------------------------------------------------------------------------ 13. round trip
@pytest.mark.parametrize("OS", OSS)
@pytest.mark.parametrize("M", [16, 256])
def test_round_trip_through_the_synthesizer(tg, M, OS):
    """oversampled(h, M, OS) -> its rows extended by their conjugates on the device and delayed by one frame ->
    Synthesizer(f, M, OS), h the sine window of length M and f = h reversed: x comes back as (M OS / 2) x[p - M], real.  2e-5 of the
    peak past the first 2 M samples, the two stages' bars added (test_synthesizer_os_gpu.py::test_round_trip_on_the_device)."""
    import torch
    F, D, N = 200, M // OS, M // 2
    h = np.sin(np.pi * (np.arange(M) + 0.5) / M).astype(np.float32)
    f = np.ascontiguousarray(h[::-1])
    x = np.random.default_rng(100 + M + OS).standard_normal(F * D).astype(np.float32)         # unit variance
    buf = torch.zeros((M, F + 1), dtype=torch.complex64, device="cuda")
    yd = make(tg, h, M, OS).step(dev(x), buf[:N + 1, 1:])               # columns 1 ..: column 0 stays zero
    assert yd.data_ptr() == buf[:, 1:].data_ptr() and tuple(yd.shape) == (N + 1, F)
    buf[N + 1:] = torch.conj(buf[1:N]).flip(0)                          # row M - c = conj(row c)
    out = tg.Synthesizer(f, M, oversample=OS).step(buf[:, :F])
    assert out.is_cuda and tuple(out.shape) == (F * D,)
    got = host(out)
    want = (M * OS / 2) * np.concatenate([np.zeros(M), x.astype(np.float64)])[:F * D]
    peak = np.abs(want).max()
    er = np.abs(got.real - want)[2 * M:].max() / peak
    ei = np.abs(got.imag)[2 * M:].max() / peak
    print(f"M={M} OS={OS}: round trip {er:.2e} of the peak, imaginary part {ei:.2e}")
    assert er <= 2e-5
    assert ei <= 2e-5
