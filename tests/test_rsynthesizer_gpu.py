"""Real-output polyphase synthesizer (include/tsdgpu.h: tsdgpu_synthesizer_create_real; synthesizer_real.hip) through the C ABI via
RealSynthesizer, against the float64 references of tests/rsyn_ref.py: the definition, parity over every first radix of the
M / 2-point transform and the tap counts around its branch lengths, the complex Synthesizer on the extended block, the imaginary
parts of rows 0 and M / 2 that are not used, chunk invariance and restart bit for bit, the per-sample float64 bound at every branch
length (its inputs and bound are shown to discriminate, without a GPU, by tests/test_rsynthesizer_cpu.py), long steps, layouts,
exact homogeneity, the non-finite horizon, the argument checks, and the round trips RealChannelizer -> (banks) -> RealSynthesizer
on the device.

Parity inputs: rows 0 .. M / 2 of syn_ref.rows (complex normal rows plus a constant 1e3 in row 3); prototype: Hann-windowed sinc of
cutoff 1 / M.  Bar: max |x - ref| <= 1e-5 max |ref| over the step.  Per-sample inputs: rows 0 .. M / 2 of poly_f64.syn_input,
standard normal taps; bar: worst err / bound <= 1, poly_f64.syn's bound on the extended block with M the real frame length, no
constant added."""
import ctypes
import functools

import numpy as np
import pytest

import chan_ref
import poly_f64 as PF
import rchan_ref
import rsyn_ref as R
import syn_ref
from rsyn_ref import bits, dev, host, run

pytestmark = pytest.mark.gpu
TOL = 1e-5
MS = (16, 32, 64, 128, 256, 512, 1024)
FRAMES = 300


@pytest.fixture(scope="module")
def tg():
    import libtsd_amd as t
    assert t.device_count() >= 1
    return t


def half_rows(M, F, seed):
    return np.ascontiguousarray(syn_ref.rows(M, F, seed)[: M // 2 + 1])


# --------------------------------------------------------------------------------------------------------- 1. definition
def test_small_case_against_the_definition(tg):
    M, K, F = 16, 40, 5
    f = chan_ref.prototype(M, K)
    u = half_rows(M, F, seed=3)
    sy = tg.RealSynthesizer(f, M)
    assert (sy.rows, sy.hop, sy.history_len, sy.frames_kept) == (M // 2 + 1, M, 2 * (M // 2 + 1), 2)
    L = tg.lib()
    assert L.tsdgpu_synthesizer_is_real(sy._h) == 1 and L.tsdgpu_synthesizer_rows(sy._h) == M // 2 + 1
    assert L.tsdgpu_synthesizer_history_len(sy._h) == 2 * (M // 2 + 1) and sy.out_count(F) == F * M
    x = run(sy, dev(u), [F])
    assert x.shape == (F * M,) and x.dtype == np.float32
    assert R.rel_err(x, R.definition(u, f)) <= TOL
    other = tg.Synthesizer(f, M)
    assert L.tsdgpu_synthesizer_is_real(other._h) == 0 and L.tsdgpu_synthesizer_rows(other._h) == M
    assert (other.hop, other.history_len) == (M, 2 * M)


# ------------------------------------------------------------------------------------------------------------- 2. parity
@functools.lru_cache(maxsize=None)
def parity_rows(M, F):
    u = half_rows(M, 2 * F, seed=M + F)
    return u, dev(u)


@pytest.mark.parametrize("F", [1, 15, 16, 17, 50])
@pytest.mark.parametrize("kk", ["1", "M-3", "4M", "16M-5"])
@pytest.mark.parametrize("M", MS)
def test_parity_two_steps(tg, M, kk, F):
    K = {"1": 1, "M-3": M - 3, "4M": 4 * M, "16M-5": 16 * M - 5}[kk]
    f = chan_ref.prototype(M, K)
    u, ud = parity_rows(M, F)
    ref = R.synth64(u, f)
    sy = tg.RealSynthesizer(f, M)
    assert sy.out_count(F) == F * M
    x = run(sy, ud, [F, F])                      # the second step starts from real history
    assert x.shape == (2 * F * M,)
    err = R.rel_err(x, ref)
    print(f"M={M} K={K} F={F}: {err:.2e}")
    assert err <= TOL


# ------------------------------------------------------------------- 3. the complex bank, 4. the parts that are not used
@pytest.mark.parametrize("M", MS)
def test_agrees_with_the_complex_synthesizer_on_the_extended_block(tg, M):
    K, F = 4 * M - 3, 33
    f = chan_ref.prototype(M, K)
    u = half_rows(M, F, seed=4)
    x = R.fresh_run(tg, f, M, dev(u), [F])
    xc = host(tg.Synthesizer(f, M).step(dev(R.extend(u))))
    peak = np.abs(x).max()
    assert np.abs(xc.real.astype(np.float64) - x).max() <= TOL * peak
    assert np.abs(xc.imag).max() <= 2 * TOL * peak


@pytest.mark.parametrize("M", MS)
def test_imaginary_parts_of_rows_0_and_nyquist_are_not_used(tg, M):
    K, F = 3 * M + 1, 37
    N = M // 2
    f = chan_ref.prototype(M, K)
    u = half_rows(M, F, seed=5)
    assert u[0].imag.any() and u[N].imag.any()
    base = R.fresh_run(tg, f, M, dev(u), [20, 17])
    rng = np.random.default_rng(M)
    for what in ("zero", "garbage", "nan"):
        v = u.copy()
        for c in (0, N):
            v[c].imag = {"zero": 0.0, "garbage": 1e30 * rng.standard_normal(F), "nan": np.nan}[what]
        got = R.fresh_run(tg, f, M, dev(v), [20, 17])                    # the second step reads them from the history too
        assert np.array_equal(bits(got), bits(base)), what
    v = u.copy()
    v[1].imag += 1.0                                                     # (a part that IS used shows)
    assert not np.array_equal(bits(R.fresh_run(tg, f, M, dev(v), [20, 17])), bits(base))


# ----------------------------------------------------------------------------------- 5. chunk invariance and restart, bit for bit
@pytest.mark.parametrize("kk", ["M+1", "16M"])
@pytest.mark.parametrize("M", [16, 64, 1024])
def test_chunk_invariance_and_restart_bit_for_bit(tg, M, kk):
    K = M + 1 if kk == "M+1" else 16 * M
    P, C = -(-K // M), M // 2 + 1
    f = chan_ref.prototype(M, K)
    F = 150
    u = half_rows(M, F, seed=6)
    ud = dev(u)
    one = R.fresh_run(tg, f, M, ud, [F])
    steps = PF.ragged(np.random.default_rng([5, M, K]), F)
    assert len(steps) > 2
    many = R.fresh_run(tg, f, M, ud, steps)
    assert np.array_equal(bits(one), bits(many))
    # get_state -> a fresh handle -> set_state
    cut = steps[0] + steps[1]
    a = tg.RealSynthesizer(f, M)
    assert a.history_len == (P - 1) * C and a.frames_kept == P - 1
    first = run(a, ud, steps[:2])
    st = a.get_state()
    assert st.dtype == np.complex64 and st.shape == (C, P - 1)
    want = np.concatenate([np.zeros((C, P - 1), np.complex64), u[:, :cut]], axis=1)[:, cut:]
    assert np.array_equal(bits(st), bits(want))                         # the last input frames as they were fed, oldest first
    b = tg.RealSynthesizer(f, M)
    b.set_state(st)
    rest = run(b, ud[:, cut:], [F - cut])
    assert np.array_equal(bits(np.concatenate([first, rest])), bits(one))
    # a device-side state, and reset = a new handle
    import torch
    sd = torch.empty((C, P - 1), dtype=torch.complex64, device="cuda")
    a.get_state(sd)
    c = tg.RealSynthesizer(f, M)
    c.set_state(sd)
    assert np.array_equal(bits(run(c, ud[:, cut:], [F - cut])), bits(rest))
    a.reset()
    assert np.array_equal(bits(run(a, ud, [17])), bits(one[:17 * M]))


def test_no_history_below_one_branch_tap(tg):
    M = 32
    for K in (1, M - 1, M):
        sy = tg.RealSynthesizer(chan_ref.prototype(M, K), M)
        assert sy.history_len == 0 and sy.frames_kept == 0
        assert sy.get_state().shape == (M // 2 + 1, 0)
        sy.set_state(None)                       # a null buffer is accepted
        sy.reset()


# ----------------------------------------------------------------------------------------------- 6. per-sample float64 sweep
@functools.lru_cache(maxsize=None)
def f64_data(M, frames=FRAMES):
    u = R.input(np.random.default_rng([1, M, frames]), M, frames)
    return u, dev(u)


def run_and_judge(tg, M, f, data, steps, what):
    u, ud = data
    x64, bound = R.f64_case(u, f, M)
    x = R.fresh_run(tg, f, M, ud, steps)
    return PF.syn_judge(x, x64, bound, what), x


@pytest.mark.parametrize("P", range(1, 17))
@pytest.mark.parametrize("M", MS)
def test_branch_length_sweep(tg, M, P):
    """P: the kernel's template argument.  Two tap counts: inside the last row (zero-padded taps), and the row full.  Samples
    whose bound is 0 must come out exactly 0 (syn_judge)."""
    rng = np.random.default_rng([3, M, P])
    for K in rchan_ref.two_tap_counts(rng, M, P):
        f = PF.taps(rng, K)
        what = f"rsyn M={M} P={P} K={K}"
        ratio, _ = run_and_judge(tg, M, f, f64_data(M), PF.ragged(rng, FRAMES), what)
        print(f"{what}: worst err / bound {ratio:.3f}")
        assert ratio <= 1.0, what


# ------------------------------------------------------------------------------------------------------------ 7. long step
@pytest.mark.parametrize("P", [3, 16])
@pytest.mark.parametrize("M", [16, 128, 1024])
def test_long_step_second_iteration(tg, M, P):
    """F = 2 x 16 x R x grid + 17 frames (R = 512 / (M / 2) sub-runs of the M / 2-point tile, grid = 2 CUs): 2 R grid + 2 units,
    so every sub-run takes per = 3 units of the persistent loop.  Then the same rows in three odd-cut steps: the same bits."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    subruns = (1024 // M) * 2 * cus
    F = 2 * 16 * subruns + 17
    assert -(-(-(-F // 16)) // subruns) == 3                            # ceil(ceil(F / 16) / subruns)
    rng = np.random.default_rng([4, M, P])
    K = rchan_ref.two_tap_counts(rng, M, P)[0]
    f = PF.taps(rng, K)
    data = f64_data(M, F)
    what = f"rsyn M={M} P={P} K={K} F={F}"
    ratio, one = run_and_judge(tg, M, f, data, [F], what)
    print(f"{what}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0, what
    a, b = sorted(int(v) for v in rng.choice(np.arange(1, F, 2), 2, replace=False))
    three = R.fresh_run(tg, f, M, data[1], [a, b - a, F - b])
    assert np.array_equal(bits(one), bits(three)), what
    f64_data.cache_clear()                                              # tens of MB a side: not kept for the session


# -------------------------------------------------------------------------------------------------------------- 8. layouts
@pytest.mark.parametrize("M,K", [(16, 4 * 16 - 3), (256, 257)])
def test_layouts_give_the_same_bits(tg, M, K):
    import torch
    F, C = 20, M // 2 + 1
    f = chan_ref.prototype(M, K)
    u = half_rows(M, 2 * F, seed=8)
    ud = dev(u)

    def two_steps(step):
        sy = tg.RealSynthesizer(f, M)
        return [step(sy, 0), step(sy, 1)]

    def seg(v, i):
        return v[:, i * F:(i + 1) * F]

    base = two_steps(lambda sy, i: host(sy.step(seg(ud, i).contiguous())).copy())
    assert R.rel_err(np.concatenate(base), R.synth64(u, f)) <= TOL

    def strided(ld, shift):
        """rows of pitch ld from a base `shift` samples (8 B each) into an allocation"""
        def step(sy, i):
            flat = torch.zeros(C * ld + shift, dtype=torch.complex64, device="cuda")
            buf = flat[shift:].view(C, ld)
            assert buf.data_ptr() % 16 == 8 * (shift % 2)
            buf[:, :F] = seg(ud, i)
            return host(sy.step(buf[:, :F])).copy()
        return step

    def unsplit(sy, i):
        return host(sy.step(seg(ud, i))).copy()                          # a column range of the whole block: ldu = 2 F

    def from_host(sy, i):
        x = sy.step(np.ascontiguousarray(seg(u, i)))
        assert isinstance(x, np.ndarray) and x.dtype == np.float32
        return x

    def host_strided(sy, i):
        return sy.step(seg(u, i)).copy()

    def host_in_device_out(sy, i):
        buf = torch.empty(F * M, dtype=torch.float32, device="cuda")
        x = sy.step(np.ascontiguousarray(seg(u, i)), buf)
        assert x.data_ptr() == buf.data_ptr()
        return host(x).copy()

    def x_supplied(sy, i):
        buf = torch.full((F * M + 10,), 7.0, dtype=torch.float32, device="cuda")
        x = sy.step(seg(ud, i), buf)
        assert x.data_ptr() == buf.data_ptr() and tuple(x.shape) == (F * M,)
        assert bool((buf[F * M:] == 7.0).all())                          # nothing written past the step
        return host(x).copy()

    def x_4_byte_aligned(sy, i):
        buf = torch.full((F * M + 11,), 7.0, dtype=torch.float32, device="cuda")
        assert buf[1:].data_ptr() % 8 == 4
        x = sy.step(seg(ud, i), buf[1:])
        assert bool((buf[F * M + 1:] == 7.0).all()) and bool(buf[0] == 7.0)
        return host(x).copy()

    for name, step in (("ldu odd, base 8-B aligned", strided(F + 3, 1)), ("ldu odd", strided(F + 3, 0)),
                       ("ldu even, base 8-B aligned", strided(F + 4, 1)), ("ldu > F", strided(F + 4, 0)), ("ldu = F", strided(F, 0)),
                       ("ldu = 2 F", unsplit), ("host", from_host), ("host strided", host_strided),
                       ("host in, device out", host_in_device_out), ("x supplied", x_supplied), ("x 4-B aligned", x_4_byte_aligned)):
        got = two_steps(step)
        for g, b in zip(got, base):
            assert np.array_equal(bits(g), bits(b)), name


# ---------------------------------------------------------------------------------------------------- 9. exact homogeneity
@pytest.mark.parametrize("M", [16, 64, 1024])
def test_power_of_two_scaling_is_exact(tg, M):
    K, F = 5 * M - 2, 40
    f = chan_ref.prototype(M, K)
    u = half_rows(M, F, seed=9)
    x = R.fresh_run(tg, f, M, dev(u), [F])
    for k in (np.float32(128.0), np.float32(2.0 ** -9)):
        x2 = R.fresh_run(tg, f, M, dev(u * k), [F])
        assert np.array_equal(bits(x * k), bits(x2))


# ------------------------------------------------------------------------------------------------------ 10. non-finite horizon
@pytest.mark.parametrize("what", [np.nan, np.inf])
@pytest.mark.parametrize("c", [0, 5, 16, 27, 32])                        # the lone pairs (0 with M / 2; M / 4) and both rows of a pair
def test_non_finite_horizon(tg, what, c):
    M, F = 64, 40
    K = 4 * M - 3                                                       # P = 4: positions 61 .. 63 meet a zero-padded tap
    f = chan_ref.prototype(M, K)
    u = half_rows(M, F, seed=10)
    clean = R.fresh_run(tg, f, M, dev(u), [F]).reshape(F, M)
    keep = np.r_[0:9, 13:F]
    ub = u.copy()
    ub[c, 9] = complex(what, what)
    x = R.fresh_run(tg, f, M, dev(ub), [F]).reshape(F, M)
    assert not np.isfinite(x[9:13]).any()                               # every sample of frames 9 .. 12, positions 61 .. 63 too
    assert np.array_equal(bits(x[keep]), bits(clean[keep]))
    # one part alone: no sample outside the frames either.  (Row M / 4 meets the exact factors i^p: its real part feeds the even
    # positions only, its imaginary part the odd ones, so half a frame stays finite there.)
    ub[c, 9] = complex(what, 1.0)
    x = R.fresh_run(tg, f, M, dev(ub), [F]).reshape(F, M)
    assert not np.isfinite(x[9:13, 0::2]).any()
    assert c == M // 4 or not np.isfinite(x[9:13]).any()
    assert np.array_equal(bits(x[keep]), bits(clean[keep]))


# --------------------------------------------------------------------------------------------------------------- 11. errors
def test_step_errors_leave_the_stream_untouched(tg):
    import torch
    M, K, F = 64, 4 * 64 - 3, 10
    C = M // 2 + 1
    f = chan_ref.prototype(M, K)
    ud = dev(half_rows(M, 3 * F, seed=9))
    a, b = tg.RealSynthesizer(f, M), tg.RealSynthesizer(f, M)
    a.step(ud[:, :F])
    b.step(ud[:, :F])
    seg = ud[:, F:2 * F].contiguous()
    with pytest.raises(tg.TsdGpuError, match="status 1"):              # x_capacity too small, counted in floats
        a.step(seg, torch.empty(F * M - 1, dtype=torch.float32, device="cuda"))
    # u and x share addresses: the end of x in the first sample of row 0 (8 bytes), the start of x in the last sample of row M / 2 (4)
    flat = torch.zeros(F * M + 2 * C * F, dtype=torch.float32, device="cuda")

    def rows_at(o):
        return torch.view_as_complex(flat[o:o + 2 * C * F].view(-1, 2)).view(C, F)
    for xo, uo in ((0, F * M - 2), (2 * C * F - 1, 0)):
        rows_at(uo)[:] = seg
        with pytest.raises(tg.TsdGpuError, match="status 1"):
            a.step(rows_at(uo), flat[xo:xo + F * M])
        assert "overlap" in tg.lib().tsdgpu_last_error().decode()
    with pytest.raises(tg.TsdGpuError, match="row stride"):            # ldu below a row's inputs: the Python layer's check
        a.step(torch.as_strided(torch.empty(C * F, dtype=torch.complex64, device="cuda"), (C, F), (F - 1, 1)))
    xbuf, got = torch.empty(F * M, dtype=torch.float32, device="cuda"), ctypes.c_int64(-1)
    rc = tg.lib().tsdgpu_synthesizer_step(a._h, seg.data_ptr(), F - 1, F, xbuf.data_ptr(), F * M, ctypes.byref(got), None)
    assert rc == 1 and got.value == 0 and "ldu" in tg.lib().tsdgpu_last_error().decode()     # the C ABI's check
    with pytest.raises(tg.TsdGpuError, match="complex64"):             # float rows
        a.step(seg.real.contiguous())
    with pytest.raises(tg.TsdGpuError, match="complex64"):             # a 1-D block
        a.step(seg.reshape(-1))
    with pytest.raises(tg.TsdGpuError, match="float32"):               # a complex x
        a.step(seg, torch.empty(F * M, dtype=torch.complex64, device="cuda"))
    with pytest.raises(tg.TsdGpuError, match="rows"):                  # M rows, as for the complex bank
        a.step(torch.zeros((M, F), dtype=torch.complex64, device="cuda"))
    assert a.step(ud[:, :0]).shape == (0,)                              # frames = 0: a no-op
    # an x that starts where the rows end, and rows that start where the 4-B samples of x end, are no overlap
    rows_at(F * M)[:] = seg
    xa, xb = host(a.step(rows_at(F * M), flat[:F * M])), host(b.step(seg))
    assert np.array_equal(bits(xa), bits(xb))


def test_create_errors(tg):
    def fails(channels, K, status, *words, oversample=1):
        with pytest.raises(tg.TsdGpuError, match=f"status {status}"):
            tg.RealSynthesizer(np.ones(K, np.float32), channels, oversample=oversample)
        msg = tg.lib().tsdgpu_last_error().decode()
        for w in words:
            assert w in msg, msg
    fails(8, 16, 3, "16", "1024")              # UNSUPPORTED, with the limit
    fails(48, 96, 3, "16", "1024")
    fails(2048, 2048, 3, "16", "1024")         # two positions per thread: not served
    fails(64, 16 * 64 + 1, 3, "16")
    fails(64, 128, 3, "oversample", oversample=2)
    fails(64, 128, 1, oversample=0)            # INVALID
    fails(64, 0, 1)                            # null taps
    fails(0, 8, 1)
    raw = ctypes.c_void_p()
    assert tg.lib().tsdgpu_synthesizer_create_real(ctypes.byref(raw), 64, 1, None, 128) == 1 and not raw.value
    sy = tg.RealSynthesizer(np.ones(16 * 64, np.float32), 64)           # the handle after the refusals is usable
    assert sy.step(dev(np.ones((33, 1), np.complex64))).shape == (64,)
    sy.close()


# ------------------------------------------------------------------------------------------------------- 13. round trips
@pytest.mark.parametrize("M", [16, 256])
def test_round_trip_through_the_real_channelizer(tg, M):
    """K = M: one tap per branch both ways, x^[q M + s] = M f[s] h[M - 1 - s] x[q M + s] (tests/test_rsynthesizer_cpu.py)"""
    rng = np.random.default_rng(M + 2)
    F = 40
    x = rng.standard_normal(F * M).astype(np.float32)
    h = (0.5 + rng.random(M)).astype(np.float32)
    f = (0.5 + rng.random(M)).astype(np.float32)
    yd = tg.RealChannelizer(h, M).step(dev(x))
    assert tuple(yd.shape) == (M // 2 + 1, F) and yd.is_cuda
    back = host(tg.RealSynthesizer(f, M).step(yd))
    want = ((M * f.astype(np.float64) * h[::-1].astype(np.float64))[None, :] * x.reshape(F, M)).reshape(-1)
    assert np.abs(back - want).max() <= TOL * np.abs(want).max()


def test_round_trip_through_a_bank(tg):
    """RealChannelizer -> FirBank over the 33 rows -> RealSynthesizer, nothing leaving the device, against the float64 composition"""
    M, K, F = 64, 8 * 64, 200
    C = M // 2 + 1
    h = chan_ref.prototype(M, K)
    x = rchan_ref.stream(F * M, M, seed=12)
    h2 = (np.random.default_rng(13).standard_normal(31) / 8).astype(np.float32)
    yd = tg.RealChannelizer(h, M).step(dev(x))
    zd = tg.FirBank(h2, tg.C64, C).step(yd)
    assert tuple(zd.shape) == (C, F) and zd.is_cuda
    back = host(tg.RealSynthesizer(h, M).step(zd))
    ref = rchan_ref.polyphase64(x, h, M)
    fir_ref = np.stack([np.convolve(r, h2.astype(np.float64))[:F] for r in ref])
    want = R.synth64(fir_ref, h)
    assert back.shape == (F * M,) and back.dtype == np.float32
    assert R.rel_err(back, want) <= TOL
