"""Oversampled real-output polyphase synthesizer (include/tsdgpu.h: tsdgpu_synthesizer_create_real_oversampled;
synthesizer_real_os.hip) through the C ABI via RealSynthesizer.oversampled, against the float64 references of tests/rsyn_os_ref.py:
the definition from a non-zero history and phase, parity over every first radix of the M / 2-point transform, both sides of
D = 128 and the tap counts around the hop, the complex oversampled Synthesizer on the extended block, the imaginary parts of rows 0
and M / 2 that are not used, chunk invariance with the phase checked after every step, state + phase to a fresh handle bit for bit,
OS = 1 against the plain real bank, the per-sample float64 bound at every Q (shown to discriminate, without a GPU, by
tests/test_rsynthesizer_os_cpu.py), long steps, layouts, exact homogeneity, the non-finite horizon, the argument checks, the chains
RealChannelizer.oversampled -> (banks) -> RealSynthesizer.oversampled on the device, and the order of the caller's stream.

Parity inputs: rows 0 .. M / 2 of syn_ref.rows (complex normal rows plus a constant 1e3 in row 3); prototype: Hann-windowed sinc of
cutoff 1 / M.  Bar: max |x - ref| <= 1e-5 max |ref| over the step.  Per-sample inputs: rows 0 .. M / 2 of poly_f64.syn_input,
standard normal taps; bar: worst err / bound <= 1, poly_f64.syn's bound on the extended block at that OS with M the real frame
length, no constant added.

Every case of a grid runs inside one test function (`cases` below collects the cases that miss and the test fails with the whole
list): the grids here are some 600 cases, and the suite keeps the number of collected GPU tests small."""
import ctypes
import functools

import numpy as np
import pytest

import chan_ref
import poly_f64 as PF
import rchan_os_ref
import rchan_ref
import rsyn_os_ref as RO
import stream_order as so
import syn_ref
from rsyn_os_ref import bits, dev, host, run

pytestmark = pytest.mark.gpu
TOL = 1e-5
MS = (16, 32, 64, 128, 256, 512, 1024)
OSS = (2, 4)
FRAMES = 300


@pytest.fixture(scope="module")
def tg():
    import libtsd_amd as t
    assert t.device_count() >= 1
    return t


def make(tg, f, M, OS):
    return tg.RealSynthesizer.oversampled(f, M, OS)


class cases:
    """with cases() as c: ... c.check(ok, label) for every case of a grid; leaving the block fails with every label that missed"""

    def __enter__(self):
        self.bad, self.n = [], 0
        return self

    def check(self, ok, label):
        self.n += 1
        if not ok:
            self.bad.append(label)

    def __exit__(self, et, ev, tb):
        if et is None:
            assert self.n > 0 and not self.bad, f"{len(self.bad)} of {self.n} cases missed: {self.bad}"
        return False


def grid(*axes):
    import itertools
    return itertools.product(*axes)


def half_rows(M, F, seed):
    return np.ascontiguousarray(syn_ref.rows(M, F, seed)[: M // 2 + 1])


# --------------------------------------------------------------------------------------------------------- 1. definition
def test_small_case_against_the_definition(tg):
    for OS in OSS:
        _small_case(tg, OS)


def _small_case(tg, OS):
    M, F, F0 = 16, 9, 3
    D, C = M // OS, M // 2 + 1
    K = 2 * D + 3
    Q = -(-K // D)
    f = chan_ref.prototype(M, K)
    u = half_rows(M, F0 + F, seed=3)
    sy = make(tg, f, M, OS)
    assert (sy.rows, sy.hop, sy.history_len, sy.frames_kept, sy.oversample, sy.phase) == (C, D, (Q - 1) * C, Q - 1, OS, 0)
    L = tg.lib()
    assert L.tsdgpu_synthesizer_is_real(sy._h) == 1 and L.tsdgpu_synthesizer_rows(sy._h) == C
    assert L.tsdgpu_synthesizer_hop(sy._h) == D and sy.out_count(F) == F * D
    ud = dev(u)
    sy.step(ud[:, :F0])                                                 # an odd number of hops: a history and a phase
    assert sy.phase == F0 % OS
    x = host(sy.step(ud[:, F0:]))
    assert x.shape == (F * D,) and x.dtype == np.float32
    hist = np.concatenate([np.zeros((C, Q - 1), np.complex64), u[:, :F0]], axis=1)[:, -(Q - 1):]
    assert hist.any()
    assert RO.rel_err(x, RO.definition(u[:, F0:], f, M, OS, F0, hist)) <= TOL


# ------------------------------------------------------------------------------------------------------------- 2. parity
@functools.lru_cache(maxsize=None)
def parity_rows(M, F):
    u = half_rows(M, 2 * F, seed=M + F)
    return u, dev(u)


def test_parity_two_steps(tg):
    """M x OS x K in {1, D - 3, 4 D, 16 D - 5} x F in {1, 15, 16, 17, 50}: every first radix; M = 128 / OS = 2 and M = 256 / OS = 4
    (D = 64) and below diverge in the ownership test, M = 256 / OS = 2 (D = 128) and above are wave-uniform"""
    worst = 0.0
    with cases() as c:
        for M, OS, kk, F in grid(MS, OSS, ["1", "D-3", "4D", "16D-5"], [1, 15, 16, 17, 50]):
            err = _parity(tg, M, OS, kk, F)
            worst = max(worst, err)
            c.check(err <= TOL, (M, OS, kk, F, err))
    print(f"parity, worst of {c.n} cases: {worst:.2e}")
    assert c.n == 280


def _parity(tg, M, OS, kk, F):
    D = M // OS
    K = {"1": 1, "D-3": D - 3, "4D": 4 * D, "16D-5": 16 * D - 5}[kk]
    f = chan_ref.prototype(M, K)
    u, ud = parity_rows(M, F)
    ref = RO.synth64(u, f, M, OS)
    sy = make(tg, f, M, OS)
    assert sy.hop == D and sy.out_count(F) == F * D
    x = run(sy, ud, [F, F])                      # the second step starts from real history and, for odd F, a non-zero phase
    assert x.shape == (2 * F * D,)
    err = RO.rel_err(x, ref)
    print(f"M={M} OS={OS} K={K} F={F}: {err:.2e}")
    return err


# ------------------------------------------------------------------- 3. the complex bank, 4. the parts that are not used
def test_agrees_with_the_complex_synthesizer_on_the_extended_block(tg):
    """two float32 results, each held to 1e-5 of float64: 2e-5 of the peak between them; every M x OS"""
    with cases() as c:
        for M, OS in grid(MS, OSS):
            er, ei = _against_complex(tg, M, OS)
            print(f"M={M} OS={OS}: real part {er:.2e}, imaginary part {ei:.2e} of the peak")
            c.check(er <= 2 * TOL and ei <= 2 * TOL, (M, OS, er, ei))
    assert c.n == 14


def _against_complex(tg, M, OS):
    D = M // OS
    K, F = 4 * D - 3, 33
    f = chan_ref.prototype(M, K)
    u = half_rows(M, F, seed=4)
    x = RO.fresh_run(tg, f, M, OS, dev(u), [F])
    xc = host(tg.Synthesizer(f, M, oversample=OS).step(dev(RO.extend(u))))
    peak = np.abs(x).max()
    return np.abs(xc.real.astype(np.float64) - x).max() / peak, np.abs(xc.imag).max() / peak


def test_imaginary_parts_of_rows_0_and_nyquist_are_not_used(tg):
    for M, OS in grid(MS, OSS):
        _unused_parts(tg, M, OS)


def _unused_parts(tg, M, OS):
    D = M // OS
    K, F = 3 * D + 1, 37
    N = M // 2
    f = chan_ref.prototype(M, K)
    u = half_rows(M, F, seed=5)
    assert u[0].imag.any() and u[N].imag.any()
    base = RO.fresh_run(tg, f, M, OS, dev(u), [19, 18])
    rng = np.random.default_rng(M + OS)
    for what in ("zero", "garbage", "nan"):
        v = u.copy()
        for c in (0, N):
            v[c].imag = {"zero": 0.0, "garbage": 1e30 * rng.standard_normal(F), "nan": np.nan}[what]
        got = RO.fresh_run(tg, f, M, OS, dev(v), [19, 18])               # the second step reads them from the history too
        assert np.array_equal(bits(got), bits(base)), (M, OS, what)
    v = u.copy()
    v[1].imag += 1.0                                                     # (a part that IS used shows)
    assert not np.array_equal(bits(RO.fresh_run(tg, f, M, OS, dev(v), [19, 18])), bits(base)), (M, OS)


# ----------------------------------------------------------------------------------- 5. chunk invariance and state, bit for bit
def test_chunk_invariance_bit_for_bit(tg):
    for M, OS, kk in grid([16, 64, 1024], OSS, ["D+1", "16D"]):
        _chunks(tg, M, OS, kk)


def _chunks(tg, M, OS, kk):
    D = M // OS
    K = D + 1 if kk == "D+1" else 16 * D
    f = chan_ref.prototype(M, K)
    F = 150
    ud = dev(half_rows(M, F, seed=6))
    one = RO.fresh_run(tg, f, M, OS, ud, [F])
    steps = PF.ragged(np.random.default_rng([5, M, OS, K]), F)
    assert len(steps) > 2 and any(s % 2 for s in steps)
    many = RO.fresh_run(tg, f, M, OS, ud, steps)                        # (run() checks the phase after every step)
    assert np.array_equal(bits(one), bits(many)), (M, OS, kk)


def test_state_and_phase_move_to_a_fresh_handle(tg):
    for M, OS, K in [(16, 4, 16 * 4), (64, 2, 4 * 64 - 3), (1024, 2, 1025), (64, 4, 65), (256, 2, 3 * 128 + 1)]:
        _state_and_phase(tg, M, OS, K)


def _state_and_phase(tg, M, OS, K):
    import torch
    D, C = M // OS, M // 2 + 1
    f = chan_ref.prototype(M, K)
    QW = -(-K // D) - 1
    u = half_rows(M, 60, seed=6)
    ud = dev(u)
    a = make(tg, f, M, OS)
    assert a.history_len == QW * C and a.frames_kept == QW and a.phase == 0
    a.step(ud[:, :23])                                                   # 23 frames: odd
    assert a.phase == 23 % OS
    st = a.get_state()
    assert st.shape == (C, QW) and st.dtype == np.complex64
    want = np.concatenate([np.zeros((C, QW), np.complex64), u[:, :23]], axis=1)[:, -QW:]
    assert np.array_equal(bits(st), bits(want))                         # the last Q - 1 input frames as they were fed
    b, nophase = make(tg, f, M, OS), make(tg, f, M, OS)
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
    sd = torch.empty((C, QW), dtype=torch.complex64, device="cuda")
    a.get_state(sd)
    c = make(tg, f, M, OS)
    c.set_state(sd)
    c.phase = a.phase
    a.step(ud[:, :1])                                                    # leave a on a non-zero phase before the reset
    a.reset()
    assert a.phase == 0
    fresh = host(make(tg, f, M, OS).step(ud[:, :17]))
    assert np.array_equal(bits(host(a.step(ud[:, :17]))), bits(fresh))
    xc, xb2 = host(c.step(ud[:, :17])), host(b.step(ud[:, :17]))
    assert np.array_equal(bits(xc), bits(xb2))


# -------------------------------------------------------------------------------------------------------------- 7. OS = 1
def test_oversample_one_is_the_plain_real_bank(tg):
    """one shape per first radix of the M / 2-point transform (dft8; 16, 2, 4; 2 at N = 512)"""
    for M, K in [(16, 33), (32, 3 * 32), (64, 65), (128, 2 * 128), (1024, 1025)]:
        _oversample_one(tg, M, K)


def _oversample_one(tg, M, K):
    f = chan_ref.prototype(M, K)
    ud = dev(half_rows(M, 37, seed=7))
    a, b = tg.RealSynthesizer(f, M), make(tg, f, M, 1)
    assert (b.hop, b.rows, b.history_len, b.frames_kept, b.phase) == (M, a.rows, a.history_len, a.frames_kept, 0)
    xa, xb = run(a, ud, [20, 17]), run(b, ud, [20, 17])
    assert xa.shape == (37 * M,)
    assert np.array_equal(bits(xa), bits(xb)), M
    assert b.phase == 0


# ----------------------------------------------------------------------------------------------- 8. per-sample float64 sweep
@functools.lru_cache(maxsize=None)
def f64_data(M, frames=FRAMES):
    u = RO.input(np.random.default_rng([1, M, frames]), M, frames)
    return u, dev(u)


def run_and_judge(tg, M, OS, f, data, steps, what):
    u, ud = data
    x64, bound = RO.f64_case(u, f, M, OS)
    x = RO.fresh_run(tg, f, M, OS, ud, steps)
    return PF.syn_judge(x, x64, bound, what), x


def test_tap_row_sweep(tg):
    """every M x OS x Q = 1 .. 16, Q the kernel's template argument.  Two tap counts each: inside the last row (zero-padded taps), and the
    row full; ragged steps, odd ones among them.  Samples whose bound is 0 must come out exactly 0 (syn_judge)."""
    worst = 0.0
    with cases() as c:
        for M, OS, Q in grid(MS, OSS, range(1, 17)):
            rng = np.random.default_rng([3, M, OS, Q])
            for K in rchan_ref.two_tap_counts(rng, M // OS, Q):
                f = PF.taps(rng, K)
                what = f"rsyn_os M={M} OS={OS} Q={Q} K={K}"
                ratio, _ = run_and_judge(tg, M, OS, f, f64_data(M), PF.ragged(rng, FRAMES), what)
                print(f"{what}: worst err / bound {ratio:.3f}")
                worst = max(worst, ratio)
                c.check(ratio <= 1.0, (what, ratio))
    print(f"worst err / bound of {c.n} cases {worst:.3f}")
    assert c.n == 448


@pytest.mark.parametrize("OS,Q", [(2, 3), (4, 16)])
def test_long_step_third_iteration(tg, OS, Q):
    """M in {16, 128, 1024}.  F = 2 x 16 x R x grid + 17 frames (R = 512 / (M / 2) sub-runs of the M / 2-point tile, grid = 2 CUs): 2 R grid + 2 units,
    so every sub-run takes per = 3 units of the persistent loop.  Then the same rows in three odd-cut steps: the same bits."""
    for M in (16, 128, 1024):
        _long_step(tg, M, OS, Q)


def _long_step(tg, M, OS, Q):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    subruns = (1024 // M) * 2 * cus
    F = 2 * 16 * subruns + 17
    assert -(-(-(-F // 16)) // subruns) == 3                            # ceil(ceil(F / 16) / subruns)
    rng = np.random.default_rng([4, M, OS, Q])
    K = rchan_ref.two_tap_counts(rng, M // OS, Q)[0]
    f = PF.taps(rng, K)
    data = f64_data(M, F)
    what = f"rsyn_os M={M} OS={OS} Q={Q} K={K} F={F}"
    ratio, one = run_and_judge(tg, M, OS, f, data, [F], what)
    print(f"{what}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0, what
    a, b = sorted(int(v) for v in rng.choice(np.arange(1, F, 2), 2, replace=False))
    three = RO.fresh_run(tg, f, M, OS, data[1], [a, b - a, F - b])
    assert np.array_equal(bits(one), bits(three)), what
    f64_data.cache_clear()                                              # tens of MB a side: not kept for the session


# ------------------------------------------------------------------------------------------ 9. many tiles and workgroups
def test_many_tiles_and_workgroups(tg):
    for M, OS, F in [(16, 4, 40000), (1024, 2, 600)]:
        K = 8 * (M // OS)
        f = chan_ref.prototype(M, K)
        u = half_rows(M, F, seed=11)
        x = RO.fresh_run(tg, f, M, OS, dev(u), [F])
        err = RO.rel_err(x, RO.synth64(u, f, M, OS))
        print(f"M={M} OS={OS} F={F}: {err:.2e}")
        assert err <= TOL, (M, OS, F)


# ------------------------------------------------------------------------------------------------------------- 10. layouts
def test_layouts_give_the_same_bits(tg):
    """(16, 4): D = 4, the shortest hop, two pairs to a hop; M = 256: D = 128 wave-uniform and D = 64 diverging"""
    for M, OS, K in [(16, 4, 4 * 16 - 3), (256, 2, 257), (256, 4, 129)]:
        _layouts(tg, M, OS, K)


def _layouts(tg, M, OS, K):
    import torch
    F, C, D = 21, M // 2 + 1, M // OS                                   # F odd: the second step from a non-zero phase
    f = chan_ref.prototype(M, K)
    u = half_rows(M, 2 * F, seed=8)
    ud = dev(u)

    def two_steps(step):
        sy = make(tg, f, M, OS)
        return [step(sy, 0), step(sy, 1)]

    def seg(v, i):
        return v[:, i * F:(i + 1) * F]

    base = two_steps(lambda sy, i: host(sy.step(seg(ud, i).contiguous())).copy())
    assert RO.rel_err(np.concatenate(base), RO.synth64(u, f, M, OS)) <= TOL

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
        assert isinstance(x, np.ndarray) and x.dtype == np.float32 and x.shape == (F * D,)
        return x

    def host_strided(sy, i):
        return sy.step(seg(u, i)).copy()

    def host_in_device_out(sy, i):
        buf = torch.empty(F * D, dtype=torch.float32, device="cuda")
        x = sy.step(np.ascontiguousarray(seg(u, i)), buf)
        assert x.data_ptr() == buf.data_ptr()
        return host(x).copy()

    def x_supplied(sy, i):
        buf = torch.full((F * D + 10,), 7.0, dtype=torch.float32, device="cuda")
        x = sy.step(seg(ud, i), buf)
        assert x.data_ptr() == buf.data_ptr() and tuple(x.shape) == (F * D,)
        assert bool((buf[F * D:] == 7.0).all())                          # nothing written past the step
        return host(x).copy()

    def x_4_byte_aligned(sy, i):
        buf = torch.full((F * D + 11,), 7.0, dtype=torch.float32, device="cuda")
        assert buf[1:].data_ptr() % 8 == 4
        x = sy.step(seg(ud, i), buf[1:])
        assert bool((buf[F * D + 1:] == 7.0).all()) and bool(buf[0] == 7.0)
        return host(x).copy()

    for name, step in (("ldu odd, base 8-B aligned", strided(F + 2, 1)), ("ldu odd", strided(F + 2, 0)),
                       ("ldu even, base 8-B aligned", strided(F + 3, 1)), ("ldu > F", strided(F + 3, 0)), ("ldu = F", strided(F, 0)),
                       ("ldu = 2 F", unsplit), ("host", from_host), ("host strided", host_strided),
                       ("host in, device out", host_in_device_out), ("x supplied", x_supplied), ("x 4-B aligned", x_4_byte_aligned)):
        got = two_steps(step)
        for g, b in zip(got, base):
            assert np.array_equal(bits(g), bits(b)), (M, OS, name)


# --------------------------------------------------------------------------------------------------- 11. exact homogeneity
def test_power_of_two_scaling_is_exact(tg):
    for M, OS in grid([16, 64, 1024], OSS):
        K, F = 5 * (M // OS) - 2, 41
        f = chan_ref.prototype(M, K)
        u = half_rows(M, F, seed=9)
        x = RO.fresh_run(tg, f, M, OS, dev(u), [F])
        for k in (np.float32(128.0), np.float32(2.0 ** -9)):
            x2 = RO.fresh_run(tg, f, M, OS, dev(u * k), [F])
            assert np.array_equal(bits(x * k), bits(x2)), (M, OS, k)


# ------------------------------------------------------------------------------------------------------ 12. non-finite horizon
def test_non_finite_horizon(tg):
    """rows c in {0, 5, M / 4, M / 2} (the lone pairs and a row of a pair) x NaN, Inf x OS:
    a NaN / Inf in input frame m of a row reaches output hops m .. m + Q - 1 only; everything else keeps the clean run's bits.
    Within those hops: both parts non-finite make every float non-finite, the floats that meet a zero-padded tap included; the real
    part alone still reaches every even float (and every float unless the row is M / 4: that row meets the exact factors i^p, so
    its real part feeds the even positions only and its imaginary part the odd ones, and half of the floats stay finite)."""
    for OS, c, what in grid(OSS, [0, 5, 16, 32], [np.nan, np.inf]):
        _horizon(tg, OS, what, c)


def _horizon(tg, OS, what, c):
    M, F = 64, 40
    D = M // OS
    K = 4 * D - 3                                                       # Q = 4: the last floats of a hop meet a zero-padded tap
    Q = -(-K // D)
    f = chan_ref.prototype(M, K)
    u = half_rows(M, F, seed=10)
    clean = RO.fresh_run(tg, f, M, OS, dev(u), [F]).reshape(F, D)
    keep = np.r_[0:9, 9 + Q:F]
    ub = u.copy()
    ub[c, 9] = complex(what, what)
    x = RO.fresh_run(tg, f, M, OS, dev(ub), [F]).reshape(F, D)
    assert not np.isfinite(x[9:9 + Q]).any()
    assert np.array_equal(bits(x[keep]), bits(clean[keep]))
    ub[c, 9] = complex(what, 1.0)
    x = RO.fresh_run(tg, f, M, OS, dev(ub), [F]).reshape(F, D)
    assert not np.isfinite(x[9:9 + Q, 0::2]).any()                      # (D is even: even floats of a hop are even positions)
    odd_finite = int(np.isfinite(x[9:9 + Q, 1::2]).sum())
    print(f"OS={OS} c={c} {what}: {odd_finite} of {Q * D // 2} odd floats of hops 9 .. {9 + Q - 1} finite")
    if c == M // 4:
        assert odd_finite == Q * D // 2
    else:
        assert odd_finite == 0
    assert np.array_equal(bits(x[keep]), bits(clean[keep]))


# --------------------------------------------------------------------------------------------------------------- 13. errors
def test_step_errors_leave_history_and_phase_untouched(tg):
    import torch
    M, OS, F = 64, 2, 11                                                # F odd: the failing steps meet a non-zero phase
    D, C = M // OS, M // 2 + 1
    K, n = 4 * M - 3, F * D
    f = chan_ref.prototype(M, K)
    ud = dev(half_rows(M, 3 * F, seed=9))
    a, b = make(tg, f, M, OS), make(tg, f, M, OS)
    a.step(ud[:, :F])
    b.step(ud[:, :F])
    assert a.phase == b.phase == F % OS
    seg = ud[:, F:2 * F].contiguous()
    with pytest.raises(tg.TsdGpuError, match="status 1"):              # x_capacity below F D, counted in floats
        a.step(seg, torch.empty(n - 1, dtype=torch.float32, device="cuda"))
    # u and x share addresses: the end of x in the first sample of row 0 (8 bytes), the start of x in the last sample of row M / 2 (4)
    flat = torch.zeros(n + 2 * C * F, dtype=torch.float32, device="cuda")

    def rows_at(o):
        return torch.view_as_complex(flat[o:o + 2 * C * F].view(-1, 2)).view(C, F)
    for xo, uo in ((0, n - 2), (2 * C * F - 1, 0)):
        rows_at(uo)[:] = seg
        with pytest.raises(tg.TsdGpuError, match="status 1"):
            a.step(rows_at(uo), flat[xo:xo + n])
        assert "overlap" in tg.lib().tsdgpu_last_error().decode()
    with pytest.raises(tg.TsdGpuError, match="row stride"):            # ldu below a row's inputs: the Python layer's check
        a.step(torch.as_strided(torch.empty(C * F, dtype=torch.complex64, device="cuda"), (C, F), (F - 1, 1)))
    xbuf, got = torch.empty(n, dtype=torch.float32, device="cuda"), ctypes.c_int64(-1)
    L = tg.lib()
    rc = L.tsdgpu_synthesizer_step(a._h, seg.data_ptr(), F - 1, F, xbuf.data_ptr(), n, ctypes.byref(got), None)
    assert rc == 1 and got.value == 0 and "ldu" in L.tsdgpu_last_error().decode()     # the C ABI's checks
    rc = L.tsdgpu_synthesizer_step(a._h, seg.data_ptr(), F, F, xbuf.data_ptr(), n - 1, ctypes.byref(got), None)
    assert rc == 1 and got.value == 0 and "x_capacity" in L.tsdgpu_last_error().decode()
    rc = L.tsdgpu_synthesizer_step(a._h, None, F, F, xbuf.data_ptr(), n, ctypes.byref(got), None)
    assert rc == 1 and got.value == 0 and "NULL" in L.tsdgpu_last_error().decode()
    rc = L.tsdgpu_synthesizer_step(a._h, seg.data_ptr(), F, F, None, n, ctypes.byref(got), None)
    assert rc == 1 and got.value == 0 and "NULL" in L.tsdgpu_last_error().decode()
    with pytest.raises(tg.TsdGpuError, match="complex64"):             # float rows
        a.step(seg.real.contiguous())
    with pytest.raises(tg.TsdGpuError, match="float32"):               # a complex x
        a.step(seg, torch.empty(n, dtype=torch.complex64, device="cuda"))
    with pytest.raises(tg.TsdGpuError, match="rows"):                  # M rows, as for the complex bank
        a.step(torch.zeros((M, F), dtype=torch.complex64, device="cuda"))
    assert a.step(ud[:, :0]).shape == (0,)                              # frames = 0: a no-op
    assert a.phase == b.phase == F % OS
    assert np.array_equal(bits(a.get_state()), bits(b.get_state()))
    # an x that starts where the rows end is no overlap; the twins stay in step
    rows_at(n)[:] = seg
    xa, xb = host(a.step(rows_at(n), flat[:n])), host(b.step(seg))
    assert np.array_equal(bits(xa), bits(xb))
    assert a.phase == b.phase == 0
    assert np.array_equal(bits(a.get_state()), bits(b.get_state()))


def test_create_errors(tg):
    def fails(channels, OS, K, status, *words):
        with pytest.raises(tg.TsdGpuError, match=f"status {status}"):
            make(tg, np.ones(K, np.float32), channels, OS)
        msg = tg.lib().tsdgpu_last_error().decode()
        for w in words:
            assert w in msg, msg
    for OS in (1,) + OSS:
        fails(8, OS, 16, 3, "16", "1024")          # UNSUPPORTED, with the limit
        fails(48, OS, 96, 3, "16", "1024")
        fails(2048, OS, 2048, 3, "16", "1024")     # two positions per thread: not served
        fails(64, OS, 16 * (64 // OS) + 1, 3, "16", str(16 * (64 // OS)))
        fails(64, OS, 0, 1)                        # no taps: INVALID
        fails(0, OS, 8, 1)
    fails(64, 3, 64, 3, "oversample", "1, 2 and 4")
    fails(64, 8, 64, 3, "oversample", "1, 2 and 4")
    fails(64, 0, 64, 1)
    fails(64, -2, 64, 1)
    L, raw = tg.lib(), ctypes.c_void_p()
    assert L.tsdgpu_synthesizer_create_real_oversampled(ctypes.byref(raw), 64, 2, None, 128) == 1 and not raw.value
    assert L.tsdgpu_synthesizer_create_real_oversampled(None, 64, 2, np.ones(8, np.float32).ctypes.data, 8) == 1
    assert "NULL" in L.tsdgpu_last_error().decode()
    # the constructor keeps refusing: the entry it calls serves oversample = 1 only
    with pytest.raises(tg.TsdGpuError, match="status 3"):
        tg.RealSynthesizer(np.ones(128, np.float32), 64, oversample=2)
    assert "oversample" in L.tsdgpu_last_error().decode()
    for OS in OSS:                                 # the handle after the refusals is usable, at the limit
        sy = make(tg, np.ones(16 * (64 // OS), np.float32), 64, OS)
        assert sy.step(dev(np.ones((33, 1), np.complex64))).shape == (64 // OS,)
        sy.close()


# ------------------------------------------------------------------------- 15. on the device, no copy and no conjugate rows
def test_round_trip_on_the_device(tg):
    """M in {16, 256} x OS.  RealChannelizer.oversampled(h, M, OS) writes its rows into columns 1 .. of a block whose column 0 is
    zero (the one-frame delay); RealSynthesizer.oversampled(f, M, OS) reads columns 0 .. F - 1 of that block: h the sine window of length M, f = h
    reversed, x comes back as (M OS / 2) x[p - M].  2e-5 of the peak past the first 2 M samples, the two stages' bars added."""
    for M, OS in grid([16, 256], OSS):
        _round_trip(tg, M, OS)


def _round_trip(tg, M, OS):
    import torch
    F, D, C = 200, M // OS, M // 2 + 1
    h = np.sin(np.pi * (np.arange(M) + 0.5) / M).astype(np.float32)
    f = np.ascontiguousarray(h[::-1])
    x = np.random.default_rng(100 + M + OS).standard_normal(F * D).astype(np.float32)         # unit variance
    buf = torch.zeros((C, F + 1), dtype=torch.complex64, device="cuda")
    yd = tg.RealChannelizer.oversampled(h, M, OS).step(dev(x), buf[:, 1:])
    assert yd.data_ptr() == buf[:, 1:].data_ptr() and tuple(yd.shape) == (C, F)
    out = make(tg, f, M, OS).step(buf[:, :F])
    assert out.is_cuda and tuple(out.shape) == (F * D,) and out.dtype == torch.float32
    got = host(out)
    want = (M * OS / 2) * np.concatenate([np.zeros(M), x.astype(np.float64)])[:F * D]
    err = np.abs(got - want)[2 * M:].max() / np.abs(want).max()
    print(f"M={M} OS={OS}: round trip {err:.2e} of the peak")
    assert err <= 2e-5, (M, OS)


def test_banks_in_between(tg):
    """RealChannelizer.oversampled(h, 64, 2) -> FirBank over the 33 rows -> RealSynthesizer.oversampled, nothing leaving the device,
    against the float64 composition at 2e-5 of the peak"""
    M, OS, F = 64, 2, 200
    C, D = M // 2 + 1, M // OS
    K = 8 * D
    h = chan_ref.prototype(M, K)
    x = rchan_ref.stream(F * D, M, seed=12)
    h2 = (np.random.default_rng(13).standard_normal(31) / 8).astype(np.float32)
    yd = tg.RealChannelizer.oversampled(h, M, OS).step(dev(x))
    zd = tg.FirBank(h2, tg.C64, C).step(yd)
    assert tuple(zd.shape) == (C, F) and zd.is_cuda
    out = make(tg, h, M, OS).step(zd)
    assert out.is_cuda and tuple(out.shape) == (F * D,)
    y64 = rchan_os_ref.polyphase64(x, h, M, OS)
    z64 = np.stack([np.convolve(r, h2.astype(np.float64))[:F] for r in y64])
    err = RO.rel_err(host(out), RO.synth64(z64, h, M, OS))
    print(f"real channelizer -> FirBank -> real synthesizer at OS = 2 against the float64 composition: {err:.2e}")
    assert err <= 2e-5


# --------------------------------------------------------------------------------------------------------- 16. stream order
def _stream_ops(t):
    ops = []
    for M in (16, 64):
        h4, hop = so.lowpass(4 * M, 0.5 / M), M // 2
        ops.append(so.Op(f"rsynthesizer-M{M}-os2", (lambda M=M, h4=h4: t.RealSynthesizer.oversampled(h4, M, 2)),
                         [so.rand2(M // 2 + 1, n // hop, True, 230 + n) for n in so._ragged(hop)], so._step,
                         (lambda u, hop=hop: ((u.shape[1] * hop,), np.float32)), "tsdgpu_synthesizer_step", lambda h: h.reset()))
    return ops


@pytest.fixture(scope="module")
def delay(tg):
    d = so.Delay()
    assert d.ms >= so.MIN_MS, f"the device-side delay reached {d.ms:.1f} ms only"
    return d


@pytest.fixture(scope="module")
def side(tg):
    import torch
    return torch.cuda.Stream(), torch.cuda.Stream()


def test_stream_order(tg, delay, side):
    """the two Ops "rsynthesizer-M{16,64}-os2": one side stream; a hand-over between two streams; state and phase moved to a fresh
    handle on a second stream: bit for bit against the synchronised run on the default stream, and asynchronous, as the contract
    lists tsdgpu_synthesizer_step"""
    ops = _stream_ops(tg)
    assert [o.name for o in ops] == ["rsynthesizer-M16-os2", "rsynthesizer-M64-os2"]
    for op in ops:
        _stream_scenarios(op, delay, side)


def _stream_scenarios(op, delay, side):
    import torch
    assert op.expect_async and so.CONTRACT["tsdgpu_synthesizer_get_state"] == so.ASYNC
    want = so.reference(op, True)
    r, got = so.under_test(op, [side[0]] * len(op.xs), delay, True)
    so.check(f"A {op.name}", want, got, r.pending, delay, True)
    r, got = so.under_test(op, [side[0]] + [side[1]] * (len(op.xs) - 1), delay, True)
    so.check(f"B {op.name}", want, got, r.pending, delay, True)
    # F: step 1 on handle a (s1), its history into a device buffer on s1 and its phase, an event, both into the fresh handle b on
    # s2, steps 2 and 3 on b
    s1, s2 = side
    a, b = op.make(), op.make()
    so.warm(op, a)
    so.warm(op, b)
    st_dev = so.alloc((a.rows, a.frames_kept), np.complex64, "plain", so.POISON_X)
    r = so.Run(op)
    r.extra += [a, b, st_dev]
    r.head(s1, delay)
    r.step(a, 0, s1)
    with torch.cuda.stream(s1):
        a.get_state(st_dev, stream=s1.cuda_stream)
        phase = a.phase
        r.note()
    assert phase == op.xs[0].shape[1] % 2
    r.hand_over(s1, s2)
    with torch.cuda.stream(s2):
        b.set_state(st_dev, stream=s2.cuda_stream)
        b.phase = phase
        r.note()
    r.step(b, 1, s2)
    r.step(b, 2, s2)
    s1.synchronize()
    s2.synchronize()
    so.check(f"F {op.name} against the uninterrupted stream", want, r.results(), r.pending, delay, True)
