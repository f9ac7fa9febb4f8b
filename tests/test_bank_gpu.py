"""Channel banks (include/tsdgpu.h: tsdgpu_fir_bank / tsdgpu_sos_bank): every channel against its own single-stream handle
fed the same blocks -- bit-identical for the FIR, within 1e-5 of the peak and per window against float64 for the SOS chain --
plus layouts (strides, misaligned rows, in place, host arrays), state interchange, channel isolation, many channels, channel
offsets past 2^31 elements and the argument checks."""
import ctypes

import numpy as np
import pytest

import f64ref as R

pytestmark = pytest.mark.gpu
KINDS = {"f32": ("F32", False), "c64_rtaps": ("C64", False), "c64_ctaps": ("C64", True)}


@pytest.fixture(scope="module")
def tg():
    import libtsd_amd as t
    assert t.device_count() >= 1
    return t


def bits(a):
    """bit pattern of a device tensor (NaN-safe exact comparison)"""
    import torch
    if a.is_complex():
        a = torch.view_as_real(a)
    return a.contiguous().view(torch.int32)


def same_bits(a, b):
    import torch
    return torch.equal(bits(a), bits(b))


def rand_dev(rng, shape, cplx, scale=1.0):
    import torch
    x = rng.standard_normal(shape)
    if cplx:
        x = x + 1j * rng.standard_normal(shape)
    return torch.from_numpy((scale * x).astype(np.complex64 if cplx else np.float32)).cuda()


# ------------------------------------------------------------------------------------------------------------ FIR
@pytest.mark.parametrize("C", [1, 3, 257])
@pytest.mark.parametrize("K", [1, 2, 31, 127, 1000])
@pytest.mark.parametrize("kind", list(KINDS))
def test_fir_bank_bit_identical_to_direct_handles(tg, kind, K, C):
    import torch
    dts, ctaps = KINDS[kind]
    dt, cplx = getattr(tg, dts), dts == "C64"
    rng = np.random.default_rng(K * 7 + C)
    h = rng.standard_normal(K) + (1j * rng.standard_normal(K) if ctaps else 0)
    h = h.astype(np.complex64 if ctaps else np.float32)
    blocks = [1, 7, 4095, 4096, 4097, 65539] if C < 257 else [1, 7, 4096, 4097, 20003]
    bank = tg.FirBank(h, dt, C)
    xs = [rand_dev(rng, (C, n), cplx) for n in blocks]
    ys = [bank.step(x) for x in xs]
    torch.cuda.synchronize()
    for c in range(C):
        f = tg.Fir(h, dt, tg.FIR_DIRECT)
        for x, y in zip(xs, ys):
            ref = f.step(x[c].contiguous())
            assert same_bits(y[c], ref), (kind, K, C, c, x.shape[1])


@pytest.mark.parametrize("cplx,K", [(False, 31), (True, 127)])
def test_fir_bank_oracle_parity(tg, orc, cplx, K):
    rng = np.random.default_rng(K)
    h = orc.design_rif_fen(K, "lp", 0.25)
    C, n = 64, 4096
    x = rand_dev(rng, (C, n), cplx)
    y = tg.FirBank(h, tg.C64 if cplx else tg.F32, C).step(x).cpu().numpy()
    xh = x.cpu().numpy()
    for c in range(C):
        ref = orc.fir(h, xh[c])
        assert np.abs(y[c] - ref).max() <= 1e-5 * np.abs(ref).max(), c


# ------------------------------------------------------------------------------------------------------------ SOS
def sos_design(orc, order, fc, forme):
    z, p, mn, md = orc.design_butter_lp(order, fc)
    return orc.SosChain(z, p, mn, md, forme=forme).coefs()


SOS_CASES = [(12, 0.25, False, 2), (12, 0.25, True, 2), (6, 0.02, False, 2), (5, 0.1, False, 2), (3, 0.05, True, 2),
             (12, 0.25, False, 1), (4, 0.02, True, 1)]        # test_dynamic_range_gpu.SOS_CASES


@pytest.mark.parametrize("order,fc,cplx,forme", SOS_CASES)
def test_sos_bank_against_single_handles_and_float64(tg, orc, order, fc, cplx, forme):
    import torch
    co, gain, r1 = sos_design(orc, order, fc, forme)
    dt = tg.C64 if cplx else tg.F32
    rng = np.random.default_rng(order * 10 + forme + 5 * cplx)
    C = 5
    blocks = [1, 7, 2047, 4096, 4097, 20000, 65539]
    levels = 3.0 * (np.arange(C) + 1) * (np.where(np.arange(C) % 2, -1, 1))     # a different DC level per channel
    xs = [rand_dev(rng, (C, n), cplx) for n in blocks]
    xs[0] += torch.from_numpy(levels.astype(np.float32)).cuda()[:, None].to(xs[0].dtype)
    for x in xs[1:]:
        x += torch.from_numpy(levels.astype(np.float32)).cuda()[:, None].to(x.dtype)
    bank = tg.SosBank(co, gain, dt, C, r1, forme=forme)
    ys = [bank.step(x) for x in xs]
    torch.cuda.synchronize()
    edges = np.cumsum([0] + blocks)
    for c in range(C):
        s = tg.Sos(co, gain, dt, r1, forme=forme)
        yb = np.concatenate([y[c].cpu().numpy() for y in ys])
        ysg = np.concatenate([s.step(x[c].contiguous()).cpu().numpy() for x in xs])
        assert np.abs(yb - ysg).max() <= 1e-5 * np.abs(ysg).max(), c
        xc = np.concatenate([x[c].cpu().numpy() for x in xs])
        y64 = R.sos(co, gain, r1, xc, forme)
        win = R.windows(edges, len(xc))
        eb, mag = R.region_err(yb.astype(np.complex128), y64, win)
        es, _ = R.region_err(ysg.astype(np.complex128), y64, win)
        lim = 5.0 * es + 8 * R.U * mag                   # no further from float64 than C_REC x the single handle
        assert (eb <= lim).all(), (c, [(int(win[i]), eb[i], es[i]) for i in np.nonzero(eb > lim)[0][:4]])


def test_sos_bank_long_blocks_go_through_the_single_stream_step(tg, orc):
    import torch
    co, gain, r1 = sos_design(orc, 12, 0.25, 2)
    rng = np.random.default_rng(3)
    C, n = 2, (1 << 20) + 3
    xs = [rand_dev(rng, (C, m), False) + 1.0 for m in (5, n, 77)]
    bank = tg.SosBank(co, gain, tg.F32, C, r1)
    ys = [bank.step(x) for x in xs]
    torch.cuda.synchronize()
    for c in range(C):
        s = tg.Sos(co, gain, tg.F32, r1)
        for x, y in zip(xs, ys):
            ref = s.step(x[c].contiguous())
            assert (y[c] - ref).abs().max().item() <= 1e-5 * ref.abs().max().item(), (c, x.shape)


# ------------------------------------------------------------------------------------------------ layouts
def _banks(tg, orc, cplx):
    dt = tg.C64 if cplx else tg.F32
    co, gain, r1 = sos_design(orc, 5, 0.1, 2)
    h = orc.design_rif_fen(31, "lp", 0.25)
    return [lambda C: tg.FirBank(h, dt, C), lambda C: tg.SosBank(co, gain, dt, C, r1)]


@pytest.mark.parametrize("cplx", [False, True])
def test_strides_pointers_in_place_and_host_arrays(tg, orc, cplx):
    import torch
    rng = np.random.default_rng(11)
    C = 6
    for make in _banks(tg, orc, cplx):
        for n in (4096, 4097, 130):
            xs = [rand_dev(rng, (C, n), cplx) + 0.5 for _ in range(2)]
            ref_bank = make(C)
            refs = [ref_bank.step(x) for x in xs]
            # strided rows, ldx != ldy > n
            b = make(C)
            for x, ref in zip(xs, refs):
                xv = torch.zeros(C, n + 5, dtype=x.dtype, device="cuda")[:, :n]
                xv.copy_(x)
                yv = torch.zeros(C, n + 9, dtype=x.dtype, device="cuda")[:, :n]
                b.step(xv, yv)
                assert same_bits(yv, ref)
            # odd ld: misaligned channel bases, input and output
            b = make(C)
            for x, ref in zip(xs, refs):
                xv = torch.zeros(C * (n + 1) + 1, dtype=x.dtype, device="cuda")[1:].view(C, n + 1)[:, :n]
                xv.copy_(x)
                yv = torch.zeros(C * (n + 3) + 1, dtype=x.dtype, device="cuda")[1:].view(C, n + 3)[:, :n]
                b.step(xv, yv)
                assert same_bits(yv, ref)
            # in place, packed and strided
            b, b2 = make(C), make(C)
            for x, ref in zip(xs, refs):
                y = x.clone()
                b.step(y, y)
                assert same_bits(y, ref)
                yv = torch.zeros(C, n + 4, dtype=x.dtype, device="cuda")[:, :n]
                yv.copy_(x)
                b2.step(yv, yv)
                assert same_bits(yv, ref)
            # numpy host arrays (packed, and a strided host view in and out)
            b, b2 = make(C), make(C)
            for x, ref in zip(xs, refs):
                xh = x.cpu().numpy()
                assert same_bits(torch.from_numpy(b.step(xh)).cuda(), ref)
                xw = np.zeros((C, n + 3), xh.dtype)
                xw[:, :n] = xh
                yw = np.zeros((C, n + 7), xh.dtype)
                b2.step(xw[:, :n], yw[:, :n])
                assert same_bits(torch.from_numpy(np.ascontiguousarray(yw[:, :n])).cuda(), ref)
            torch.cuda.synchronize()


def test_n_zero_is_a_no_op(tg, orc):
    import torch
    for make in _banks(tg, orc, False):
        b, ref = make(3), make(3)
        x = torch.randn(3, 100, device="cuda")
        b.step(torch.zeros(3, 0, device="cuda"))
        assert same_bits(b.step(x), ref.step(x))


# ------------------------------------------------------------------------------------------------ state interchange
@pytest.mark.parametrize("cplx", [False, True])
def test_fir_history_round_trip_and_reset(tg, orc, cplx):
    import torch
    rng = np.random.default_rng(5)
    h = orc.design_rif_fen(127, "lp", 0.1)
    dt = tg.C64 if cplx else tg.F32
    C = 9
    x1, x2 = rand_dev(rng, (C, 3000), cplx), rand_dev(rng, (C, 5000), cplx)
    a = tg.FirBank(h, dt, C)
    y1 = a.step(x1)
    hist = a.get_history()
    assert hist.shape == (C, 126)
    np.testing.assert_array_equal(hist, x1[:, -126:].cpu().numpy())
    b = tg.FirBank(h, dt, C)
    b.set_history(hist)
    assert same_bits(b.step(x2), a.step(x2))
    # device buffers too, and against a single handle's history
    hd = torch.empty(C, 126, dtype=x1.dtype, device="cuda")
    a.get_history(hd)
    f = tg.Fir(h, dt, tg.FIR_DIRECT)
    f.step(x1[4].contiguous()); f.step(x2[4].contiguous())
    fh = f.get_history(torch.empty(126, dtype=x1.dtype, device="cuda"))
    assert same_bits(hd[4], fh)
    a.reset()
    assert same_bits(a.step(x1), y1)


@pytest.mark.parametrize("order,fc,cplx,forme", [(12, 0.25, False, 2), (5, 0.1, True, 2), (4, 0.02, False, 1)])
def test_sos_state_moves_to_a_single_handle_and_reset(tg, orc, order, fc, cplx, forme):
    co, gain, r1 = sos_design(orc, order, fc, forme)
    dt = tg.C64 if cplx else tg.F32
    rng = np.random.default_rng(order)
    C = 7
    x1, x2 = rand_dev(rng, (C, 3001), cplx) + 2.0, rand_dev(rng, (C, 4096), cplx)
    bank = tg.SosBank(co, gain, dt, C, r1, forme=forme)
    y1 = bank.step(x1)
    states = [bank.get_state(c) for c in range(C)]
    y2 = bank.step(x2)
    for c in (0, 3, C - 1):
        s = tg.Sos(co, gain, dt, r1, forme=forme)
        s.set_state(states[c])
        ref = s.step(x2[c].contiguous())
        assert (y2[c] - ref).abs().max().item() <= 1e-5 * ref.abs().max().item(), c
    # and back: a single handle's state into a bank channel
    s = tg.Sos(co, gain, dt, r1, forme=forme)
    s.step(x1[2].contiguous())
    bank2 = tg.SosBank(co, gain, dt, C, r1, forme=forme)
    bank2.set_state(2, s.get_state())
    ref = s.step(x2[2].contiguous())
    assert (bank2.step(x2)[2] - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    bank.reset()                                          # the state at creation: the seed pending again
    assert same_bits(bank.step(x1), y1)


# ------------------------------------------------------------------------------------------------ isolation
@pytest.mark.parametrize("cplx", [False, True])
def test_nonfinite_channel_leaves_the_others_bit_identical(tg, orc, cplx):
    rng = np.random.default_rng(9)
    C = 8
    for make in _banks(tg, orc, cplx):
        x1, x2 = rand_dev(rng, (C, 5000), cplx), rand_dev(rng, (C, 4096), cplx)
        bad = x1.clone()
        bad[2, 1234] = float("nan")
        bad[5, 4999] = float("inf")
        clean, dirty = make(C), make(C)
        outs = [(clean.step(a), dirty.step(b)) for a, b in ((x1, bad), (x2, x2))]
        for yc, yd in outs:
            for c in range(C):
                if c not in (2, 5):
                    assert same_bits(yc[c], yd[c]), c


# ------------------------------------------------------------------------------------------------ many channels
def test_many_channels_beyond_the_grid_y_limit(tg, orc):
    import torch
    C, n = 70000, 64
    rng = np.random.default_rng(70)
    co, gain, r1 = sos_design(orc, 12, 0.25, 2)
    h = orc.design_rif_fen(31, "lp", 0.25)
    xs = [torch.randn(C, n, device="cuda") + 1.0 for _ in range(2)]
    fb, sb = tg.FirBank(h, tg.F32, C), tg.SosBank(co, gain, tg.F32, C, r1)
    outs = [(fb.step(x), sb.step(x)) for x in xs]
    torch.cuda.synchronize()
    for c in sorted(set([0, 1, 65534, 65535, 65536, C - 1] + list(rng.integers(0, C, 8)))):
        f, s = tg.Fir(h, tg.F32, tg.FIR_DIRECT), tg.Sos(co, gain, tg.F32, r1)
        for x, (yf, ys) in zip(xs, outs):
            assert same_bits(yf[c], f.step(x[c].contiguous())), c
            ref = s.step(x[c].contiguous())
            assert (ys[c] - ref).abs().max().item() <= 1e-5 * ref.abs().max().item(), c


def test_channel_offsets_past_2_31_elements(tg, orc):
    import torch
    C, ld, n = 131073, 16384, 16381
    assert C * ld > 2 ** 31
    co, gain, r1 = sos_design(orc, 12, 0.25, 2)
    h = orc.design_rif_fen(31, "lp", 0.25)
    g = torch.Generator(device="cuda").manual_seed(31)
    buf = torch.randn(C, ld, device="cuda", generator=g)
    x = buf[:, :n]
    y = torch.empty(C, ld, device="cuda")[:, :n]
    picks = (0, C // 2, C - 1)
    tg.FirBank(h, tg.F32, C).step(x, y)
    torch.cuda.synchronize()
    yf = {c: y[c].clone() for c in picks}
    tg.SosBank(co, gain, tg.F32, C, r1).step(x, y)
    torch.cuda.synchronize()
    for c in picks:
        assert same_bits(yf[c], tg.Fir(h, tg.F32, tg.FIR_DIRECT).step(x[c].contiguous())), c
        ref = tg.Sos(co, gain, tg.F32, r1).step(x[c].contiguous())
        assert (y[c] - ref).abs().max().item() <= 1e-5 * ref.abs().max().item(), c
    del buf, x, y
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ argument checks
def test_invalid_arguments_report_status_and_reason(tg):
    import torch
    L = tg.lib()
    h = ctypes.c_void_p()
    taps = np.ones(3, np.float32)
    coefs = np.array([1.0, 2.0, 1.0, -0.5, 0.25], np.float32)

    def status(rc, code, *words):
        assert rc == code, (rc, L.tsdgpu_last_error())
        msg = L.tsdgpu_last_error().decode()
        assert all(w in msg for w in words), msg

    status(L.tsdgpu_fir_bank_create(ctypes.byref(h), tg.F32, tg.F32, taps.ctypes.data, 3, 0), 1, "channels")
    status(L.tsdgpu_fir_bank_create(ctypes.byref(h), tg.F32, tg.C64, taps.ctypes.data, 3, 2), 1, "complex taps")
    status(L.tsdgpu_fir_bank_create(ctypes.byref(h), tg.F32, tg.F32, np.ones(12290, np.float32).ctypes.data, 12290, 2), 3, "12289")
    status(L.tsdgpu_sos_bank_create(ctypes.byref(h), tg.F32, coefs.ctypes.data, 1, 1.0, None, 2, 0), 1, "channels")
    status(L.tsdgpu_sos_bank_create(ctypes.byref(h), tg.F32, coefs.ctypes.data, 1, 1.0, None, 3, 2), 1, "forme")
    status(L.tsdgpu_sos_bank_create(ctypes.byref(h), 7, coefs.ctypes.data, 1, 1.0, None, 2, 2), 1, "data_type")
    fb, sb = tg.FirBank(taps, tg.F32, 4), tg.SosBank(coefs, 1.0, tg.F32, 4)
    x = torch.zeros(4 * 100 + 8, device="cuda")
    p = x.data_ptr()
    for step, hb in ((L.tsdgpu_fir_bank_step, fb._h), (L.tsdgpu_sos_bank_step, sb._h)):
        status(step(hb, p, 50, p + 4 * 100 * 4, 99, 100, None), 1, "leading dimensions")
        status(step(hb, p, 100, p + 4, 100, 100, None), 1, "overlap")               # y one sample after x
        status(step(hb, p, 100, p, 101, 100, None), 1, "overlap")                   # x == y, ldx != ldy
        status(step(hb, None, 100, p, 100, 100, None), 1, "NULL")
        status(step(hb, p, 100, p + 4 * 100 * 4, 100, -1, None), 1, "negative")
        assert step(hb, p, 100, p, 100, 0, None) == 0                                # n == 0: no-op
    st = np.zeros(L.tsdgpu_sos_state_floats(), np.float32)
    status(L.tsdgpu_sos_bank_get_state(sb._h, 4, st.ctypes.data, None), 1, "channel")
    status(L.tsdgpu_sos_bank_set_state(sb._h, -1, st.ctypes.data, None), 1, "channel")
    with pytest.raises(tg.TsdGpuError):
        fb.step(torch.zeros(3, 10, device="cuda"))                                   # 3 rows for 4 channels
