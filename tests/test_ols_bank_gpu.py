"""The overlap-save FIR bank (libtsd_amd/csrc/ols_bank.hip: FirBank(..., method=FIR_OVERLAP_SAVE / FIR_AUTO)): every channel
against the oracle on its own stream, channels independent of their index, the float64 bound of the single overlap-save
handle per channel at high dynamic range, non-finite samples staying inside their channel and their blocks, the state
interface shared with the direct bank, layouts, the per-step AUTO rule and the argument checks."""
import ctypes

import numpy as np
import pytest

import f64ref as R
from test_bank_gpu import KINDS, rand_dev, same_bits
from test_dynamic_range_gpu import C_FFT, ragged

pytestmark = pytest.mark.gpu
BAR = 1e-5          # of the reference's peak


@pytest.fixture(scope="module")
def tg():
    import libtsd_amd as t
    assert t.device_count() >= 1
    return t


def block_len(K):
    return 1024 - 64 * (-(-(K - 1) // 64))


def block_list(K, C):
    L = block_len(K)
    return [1, 7, L - 1, L, L + 1, 2 * L, 2 * L + 1, 4096, 4097, 20003] if C < 257 else [1, 7, 4096, 4097, 20003]


def taps_of(orc, K, ctaps):
    # (the window design has no 2-tap filter -- it returns NaNs --: the two-tap average stands in for it)
    h = orc.design_rif_fen(K, "lp", 0.1) if K > 2 else np.array([0.5, 0.5], np.float32)
    assert np.isfinite(h).all()
    if ctaps:
        h = (h * np.exp(2j * np.pi * 0.1 * np.arange(K))).astype(np.complex64)
    return h


def oracle_rows(orc, h, xh):
    """orc.fir(h, row) for every row (the oracle's C loop releases the interpreter lock: rows in parallel)"""
    from concurrent.futures import ThreadPoolExecutor
    rows = [np.ascontiguousarray(r) for r in xh]
    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(lambda r: orc.fir(h, r), rows))


def within_bar(y, ref):
    return np.abs(y - ref).max() <= BAR * np.abs(ref).max()


# ------------------------------------------------------------------------------------------------ 1, 5: parity, history
@pytest.mark.parametrize("C", [1, 3, 257])
@pytest.mark.parametrize("K", [2, 64, 65, 66, 127, 129, 513, 961])
@pytest.mark.parametrize("kind", list(KINDS))
def test_parity_with_the_reference_per_channel_streamed(tg, orc, kind, K, C):
    import torch
    dts, ctaps = KINDS[kind]
    dt, cplx = getattr(tg, dts), dts == "C64"
    rng = np.random.default_rng(K * 11 + C)
    h = taps_of(orc, K, ctaps)
    bank = tg.FirBank(h, dt, C, method=tg.FIR_OVERLAP_SAVE)
    assert bank.method_used == tg.FIR_OVERLAP_SAVE
    xs = [rand_dev(rng, (C, n), cplx) for n in block_list(K, C)]
    ys = []
    for x in xs:
        ys.append(bank.step(x))
        assert bank.method_used == tg.FIR_OVERLAP_SAVE
    torch.cuda.synchronize()
    xh = np.concatenate([x.cpu().numpy() for x in xs], axis=1)
    yh = np.concatenate([y.cpu().numpy() for y in ys], axis=1)
    for c, ref in enumerate(oracle_rows(orc, h, xh)):
        e, peak = np.abs(yh[c] - ref).max(), np.abs(ref).max()
        assert e <= BAR * peak, (kind, K, C, c, e / peak)
    # the state after these steps: the last K-1 input samples of every channel, bit-exact
    hist = bank.get_history()
    assert hist.shape == (C, K - 1)
    np.testing.assert_array_equal(hist.view(np.uint32), np.ascontiguousarray(xh[:, xh.shape[1] - (K - 1):]).view(np.uint32))


# ------------------------------------------------------------------------------------------------ 2: same rows, same bits
@pytest.mark.parametrize("K", [65, 127, 961])
@pytest.mark.parametrize("cplx", [False, True])
def test_same_rows_same_bits(tg, orc, cplx, K):
    C = 5
    rng = np.random.default_rng(K)
    h = taps_of(orc, K, False)
    bank = tg.FirBank(h, tg.C64 if cplx else tg.F32, C, method=tg.FIR_OVERLAP_SAVE)
    for n in block_list(K, C):
        x = rand_dev(rng, (1, n), cplx).repeat(C, 1).contiguous()
        y = bank.step(x)
        for c in range(1, C):
            assert same_bits(y[c], y[0]), (K, n, c)


# ------------------------------------------------------------------------------------------------ 3: float64 bound per channel
@pytest.mark.parametrize("cplx", [False, True])
def test_per_channel_float64_bound_at_high_dynamic_range(tg, orc, cplx):
    import torch
    K, C, n, N = 127, 4, 1 << 18, 1024
    rng = np.random.default_rng(K + 3 * cplx)
    h = orc.design_rif_fen(K, "lp", 0.1)
    x = np.zeros((C, n), np.complex64 if cplx else np.float32)
    x[0] = R.burst_train(rng, n, N, cplx)[0]
    for c, amp in ((1, 1e6), (2, 1e-3)):
        v = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0)
        x[c] = (amp * v).astype(x.dtype)
    bank = tg.FirBank(h, tg.C64 if cplx else tg.F32, C, method=tg.FIR_OVERLAP_SAVE)
    outs = []
    for a, b in ragged(rng, n):
        outs.append(bank.step(torch.from_numpy(np.ascontiguousarray(x[:, a:b])).cuda()).cpu().numpy())
    y = np.concatenate(outs, axis=1)
    Hmax = np.abs(np.fft.fft(h.astype(np.float64), N)).max()
    for c in range(C):
        # every channel on ITS OWN input (real data: two blocks of the channel share a transform, hence 4N)
        bound = C_FFT * R.U * np.log2(N) * Hmax * R.window_norm(x[c], N if cplx else 4 * N)
        e = np.abs(y[c].astype(np.complex128) - R.fir(h, x[c]))
        worst = float((e / np.maximum(bound, 1e-300)).max())
        print("ols bank channel", c, "worst err / normwise bound", worst)
        assert (e <= bound).all(), (c, int(np.argmax(e > bound)), worst)
    assert not y[3].any()                                    # exact zeros in, exact zeros out


# ------------------------------------------------------------------------------------------------ 4: non-finite isolation
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("cplx", [False, True])
def test_nonfinite_sample_stays_in_its_channel_and_its_blocks(tg, orc, cplx, bad):
    import torch
    C, n, K, p = 3, 8192, 127, 3000
    rng = np.random.default_rng(4)
    h = orc.design_rif_fen(K, "lp", 0.1)
    dt = tg.C64 if cplx else tg.F32
    x1, x2 = rand_dev(rng, (C, n), cplx), rand_dev(rng, (C, n), cplx)
    xb = x1.clone()
    xb[1, p] = bad
    clean, dirty = tg.FirBank(h, dt, C, method=tg.FIR_OVERLAP_SAVE), tg.FirBank(h, dt, C, method=tg.FIR_OVERLAP_SAVE)
    yc, yd = clean.step(x1), dirty.step(xb)
    for c in (0, 2):
        assert same_bits(yc[c], yd[c]), c
    assert same_bits(yc[1, : p - 4096 if p > 4096 else 0], yd[1, : p - 4096 if p > 4096 else 0])
    assert same_bits(yc[1, p + 4097:], yd[1, p + 4097:])
    assert not torch.isfinite(torch.view_as_real(yd[1, p]) if cplx else yd[1, p]).all()
    # the history carries nothing of it here (p lies more than K-1 before the end): the next step is clean from K-1 on
    yc2, yd2 = clean.step(x2), dirty.step(x2)
    assert same_bits(yc2[:, K - 1:], yd2[:, K - 1:])
    # ... and when it does sit in the history, it reaches the channel's first blocks of the next step and nothing else
    xe = x1.clone()
    xe[1, n - 5] = bad
    dirty2, clean2 = tg.FirBank(h, dt, C, method=tg.FIR_OVERLAP_SAVE), tg.FirBank(h, dt, C, method=tg.FIR_OVERLAP_SAVE)
    dirty2.step(xe), clean2.step(x1)
    ye, yk = dirty2.step(x2), clean2.step(x2)
    assert same_bits(ye[0], yk[0]) and same_bits(ye[2], yk[2])
    assert same_bits(ye[1, 2048:], yk[1, 2048:])


# ------------------------------------------------------------------------------------------------ 5: state
@pytest.mark.parametrize("cplx", [False, True])
def test_state_set_reset_and_exchange_with_a_direct_bank(tg, orc, cplx):
    rng = np.random.default_rng(55)
    K, C = 127, 4
    h = orc.design_rif_fen(K, "lp", 0.1)
    dt = tg.C64 if cplx else tg.F32
    x1, x2, x3 = (rand_dev(rng, (C, n), cplx) for n in (3000, 5000, 2049))
    xh = np.concatenate([v.cpu().numpy() for v in (x1, x2, x3)], axis=1)
    refs = [orc.fir(h, xh[c]) for c in range(C)]
    a = tg.FirBank(h, dt, C, method=tg.FIR_OVERLAP_SAVE)
    y1 = a.step(x1)
    hist = a.get_history()
    np.testing.assert_array_equal(hist, x1[:, -(K - 1):].cpu().numpy())
    # set_history on a fresh bank, one step: the continued stream
    b = tg.FirBank(h, dt, C, method=tg.FIR_OVERLAP_SAVE)
    b.set_history(hist)
    y2 = b.step(x2).cpu().numpy()
    for c in range(C):
        seg = refs[c][3000:8000]
        assert np.abs(y2[c] - seg).max() <= BAR * np.abs(refs[c]).max(), c
    # reset: the first block again, bit-exact
    a.reset()
    assert same_bits(a.step(x1), y1)
    # a stream that moves overlap-save -> direct -> overlap-save through get / set_history
    d = tg.FirBank(h, dt, C, method=tg.FIR_DIRECT)
    d.set_history(a.get_history())
    yd = d.step(x2).cpu().numpy()
    o = tg.FirBank(h, dt, C, method=tg.FIR_OVERLAP_SAVE)
    o.set_history(d.get_history())
    yo = o.step(x3).cpu().numpy()
    assert d.method_used == tg.FIR_DIRECT and o.method_used == tg.FIR_OVERLAP_SAVE
    for c in range(C):
        peak = np.abs(refs[c]).max()
        assert np.abs(yd[c] - refs[c][3000:8000]).max() <= BAR * peak, c
        assert np.abs(yo[c] - refs[c][8000:]).max() <= BAR * peak, c


# ------------------------------------------------------------------------------------------------ 6: layouts
@pytest.mark.parametrize("cplx", [False, True])
def test_strides_misaligned_rows_in_place_and_host_arrays(tg, orc, cplx):
    import torch
    rng = np.random.default_rng(11)
    C, K = 6, 127
    h = orc.design_rif_fen(K, "lp", 0.1)
    make = lambda: tg.FirBank(h, tg.C64 if cplx else tg.F32, C, method=tg.FIR_OVERLAP_SAVE)
    for n in (4097, 130):
        xs = [rand_dev(rng, (C, n), cplx) + 0.5 for _ in range(2)]
        ref_bank = make()
        refs = [ref_bank.step(x) for x in xs]
        b = make()                                  # row-strided views
        for x, ref in zip(xs, refs):
            xv = torch.zeros(C, n + 5, dtype=x.dtype, device="cuda")[:, :n]
            xv.copy_(x)
            yv = torch.zeros(C, n + 5, dtype=x.dtype, device="cuda")[:, :n]
            b.step(xv, yv)
            assert same_bits(yv, ref)
        b = make()                                  # base offset of one sample, odd ld
        for x, ref in zip(xs, refs):
            xv = torch.zeros(C * (n + 1) + 1, dtype=x.dtype, device="cuda")[1:].view(C, n + 1)[:, :n]
            xv.copy_(x)
            yv = torch.zeros(C * (n + 3) + 1, dtype=x.dtype, device="cuda")[1:].view(C, n + 3)[:, :n]
            b.step(xv, yv)
            assert same_bits(yv, ref)
        b, b2 = make(), make()                      # in place, packed and strided
        for x, ref in zip(xs, refs):
            y = x.clone()
            b.step(y, y)
            assert same_bits(y, ref)
            yv = torch.zeros(C, n + 4, dtype=x.dtype, device="cuda")[:, :n]
            yv.copy_(x)
            b2.step(yv, yv)
            assert same_bits(yv, ref)
        b, b2 = make(), make()                      # host numpy arrays, packed and strided
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
    h = orc.design_rif_fen(127, "lp", 0.1)
    b, ref = (tg.FirBank(h, tg.F32, 3, method=tg.FIR_OVERLAP_SAVE) for _ in range(2))
    x = torch.randn(3, 100, device="cuda")
    b.step(torch.zeros(3, 0, device="cuda"))
    assert same_bits(b.step(x), ref.step(x))


def test_many_channels_in_one_linear_grid(tg, orc):
    import torch
    C, n, K = 70001, 16, 65
    h = orc.design_rif_fen(K, "lp", 0.1)
    g = torch.Generator(device="cuda").manual_seed(7)
    xs = [torch.randn(C, n, device="cuda", generator=g) + 1.0 for _ in range(2)]
    bank = tg.FirBank(h, tg.F32, C, method=tg.FIR_OVERLAP_SAVE)
    ys = [bank.step(x) for x in xs]
    torch.cuda.synchronize()
    rng = np.random.default_rng(70)
    for c in sorted(set([0, 1, 65534, 65535, 65536, C - 1] + [int(v) for v in rng.integers(0, C, 8)])):
        xc = np.concatenate([x[c].cpu().numpy() for x in xs])
        yc = np.concatenate([y[c].cpu().numpy() for y in ys])
        assert within_bar(yc, orc.fir(h, xc)), c


def test_channel_offsets_past_2_31_elements(tg, orc):
    import torch
    C, ld, n = 131073, 16384, 16381                   # tests/test_bank_gpu.py's shape for the direct bank
    assert C * ld > 2 ** 31
    K = 127
    h = orc.design_rif_fen(K, "lp", 0.1)
    g = torch.Generator(device="cuda").manual_seed(31)
    buf = torch.randn(C, ld, device="cuda", generator=g)
    x = buf[:, :n]
    y = torch.empty(C, ld, device="cuda")[:, :n]
    bank = tg.FirBank(h, tg.F32, C, method=tg.FIR_OVERLAP_SAVE)
    bank.step(x, y)
    torch.cuda.synchronize()
    hist = torch.empty(C, K - 1, device="cuda")
    bank.get_history(hist)
    for c in (0, C // 2, C - 1):
        assert within_bar(y[c].cpu().numpy(), orc.fir(h, x[c].cpu().numpy())), c
        assert same_bits(hist[c], x[c, n - (K - 1):])
    del buf, x, y, bank
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ 7: AUTO
@pytest.mark.parametrize("cplx", [False, True])
def test_auto_short_filter_is_the_direct_bank(tg, orc, cplx):
    rng = np.random.default_rng(31)
    h = orc.design_rif_fen(31, "lp", 0.25)
    dt = tg.C64 if cplx else tg.F32
    a, d = tg.FirBank(h, dt, 5, method=tg.FIR_AUTO), tg.FirBank(h, dt, 5, method=tg.FIR_DIRECT)
    assert a.method_used == tg.FIR_DIRECT
    for n in (4096, 100):
        x = rand_dev(rng, (5, n), cplx)
        assert same_bits(a.step(x), d.step(x))
        assert a.method_used == tg.FIR_DIRECT


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("K", [127, 961])
def test_auto_chooses_per_step_on_one_shared_history(tg, orc, cplx, K):
    """A long step then a short one, twice, in one stream.  The committed rule (ols_bank.hip: ols_bank_preferred, measured in
    profiles/r7_perf_ols_bank.txt): K = 127 lies between the lower tap count and 897, overlap-save at every n; K = 961
    (64 outputs per 1024-point block) takes overlap-save only for channels of up to 256 samples (512 for real data) -- so the
    steps of this stream alternate between the two schemes on the channels' one history row."""
    rng = np.random.default_rng(K)
    C = 3
    h = orc.design_rif_fen(K, "lp", 0.1)
    bank = tg.FirBank(h, tg.C64 if cplx else tg.F32, C, method=tg.FIR_AUTO)
    D, O = tg.FIR_DIRECT, tg.FIR_OVERLAP_SAVE
    assert bank.method_used == (O if K == 127 else D)           # before any step: what n >= 1024 takes
    xs = [rand_dev(rng, (C, n), cplx) for n in (4096, 16, 4096, 200)]
    ys, used = [], []
    for x in xs:
        ys.append(bank.step(x))
        used.append(bank.method_used)
    assert used == ([O, O, O, O] if K == 127 else [D, O, D, O])
    xh = np.concatenate([x.cpu().numpy() for x in xs], axis=1)
    yh = np.concatenate([y.cpu().numpy() for y in ys], axis=1)
    for c in range(C):
        assert within_bar(yh[c], orc.fir(h, xh[c])), c
    np.testing.assert_array_equal(bank.get_history(), xh[:, -(K - 1):])


# ------------------------------------------------------------------------------------------------ 8: argument checks
def test_argument_checks(tg, orc):
    import torch
    L = tg.lib()
    hd = ctypes.c_void_p()
    taps = np.ones(3, np.float32)
    for bad in (-1, 3, 17):
        rc = L.tsdgpu_fir_bank_create_method(ctypes.byref(hd), tg.F32, tg.F32, taps.ctypes.data, 3, 2, bad)
        assert rc == 1 and b"method" in L.tsdgpu_last_error(), (rc, L.tsdgpu_last_error())
    assert L.tsdgpu_fir_bank_method_used(None) == -1
    rng = np.random.default_rng(8)
    for K in (1, 1000):                                # outside the 1024-point plan: the direct scheme, and it says so
        h = rng.standard_normal(K).astype(np.float32)
        b, d = tg.FirBank(h, tg.F32, 3, method=tg.FIR_OVERLAP_SAVE), tg.FirBank(h, tg.F32, 3)
        assert b.method_used == tg.FIR_DIRECT
        x = rand_dev(rng, (3, 4097), False)
        assert same_bits(b.step(x), d.step(x))
        assert b.method_used == tg.FIR_DIRECT
    fb = tg.FirBank(orc.design_rif_fen(127, "lp", 0.1), tg.F32, 4, method=tg.FIR_OVERLAP_SAVE)
    x = torch.zeros(4 * 100 + 8, device="cuda")
    p = x.data_ptr()
    step = L.tsdgpu_fir_bank_step
    for args, word in (((p, 100, p + 4, 100, 100), b"overlap"),                          # y one sample after x
                       ((p, 100, p + 4 * 50, 100, 100), b"overlap"),                     # y inside x's first channel
                       ((p, 100, p, 101, 100), b"overlap"),                              # x == y, ldx != ldy
                       ((p, 50, p + 4 * 100 * 4, 99, 100), b"leading dimensions"),
                       ((None, 100, p, 100, 100), b"NULL")):
        rc = step(fb._h, *args, None)
        assert rc == 1 and word in L.tsdgpu_last_error(), (args, rc, L.tsdgpu_last_error())
    assert step(fb._h, p, 100, p, 100, 0, None) == 0
