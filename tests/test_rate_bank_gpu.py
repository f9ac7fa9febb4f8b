"""Rate-changing channel bank (include/tsdgpu.h: tsdgpu_polyfir_bank): every channel against its own single-stream PolyFir fed
the same blocks (bit-identical wherever the single handle runs its direct or fused kernel), against the oracle and float64 on
every output elsewhere, plus block invariance, layouts (strides, misaligned rows, y a view of x, host arrays), state, channel
isolation, many channels, channel offsets past 2^31 elements and the argument checks."""
import ctypes

import numpy as np
import pytest

import f64ref as R

pytestmark = pytest.mark.gpu
DEC, HB, UPS, PICK = 0, 1, 2, 3


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
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def rand_dev(rng, shape, cplx, scale=1.0):
    import torch
    x = rng.standard_normal(shape)
    if cplx:
        x = x + 1j * rng.standard_normal(shape)
    return torch.from_numpy((scale * x).astype(np.complex64 if cplx else np.float32)).cuda()


def dtype_of(tg, cplx):
    return tg.C64 if cplx else tg.F32


def make_bank(tg, kind, cplx, C, taps, Rr):
    return tg.PolyFirBank(kind, dtype_of(tg, cplx), C, None if kind == PICK else taps, Rr)


def make_single(tg, kind, cplx, taps, Rr):
    return tg.PolyFir(kind, dtype_of(tg, cplx), None if kind == PICK else taps, Rr)


def run_blocks(bank, x, cuts):
    """the (C, N) stream through the bank in calls [a, b); returns the (C, n_out) outputs side by side"""
    import torch
    outs = [bank.step(x[:, a:b]) for a, b in cuts]
    torch.cuda.synchronize()
    return torch.cat(outs, dim=1)


def cuts_of(sizes):
    e = np.concatenate([[0], np.cumsum(sizes)])
    return [(int(a), int(b)) for a, b in zip(e[:-1], e[1:])]


# ------------------------------------------------------------------------------------- 1. bit identity with single handles
# every configuration here is one the single handle serves with decim_direct_kernel / ups_direct_kernel / polyfir_fused_kernel
# (fused_step's dispatch in polyphase.hip: the rows kernel takes decimators of rate 2..16 with 32 taps or more outside the
# direct regime -- none below)
BIT_CASES = ([(DEC, r, k) for r in (2, 4, 8) for k in (1, 15, 31, 64)] + [(DEC, r, k) for r in (3, 5, 16, 48) for k in (7, 31)] +
             [(HB, 2, k) for k in (7, 15, 31, 63)] + [(UPS, r, k) for r in (2, 4) for k in (8, 31, 128)] +
             [(UPS, r, k) for r in (3, 8) for k in (24, 95)] + [(PICK, r, 0) for r in (1, 2, 7, 100)])


@pytest.mark.parametrize("C", [1, 3, 257])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("kind,Rr,K", BIT_CASES)
def test_bank_bit_identical_to_single_handles(tg, kind, Rr, K, cplx, C):
    import torch
    rng = np.random.default_rng(1000 * kind + 10 * Rr + K + C)
    taps = rng.standard_normal(max(K, 1)).astype(np.float32)
    blocks = [1, 7, 4095, 4096, 4097, 65539] if C < 257 else [1, 7, 4096, 4097, 20003]
    bank = make_bank(tg, kind, cplx, C, taps, Rr)
    xs = [rand_dev(rng, (C, n), cplx) for n in blocks]
    counts, ys = [], []
    for x in xs:
        counts.append(bank.out_count(x.shape[1]))       # (advances nothing: asked before the step it describes)
        ys.append(bank.step(x))
    torch.cuda.synchronize()
    L = tg.lib()
    for c in range(C):
        f = make_single(tg, kind, cplx, taps, Rr)
        for x, y, m in zip(xs, ys, counts):
            assert L.tsdgpu_polyfir_out_count(f._h, x.shape[1]) == m == y.shape[1], (kind, Rr, K, C, c, x.shape[1])
            ref = f.step(x[c].contiguous())
            assert same_bits(y[c], ref), (kind, Rr, K, cplx, C, c, x.shape[1])


# short blocks share a wave in the direct scheme (8, 16 or 32 lanes per channel): every split, a last wave with fewer channels
@pytest.mark.parametrize("C", [5, 37])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("kind,Rr,K", [(DEC, 2, 15), (DEC, 4, 31), (DEC, 8, 64), (HB, 2, 31), (UPS, 2, 31), (UPS, 4, 128)])
def test_short_blocks_bit_identical_to_single_handles(tg, kind, Rr, K, cplx, C):
    import torch
    rng = np.random.default_rng(77 * kind + 10 * Rr + K + C)
    taps = rng.standard_normal(K).astype(np.float32)
    blocks = [9, 100, 129, 200, 257, 64, 300, 511, 512, 513, 128, 65]
    bank = make_bank(tg, kind, cplx, C, taps, Rr)
    xs = [rand_dev(rng, (C, n), cplx) for n in blocks]
    ys = [bank.step(x) for x in xs]
    torch.cuda.synchronize()
    for c in range(C):
        f = make_single(tg, kind, cplx, taps, Rr)
        for x, y in zip(xs, ys):
            assert same_bits(y[c], f.step(x[c].contiguous())), (kind, Rr, K, cplx, C, c, x.shape[1])


# ------------------------------------------------------------------------------------- 2. oracle and float64, every output
ORACLE_CASES = ([(DEC, r, k) for r in (3, 6, 16) for k in (32, 127, 1000)] + [(DEC, r, k) for r in (2, 4) for k in (65, 255)] +
                [(UPS, 4, 400), (DEC, 4, 31), (HB, 2, 15), (UPS, 2, 31)])


def assert_componentwise(y, y64, scale, m, what=""):
    """|y - y64|_i <= gamma_m scale_i on EVERY output"""
    g = R.gamma(m)
    e = np.abs(np.asarray(y).astype(np.complex128) - y64)
    bad = e > g * scale
    worst = float(np.max(e / np.maximum(g * scale, 1e-300))) if len(e) else 0.0
    print(what, "worst err / componentwise bound", worst)
    assert not bad.any(), (what, int(np.argmax(bad)), worst)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("kind,Rr,K", ORACLE_CASES)
def test_bank_against_oracle_and_float64(tg, orc, kind, Rr, K, cplx):
    rng = np.random.default_rng(100 * Rr + K + cplx)
    taps = orc.design_rif_fen(K, "lp", 0.4 / Rr).astype(np.float32)
    C, N = 5, 40000
    sizes, left = [], N
    while left > 0:
        s = min(left, int(rng.choice([1, 2, 7, 63, 64, 65, 1023, 2048, 4097, 9000])))
        sizes.append(s)
        left -= s
    x = rand_dev(rng, (C, N), cplx)
    bank = make_bank(tg, kind, cplx, C, taps, Rr)
    y = run_blocks(bank, x, cuts_of(sizes)).cpu().numpy()
    xh = x.cpu().numpy()
    for c in range(C):
        o = orc.PolyUps(taps, Rr) if kind == UPS else orc.PolyDecim(taps, Rr, kind=1 if kind == HB else 0)
        yo = np.concatenate([o.step(xh[c, a:b]) for a, b in cuts_of(sizes)])
        assert y.shape[1] == len(yo), (c, y.shape, len(yo))
        peak_err = np.abs(y[c] - yo).max() / np.abs(yo).max()
        print("channel", c, "err / oracle peak", peak_err)
        assert peak_err <= 1e-5, (kind, Rr, K, c, peak_err)
        xa = np.abs(xh[c].astype(np.complex128))
        if kind == UPS:
            ref = R.ups(taps, xh[c], Rr)
            cp = np.abs(R.ups_taps(taps, Rr).astype(np.float64))
            W = len(cp) // Rr
            scale = np.zeros(len(ref))
            for i in range(Rr):
                scale[i::Rr] = np.convolve(cp[Rr - 1 - i:: Rr][:W][::-1], xa)[:N]
        else:
            ref = R.decim(taps, xh[c], Rr, halfband=kind == HB)
            ca = np.abs(taps.astype(np.float64))
            if kind == HB:
                ca[1::2] = 0
                ca[K // 2] += 0.5
            W = K
            scale = np.convolve(ca[::-1], xa)[:N][Rr - 1:: Rr]
        assert len(ref) == y.shape[1]
        assert_componentwise(y[c], ref, scale, W + 2, what=f"kind={kind} R={Rr} K={K} cplx={cplx} channel {c}")


# ------------------------------------------------------------------------------------- 3. block invariance
INVARIANCE_CASES = [(DEC, 4, 31), (DEC, 8, 64), (DEC, 3, 31), (DEC, 6, 127), (HB, 2, 15), (UPS, 2, 31), (UPS, 3, 24), (UPS, 4, 400),
                    (PICK, 7, 0)]


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("kind,Rr,K", INVARIANCE_CASES)
def test_block_invariance(tg, kind, Rr, K, cplx):
    rng = np.random.default_rng(7 * Rr + K + cplx)
    taps = rng.standard_normal(max(K, 1)).astype(np.float32)
    C, N = 3, 20011
    x = rand_dev(rng, (C, N), cplx)
    whole = run_blocks(make_bank(tg, kind, cplx, C, taps, Rr), x, [(0, N)])
    ragged = run_blocks(make_bank(tg, kind, cplx, C, taps, Rr), x, cuts_of([1, 7, 63, 4097, 2, 5000, 4096, N - 13266]))
    single = run_blocks(make_bank(tg, kind, cplx, C, taps, Rr), x, cuts_of([1] * (3 * Rr) + [N - 3 * Rr]))
    assert same_bits(whole, ragged) and same_bits(whole, single), (kind, Rr, K, cplx)


# ------------------------------------------------------------------------------------- 4. layouts
LAYOUT_CASES = [(DEC, 4, 31), (DEC, 5, 31), (DEC, 3, 127), (HB, 2, 15), (UPS, 2, 31), (UPS, 3, 24), (PICK, 3, 0)]


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("kind,Rr,K", LAYOUT_CASES)
def test_strides_pointers_aliasing_and_host_arrays(tg, kind, Rr, K, cplx):
    import torch
    rng = np.random.default_rng(3 * Rr + K + cplx)
    taps = rng.standard_normal(max(K, 1)).astype(np.float32)
    C, blocks = 4, [4099, 1000, 5]

    def fresh():
        return make_bank(tg, kind, cplx, C, taps, Rr)

    xs = [rand_dev(rng, (C, n), cplx) for n in blocks]
    packed = [y.clone() for y in map(fresh().step, xs)]
    torch.cuda.synchronize()
    # row strides larger than n, on both sides; ldy > n_out
    b = fresh()
    for x, ref in zip(xs, packed):
        n, m = x.shape[1], ref.shape[1]
        xb = torch.zeros(C, n + 13, dtype=x.dtype, device="cuda")
        xb[:, :n] = x
        yb = torch.full((C, m + 9), 77.0, dtype=x.dtype, device="cuda")
        y = b.step(xb[:, :n], yb)
        assert same_bits(y, ref) and bool((yb[:, m:] == 77.0).all())
    # base pointers one element off 16-B alignment
    b = fresh()
    for x, ref in zip(xs, packed):
        n, m = x.shape[1], ref.shape[1]
        xb = torch.zeros(C, n + 4, dtype=x.dtype, device="cuda")
        xb[:, 1:n + 1] = x
        yb = torch.zeros(C, m + 4, dtype=x.dtype, device="cuda")
        y = b.step(xb[:, 1:n + 1], yb[:, 1:])
        assert same_bits(y[:, :m], ref) and y.shape[1] == m
    # y a view of x: same base, ldy == ldx (the upsampler in a buffer wide enough for its outputs)
    b = fresh()
    for x, ref in zip(xs, packed):
        n, m = x.shape[1], ref.shape[1]
        buf = torch.zeros(C, max(n, m), dtype=x.dtype, device="cuda")
        buf[:, :n] = x
        y = b.step(buf[:, :n], buf)
        assert y.data_ptr() == buf.data_ptr() and same_bits(y, ref)
    # host numpy arrays in and out (strided rows in, packed out)
    b = fresh()
    for x, ref in zip(xs, packed):
        n = x.shape[1]
        xh = np.zeros((C, n + 3), x.cpu().numpy().dtype)
        xh[:, :n] = x.cpu().numpy()
        y = b.step(xh[:, :n])
        assert isinstance(y, np.ndarray) and same_bits(torch.from_numpy(np.ascontiguousarray(y)).cuda(), ref)


def test_n_zero_is_a_no_op_and_short_blocks_advance(tg):
    import torch
    taps = np.arange(1, 16, dtype=np.float32)
    b = tg.PolyFirBank(DEC, tg.F32, 3, taps, 8)
    x = torch.randn(3, 21, device="cuda")
    assert b.step(x[:, :0]).shape == (3, 0) and b.get_state()[1] == 0
    parts = [b.step(x[:, 0:3]), b.step(x[:, 3:7]), b.step(x[:, 7:7]), b.step(x[:, 7:21])]
    assert [p.shape[1] for p in parts] == [0, 0, 0, 2]
    assert same_bits(parts[3], tg.PolyFirBank(DEC, tg.F32, 3, taps, 8).step(x))


# ------------------------------------------------------------------------------------- 5. state
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("kind,Rr,K", [(DEC, 4, 31), (DEC, 5, 31), (DEC, 6, 127), (HB, 2, 15), (UPS, 2, 31), (UPS, 3, 24), (PICK, 7, 0)])
def test_state_round_trip_reset_and_history_rows(tg, kind, Rr, K, cplx):
    import torch
    rng = np.random.default_rng(11 * Rr + K + cplx)
    taps = rng.standard_normal(max(K, 1)).astype(np.float32)
    C = 3
    b = make_bank(tg, kind, cplx, C, taps, Rr)
    x1, x2 = rand_dev(rng, (C, 4099), cplx), rand_dev(rng, (C, 3001), cplx)
    y1 = b.step(x1).clone()
    hist, phase = b.get_state()
    assert hist.shape == (C, b.history_len) and (b.history_len == 0) == (kind == PICK)
    if kind in (DEC, HB):
        assert phase == 4099 % Rr
    y2 = b.step(x2).clone()
    b.set_state(hist, phase)
    assert same_bits(b.step(x2), y2)
    # device-side state buffers as well
    if b.history_len:
        hd = torch.zeros(C, b.history_len, dtype=x1.dtype, device="cuda")
        b.set_state(hist, phase)
        _, ph = b.get_state(hd)
        assert ph == phase and np.array_equal(hd.cpu().numpy().view(np.int32), hist.view(np.int32))
        b.set_state(hd, phase)
        assert same_bits(b.step(x2), y2)
    b.reset()
    assert b.get_state()[1] == 0 and same_bits(b.step(x1), y1)
    # a history row written by set_state is what a channel would have seen: the row fed as a preceding block to a fresh bank
    if b.history_len:
        rows = rand_dev(rng, (C, b.history_len), cplx)
        via_block = make_bank(tg, kind, cplx, C, taps, Rr)
        via_block.step(rows)
        ph = via_block.get_state()[1]
        via_state = make_bank(tg, kind, cplx, C, taps, Rr)
        via_state.set_state(rows.cpu().numpy(), ph)
        assert same_bits(via_state.step(x2), via_block.step(x2))


# ------------------------------------------------------------------------------------- 6. isolation
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("kind,Rr,K", [(DEC, 4, 31), (DEC, 3, 31), (DEC, 6, 127), (HB, 2, 15), (UPS, 2, 31), (UPS, 3, 24), (PICK, 3, 0)])
def test_nonfinite_channel_leaves_the_others_bit_identical(tg, kind, Rr, K, cplx):
    import torch
    rng = np.random.default_rng(13 * Rr + K + cplx)
    taps = rng.standard_normal(max(K, 1)).astype(np.float32)
    C, bad = 6, 2
    xs = [rand_dev(rng, (C, n), cplx) for n in (4097, 1000)]
    clean = [y.clone() for y in map(make_bank(tg, kind, cplx, C, taps, Rr).step, xs)]
    dirty_in = [x.clone() for x in xs]
    dirty_in[0][bad, 99] = float("nan")
    dirty_in[0][bad, 4096] = float("inf")
    dirty_in[1][bad, 0] = float("-inf")
    dirty = [y.clone() for y in map(make_bank(tg, kind, cplx, C, taps, Rr).step, dirty_in)]
    torch.cuda.synchronize()
    for a, b in zip(clean, dirty):
        for c in range(C):
            if c != bad:
                assert same_bits(a[c], b[c]), c
    assert not bool(torch.isfinite(torch.view_as_real(dirty[0][bad]) if cplx else dirty[0][bad]).all())


# ------------------------------------------------------------------------------------- 7. scale
@pytest.mark.parametrize("kind,Rr,K", [(DEC, 4, 31), (DEC, 3, 31), (UPS, 2, 31), (PICK, 3, 0)])
def test_many_channels_beyond_the_grid_y_limit(tg, kind, Rr, K):
    import torch
    C, n = 70000, 64
    rng = np.random.default_rng(70 + Rr)
    taps = rng.standard_normal(max(K, 1)).astype(np.float32)
    xs = [torch.randn(C, n, device="cuda") for _ in range(2)]
    b = make_bank(tg, kind, False, C, taps, Rr)
    ys = [b.step(x) for x in xs]
    torch.cuda.synchronize()
    for c in sorted(set([0, 1, 65534, 65535, 65536, C - 1] + list(rng.integers(0, C, 8)))):
        f = make_single(tg, kind, False, taps, Rr)
        for x, y in zip(xs, ys):
            assert same_bits(y[c], f.step(x[c].contiguous())), c


@pytest.mark.parametrize("kind,Rr,K", [(DEC, 4, 31), (DEC, 3, 31), (UPS, 2, 31), (PICK, 3, 0)])
def test_channel_offsets_past_2_31_elements(tg, kind, Rr, K):
    import torch
    C, ld, n = 3, (1 << 30) + 8, 16381
    assert (C - 1) * ld > 2 ** 31
    rng = np.random.default_rng(31 + Rr)
    taps = rng.standard_normal(max(K, 1)).astype(np.float32)
    xbuf = torch.empty(C, ld, device="cuda")
    ybuf = torch.empty(C, ld, device="cuda")
    x = xbuf[:, :n]
    x.copy_(torch.randn(C, n, device="cuda"))
    b = make_bank(tg, kind, False, C, taps, Rr)
    y = b.step(x, ybuf[:, : 2 * n])
    torch.cuda.synchronize()
    assert y.data_ptr() == ybuf.data_ptr()
    for c in range(C):
        assert same_bits(y[c], make_single(tg, kind, False, taps, Rr).step(x[c].contiguous())), c
    del xbuf, ybuf, x, y
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------- 8. argument checks
def test_invalid_arguments_report_status_and_reason(tg):
    import torch
    L = tg.lib()
    h = ctypes.c_void_p()
    taps = np.ones(31, np.float32)
    tp = taps.ctypes.data

    def status(rc, code, *words):
        assert rc == code, (rc, L.tsdgpu_last_error())
        msg = L.tsdgpu_last_error().decode()
        assert msg and all(w in msg for w in words), msg

    create = L.tsdgpu_polyfir_bank_create
    status(create(None, DEC, tg.F32, tp, 31, 4, 2), 1, "NULL")
    status(create(ctypes.byref(h), DEC, tg.F32, tp, 31, 4, 0), 1, "channels")
    status(create(ctypes.byref(h), 4, tg.F32, tp, 31, 4, 2), 1, "kind")
    status(create(ctypes.byref(h), -1, tg.F32, tp, 31, 4, 2), 1, "kind")
    status(create(ctypes.byref(h), DEC, 7, tp, 31, 4, 2), 1, "data_type")
    status(create(ctypes.byref(h), DEC, tg.F32, tp, 31, 0, 2), 1, "rate")
    status(create(ctypes.byref(h), PICK, tg.F32, None, 0, 5000, 2), 1, "rate")
    status(create(ctypes.byref(h), DEC, tg.F32, None, 0, 4, 2), 1, "K > 0")
    # what the bank does not serve is refused at create with the limit named
    big = np.ones(5000, np.float32)
    status(create(ctypes.byref(h), DEC, tg.F32, big.ctypes.data, 5000, 2, 2), 3, "4096")
    status(create(ctypes.byref(h), UPS, tg.F32, big.ctypes.data, 5000, 3, 2), 3, "4096")
    status(create(ctypes.byref(h), DEC, tg.F32, tp, 31, 100, 2), 3, "16000")
    assert not h.value

    b = tg.PolyFirBank(DEC, tg.F32, 4, taps, 4)
    x = torch.zeros(4 * 100 + 8, device="cuda")
    y = torch.zeros(4 * 100 + 8, device="cuda")
    px, py = x.data_ptr(), y.data_ptr()
    got = ctypes.c_int64(-5)
    step = L.tsdgpu_polyfir_bank_step
    status(step(None, px, 100, 100, py, 25, 25, ctypes.byref(got), None), 1, "NULL handle")
    status(step(b._h, px, 50, 100, py, 25, 25, ctypes.byref(got), None), 1, "ldx")
    status(step(b._h, px, 100, 100, py, 24, 25, ctypes.byref(got), None), 1, "ldy")
    status(step(b._h, px, 100, 100, py, 25, 24, ctypes.byref(got), None), 1, "y_capacity")
    status(step(b._h, None, 100, 100, py, 25, 25, ctypes.byref(got), None), 1, "NULL")
    status(step(b._h, px, 100, 100, None, 25, 25, ctypes.byref(got), None), 1, "NULL")
    status(step(b._h, px, 100, -1, py, 25, 25, ctypes.byref(got), None), 1, "negative")
    assert b.get_state()[1] == 0                                                          # refused steps advance nothing
    assert step(b._h, px, 100, 0, py, 25, 25, ctypes.byref(got), None) == 0 and got.value == 0   # n == 0: no-op
    assert step(b._h, px, 100, 3, None, 0, 0, ctypes.byref(got), None) == 0 and got.value == 0   # n < R: no output needed
    assert b.get_state()[1] == 3
    assert L.tsdgpu_polyfir_bank_out_count(None, 10) == -1 and L.tsdgpu_polyfir_bank_out_count(b._h, -1) == -1
    hist = np.zeros((4, b.history_len), np.float32)
    status(L.tsdgpu_polyfir_bank_set_state(b._h, hist.ctypes.data, 4, None), 1, "phase")
    status(L.tsdgpu_polyfir_bank_set_state(b._h, hist.ctypes.data, -1, None), 1, "phase")
    status(L.tsdgpu_polyfir_bank_set_state(b._h, None, 0, None), 1, "NULL")
    status(L.tsdgpu_polyfir_bank_get_state(None, hist.ctypes.data, None, None), 1, "NULL")
    status(L.tsdgpu_polyfir_bank_reset(None), 1, "NULL")
    assert L.tsdgpu_polyfir_bank_history_len(b._h) == 30 and L.tsdgpu_polyfir_bank_history_len(None) == -1
    assert L.tsdgpu_polyfir_bank_destroy(None) == 0
    with pytest.raises(tg.TsdGpuError):
        b.step(torch.zeros(3, 10, device="cuda"))                                         # 3 rows for 4 channels
    with pytest.raises(tg.TsdGpuError):
        b.step(torch.zeros(4, 100, device="cuda"), torch.zeros(4, 10, device="cuda"))     # y too short
