"""One NaN, or one +Inf, in a streamed sequence: what it may touch and what must stay as it was.

The sample is placed mid-call, on the first and last sample of a call, and just before 1024- / 2048- / 4096-sample
boundaries inside a call (tile, block and chunk boundaries of the paths).  Compared with the clean run of the same
calls on a fresh handle:
  * causality  -- every output computed without the sample is bit-identical to the clean run;
  * recovery   -- after the contamination horizon the outputs are bit-identical to the clean run again, through the
                  later calls (the handle's history / window is not left poisoned).
Horizons (INTEGRATION.md "Non-finite samples"): libtsd's K - 1 outputs (mapped through the rate) widened to the zero-padded
tap counts of the direct kernels; overlap-save and the FFT plans: the blocks / rows that read the sample; SOS: the outputs
before the sample, then a non-finite output at the sample -- libtsd's recursion stays poisoned forever, the GPU's
block-parallel path only until a chunk starts from its warm-up after the sample, the exact carry forever; reset() clears it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tg():
    import libtsd_amd as t
    assert t.device_count() >= 1
    return t


CUTS = [(0, 70000), (70000, 70001), (70001, 200000), (200000, 300000)]
# mid-call, last / first sample of a call, just before 1024 / 2048 / 4096 boundaries inside a call
POSITIONS = [35000, 69999, 70000, 70001, 70001 + 1023, 70001 + 2047, 70001 + 4095, 200000 - 1, 200000 + 4095]


def rand(n, cplx, seed):
    rng = np.random.default_rng(seed)
    if cplx:
        return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    return rng.standard_normal(n).astype(np.float32)


def run(make, x):
    import torch
    op = make()
    out = [op.step(torch.from_numpy(np.ascontiguousarray(x[a:b])).cuda()).cpu().numpy() for a, b in CUTS]
    torch.cuda.synchronize()
    return np.concatenate(out)


def diff_span(y, clean):
    """(first, last) output index that is not bit-identical to the clean run, or None."""
    d = np.nonzero(~((y == clean) | (np.isnan(y) & np.isnan(clean))))[0]
    return (int(d[0]), int(d[-1])) if len(d) else None


def poison(x, p, bad):
    z = x.copy()
    z[p] = bad
    return z


BAD = [np.nan, np.inf]


def assert_span(make, x, p, bad, lo, hi, what, exact=False):
    """Outputs outside [lo, hi] bit-identical to the clean run; exact: the differing span IS [lo, hi], every output in
    it non-finite.  Returns the poisoned run."""
    clean = run(make, x)
    y = run(make, poison(x, p, bad))
    span = diff_span(y, clean)
    print(what, "p", p, bad, "differs over", span, "expected", (lo, hi))
    assert span is not None and span[0] >= lo and span[1] <= hi, (what, p, span, (lo, hi))
    assert not np.isfinite(y[span[0]:span[1] + 1]).all()
    if exact:
        assert span == (lo, hi) and not np.isfinite(y[lo:hi + 1]).any(), (what, p, span, (lo, hi))
    return y


@pytest.mark.parametrize("bad", BAD)
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("K", [7, 33, 127])
def test_fir_direct(tg, orc, K, cplx, bad):
    """The direct kernel pads the taps with zeros on the old side to KP = ceil(K / 2R) 2R (R = 16 float, 8 complex
    samples per lane, fir.hip) and multiplies them too: 0 x NaN reaches KP - 1 outputs after p where libtsd's reaches K - 1."""
    h = orc.design_rif_fen(K, "lp", 0.1)
    x = rand(300000, cplx, K)
    r2 = 16 if cplx else 32
    KP = -(-K // r2) * r2
    for p in POSITIONS:
        y = assert_span(lambda: tg.Fir(h, tg.C64 if cplx else tg.F32, tg.FIR_DIRECT), x, p, bad, p, p + KP - 1,
                        f"fir direct K={K}", exact=True)
        # libtsd's own mask (the oracle, streamed through the same calls): non-finite exactly on [p, p + K - 1]
        f = orc.Fir(h)
        z = poison(x, p, bad)
        yo = np.concatenate([f.step(z[a:b]) for a, b in CUTS])
        bad_o = np.nonzero(~np.isfinite(yo))[0]
        assert bad_o[0] == p and bad_o[-1] == p + K - 1 and len(bad_o) == K
        assert not np.isfinite(y[bad_o]).any()


@pytest.mark.parametrize("bad", BAD)
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("K", [127, 900])
def test_fir_overlap_save(tg, orc, K, cplx, bad):
    """The sample reaches the blocks whose input window holds it, and with real data the block transformed beside them:
    all within four transforms of [p, p + K - 1] (1024 points below K = 514, an upper bound of the long plans' size above)."""
    h = orc.design_rif_fen(K, "lp", 0.1)
    x = rand(300000, cplx, K)
    N = 1024 if K < 514 else 1 << int(np.ceil(np.log2(8 * K)))
    for p in POSITIONS:
        assert_span(lambda: tg.Fir(h, tg.C64 if cplx else tg.F32, tg.FIR_OVERLAP_SAVE), x, p, bad, p - 4 * N - K, p + K - 1 + 4 * N,
                    f"fir ols K={K}")


@pytest.mark.parametrize("no_direct", [False, True])
@pytest.mark.parametrize("bad", BAD)
@pytest.mark.parametrize("kind,Rr,K", [("decim", 2, 15), ("decim", 4, 63), ("decim", 3, 31), ("half", 2, 31),
                                       ("ups", 2, 15), ("ups", 4, 63), ("ups", 3, 31)])
def test_polyphase(tg, orc, monkeypatch, kind, Rr, K, bad, no_direct):
    """Decimators: output m reads inputs (m+1)R - K ... (m+1)R - 1; upsamplers: outputs jR .. jR + R - 1 read inputs
    j - W + 1 ... j (W = the padded tap count / R).  The direct kernels (decimators of rate 2 / 4 / 8 up to 64 taps,
    upsamplers of rate 2 / 4 up to 32 taps per branch) pad the taps on the old side to KPd = 32 or 64 (branches: 32) and
    multiply the zeros too: the sample reaches KPd - 1 inputs' worth of outputs.  The fused kernel may reach one
    output before libtsd's first."""
    if no_direct:
        monkeypatch.setenv("TSDGPU_POLY_NO_DIRECT", "1")
    c = orc.design_rif_fen(K, "lp", 0.5 / Rr)
    code = {"decim": tg.POLY_DECIM, "half": tg.POLY_HALFBAND, "ups": tg.POLY_UPS}[kind]
    x = rand(300000, False, K)
    direct = not no_direct and (Rr in (2, 4) and -(-K // Rr) <= 32 if kind == "ups" else Rr in (2, 4, 8) and K <= 64)
    for p in POSITIONS:
        if kind == "ups":
            W = 32 if direct else -(-K // Rr)
            lo, hi = p * Rr, (p + W) * Rr - 1
        else:
            KPd = (32 if K <= 32 else 64) if direct else K
            lo, hi = -(-(p + 1) // Rr) - 1 - (0 if direct else 1), (p + KPd) // Rr - 1
        assert_span(lambda: tg.PolyFir(code, tg.F32, c, Rr), x, p, bad, lo, hi, f"{kind} R={Rr} K={K} nodirect={no_direct}",
                    exact=direct)


@pytest.mark.parametrize("bad", BAD)
@pytest.mark.parametrize("ratio,K", [(160 / 147, 15), (0.7, 31), (0.9, 127)])
def test_resampler(tg, orc, ratio, K, bad):
    """Output j reads inputs idx_j - K + 1 ... idx_j of the oracle's schedule."""
    x = rand(300000, True, K)
    _, idx, _ = orc.Resampler(ratio, K).schedule(len(x))
    for p in POSITIONS:
        hit = np.nonzero((idx >= p) & (idx - K + 1 <= p))[0]
        assert_span(lambda: tg.Resampler(ratio, tg.C64, K=K), x, p, bad, int(hit[0]), int(hit[-1]), f"resampler {ratio} K={K}",
                    exact=True)


@pytest.mark.parametrize("bad", BAD)
@pytest.mark.parametrize("n", [1 << 10, 1 << 16, 3 * 1024, 1000])
def test_fft_rows(tg, n, bad):
    """One bad sample in row r of a batch: row r only."""
    import torch
    B = 8
    x = rand(B * n, True, n).reshape(B, n)
    clean = tg.Fft(n, B).step(torch.from_numpy(x).cuda()).cpu().numpy()
    z = x.copy()
    z[5, n // 3] = bad
    y = tg.Fft(n, B).step(torch.from_numpy(z).cuda()).cpu().numpy()
    rows = [r for r in range(B) if not np.array_equal(y[r], clean[r])]
    assert rows == [5] and not np.isfinite(y[5]).all()


def sos_like(make, x, p, bad, what, exact_carry, W):
    """Outputs before p bit-identical, y[p] non-finite.  The exact carry (like libtsd) stays poisoned to the end of the
    stream.  The warm-up path is bit-identical to the clean run again once a chunk has started from zero state after p:
    within 16 W + 8192 outputs (a chunk is at least 4 W long, plus its warm-up; 8192: the shortest chunk layouts).
    reset() clears the handle either way."""
    clean = run(make, x)
    y = run(make, poison(x, p, bad))
    span = diff_span(y, clean)
    print(what, "p", p, bad, "differs over", span, "non-finite", int((~np.isfinite(y)).sum()))
    assert span is not None and span[0] == p and not np.isfinite(y[p])
    if exact_carry:
        assert not np.isfinite(y[p:]).any()
    else:
        assert span[1] < p + 16 * W + 8192 and span[1] < len(y) - 1
    op = make()
    import torch
    op.step(torch.from_numpy(poison(x, p, bad)[: p + 10]).cuda())
    op.reset()
    again = op.step(torch.from_numpy(x[:70000]).cuda()).cpu().numpy()
    assert np.array_equal(again, clean[:70000])


@pytest.mark.parametrize("bad", BAD)
@pytest.mark.parametrize("order,fc,forme,exact_carry", [(12, 0.25, 2, False), (4, 0.02, 1, False), (2, 1e-4, 2, True)])
def test_sos(tg, orc, order, fc, forme, exact_carry, bad):
    z, p_, mn, md = orc.design_butter_lp(order, fc)
    co, gain, r1 = orc.SosChain(z, p_, mn, md, forme=forme).coefs()
    x = rand(300000, False, order)
    W = int(tg.Sos(co, gain, tg.F32, r1, forme=forme).halo)
    for p in (35000, 70000, 70001 + 2047):
        sos_like(lambda: tg.Sos(co, gain, tg.F32, r1, forme=forme), x, p, bad, f"sos {order} {fc} DF{forme} W={W}", exact_carry, W)
