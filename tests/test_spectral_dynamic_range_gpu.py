"""The spectral estimators, the correlations and the detector held to float64 per bin / per row / per sample
(the references and bounds of tests/f64ref.py, checked on the CPU in tests/test_f64ref_cpu.py).

The parity tests elsewhere judge these operators against the loudest value of a call: a weak line 100 dB below the
strong one, a quiet averaging group after a loud one, a score where the stream is quiet are invisible there.  Here

  Welch / Spectrum   |S - P|_k <= sum_s (2 |X_sk| d_s + d_s^2) + gamma(nseg + 4) P_k,  d_s = C_FFT u log2(N) ||w x_s||_2
                     per bin (and per row); Spectrum is judged on linear values, 10^(y/10) - FLT_MIN, with the float32
                     log10's share (ln 10 / 10) 4 ulp32(y) (P + FLT_MIN) added; Bluestein sizes against the reference's
                     own error per bin
  detector           every score inside sqrt(N/M) sqrt2 gamma(M+2) (|h| * |x|) / sqrt(e + 1e-20) + s (gamma(M+3)/2 + 8u)
                     (OLA mode: the engine's normwise bound in place of the componentwise one), the peak list against
                     the definition's
  xcorr              per window of 64 lags at most C_XC times as far from the time-domain definition as libtsd's own
                     float32 run; where L = n + 2m is a power of two also inside 3 C_FFT u log2(L) ||x|| ||y|| / n
  windowed OLA, Rfft test_dynamic_range_gpu.py's normwise bounds (with max|win|), rows and two tones

u = 2^-24; C_FFT and C_REC are test_dynamic_range_gpu.py's.  Every case prints its worst error-to-bound ratio."""
import functools

import numpy as np
import pytest

import f64ref as R
from test_dynamic_range_gpu import C_FFT, C_REC, ragged, stream

pytestmark = pytest.mark.gpu
U = R.U
# xcorr's per-window factor over libtsd's own float32 error (oracle/ola_oracle.py::xcorrb on the oracle's transform).
# Calibration (test_xcorr_calibration_white_noise: white noise, biased, cross-correlation, the shapes of XC_CASES): worst
# per-window ratios max|r_gpu - r64| / max|r_orc - r64| of
#   4.42 at (n, m) = (1024, 512) -- L = 2048, radix-2 on the oracle's side, radix-16 on the device, float32 rounding on both;
#   1.05 (1000, 1000), 1.004 (777, 300), 1.003 (1531, 1531), 1.0003 (65536, 100), 1.001 (2^20, 64) -- off the powers of
#   two both sides carry the reference's float32-chirp Bluestein, which dominates.
# C_XC = 2 x the worst, rounded down (the margin: box-to-box FMA and order differences, as for C_REC).
C_XC = 8.0


@pytest.fixture(scope="module")
def tg():
    import libtsd_amd as t
    assert t.device_count() >= 1
    return t


def hann(N):
    from oracle import ola_oracle
    return ola_oracle.fen_hann_periodique(N) if N > 2 else np.ones(N, np.float32)


def report(what, err, lim):
    """Prints the worst err / limit and asserts err <= lim everywhere."""
    err, lim = np.asarray(err, np.float64), np.asarray(lim, np.float64)
    ratio = np.where(err > 0, err / np.maximum(lim, 1e-300), 0.0)
    print(what, "worst err / bound", float(ratio.max(initial=0.0)))
    bad = np.nonzero(err > lim)
    assert len(bad[0]) == 0, (what, [tuple(int(v[i]) for v in bad) for i in range(min(5, len(bad[0])))], float(ratio.max()))


# ------------------------------------------------------------------------------------------------- Welch
# 16 ... 16384: the fused kernel on the LDS transform; 1024: on the in-wave transform
WELCH_DIRECT = [16, 64, 256, 4096, 16384, 1024]
# 125, 1000, 1001: the wave-level Bluestein kernel; 1025: the reference's float32-chirp Bluestein behind the framed transform;
# 6000 (framed transform + sums): its odd part 375 is a float32-chirp Bluestein too, in the reference and -- by design,
# INTEGRATION.md "Deliberate differences" -- on the device: libtsd's own float32 run sits at 1.63 of welch_parts' bound
# next to the strong line (the device at 1.63 as well), so this size is held to the reference's own error like the others
WELCH_OWN_ERROR = [125, 1000, 1001, 1025, 6000]


@pytest.mark.parametrize("down", [60, 100])
@pytest.mark.parametrize("N", WELCH_DIRECT)
def test_welch_two_tones_per_bin(tg, N, down):
    w = hann(N)
    x = R.two_tone(N, 40 * N + 3, down)
    S, nseg = tg.welch(x, N, w)
    P, B, k = R.welch_parts(x, N, w)
    assert nseg == k == 79
    report(f"welch N={N} -{down} dB", np.abs(S - P), B)


@pytest.mark.parametrize("down", [60, 100])
@pytest.mark.parametrize("N", WELCH_OWN_ERROR)
def test_welch_two_tones_against_the_references_own_error(tg, orc, N, down):
    from oracle import ola_oracle
    w = hann(N)
    x = R.two_tone(N, 40 * N + 3, down)
    S, nseg = tg.welch(x, N, w)
    P, B, k = R.welch_parts(x, N, w)
    So, ko = ola_oracle.psd_welch_sum(x, N, w)
    assert nseg == k == ko == 79
    report(f"welch own error N={N} -{down} dB", np.abs(S - P), C_REC * np.abs(So - P) + 8 * U * P + B / 8)


@pytest.mark.parametrize("N", [64, 1024])
def test_welch_long_resident_call(tg, N):
    """2^21 resident samples: a run holds several segments (per > 1) and a two-stage row sum follows."""
    import torch
    n = 1 << 21
    w = hann(N)
    x = R.two_tone(N, n, 100)
    S, nseg = tg.welch(torch.from_numpy(x).cuda(), N, w)
    P, B, k = R.welch_parts(x, N, w)
    assert nseg == k == (n - N - 1) // (N // 2) + 1
    report(f"welch resident 2^21 N={N}", np.abs(S - P), B)


def test_welch_burst_train(tg):
    N = 256
    x, _, _ = R.burst_train(np.random.default_rng(256), (1 << 16) + 3, N, cplx=True)
    w = hann(N)
    S, nseg = tg.welch(x, N, w)
    P, B, k = R.welch_parts(x, N, w)
    assert nseg == k
    report("welch burst train N=256", np.abs(S - P), B)


@pytest.mark.parametrize("N", [16, 1024, 1000, 6000])
def test_welch_zero_input_gives_exact_zeros(tg, N):
    S, nseg = tg.welch(np.zeros(40 * N + 3, np.complex64), N, hann(N))
    assert nseg == 79 and S.shape == (N,) and (S == 0).all()


# ------------------------------------------------------------------------------------------------- Spectrum
# (BS, nsubs, nmeans, sweep = (step, masque_bf, masque_hf)): the batched plans, the sweep's shifted accumulation, a
# non-power-of-two Nf on the batched plan, and (4099: BS no multiple of nsubs) the block-by-block path
SPEC_SHAPES = [(1024, 1, 3, None), (4096, 4, 2, None), (512, 8, 5, None), (2048, 8, 1, None), (4096, 4, 2, (700, 3, 20)),
               (3000, 3, 2, None), (4099, 4, 2, None)]
# pow2db(0 + FLT_MIN): the float32 nearest to log10(FLT_MIN), times 10 in float32 (numpy's own float32 log10 is an ulp off it)
DB_FLOOR = np.float32(10) * np.float32(np.log10(np.float64(R.FLT_MIN)))


def spec_make(tg, BS, nsubs, nmeans, sweep):
    from oracle import ola_oracle
    ref = ola_oracle.Spectrum(BS, nmeans, nsubs, hann(BS // nsubs), sweep=sweep)         # (the tables only: f, masque, mag_cnt)
    make = lambda: tg.Spectrum(BS, nsubs, nmeans, ref.f, sweep=None if sweep is None else (sweep[0], ref.masque))
    f64 = lambda x: R.spectrum(x, BS, nsubs, nmeans, ref.f, None if sweep is None else sweep[0], ref.masque,
                               getattr(ref, "mag_cnt", None))
    return ref, make, f64


def spec_floor(make, BS, nmeans):
    """What the device gives for a sum of exactly zero: 10 log10(FLT_MIN) exactly, in every bin.  A zero group after a loud
    one must read exactly this too -- anything left of the loud group's sums would show."""
    y = make().step(np.zeros(nmeans * BS, np.complex64))
    assert y.shape[0] == 1 and (y == DB_FLOOR).all(), (y[0, 0], DB_FLOOR)
    return y[0, 0]


def spec_check(what, y, P, B, floor, zero_rows=()):
    assert y.shape == P.shape, (what, y.shape, P.shape)
    lin, lg = R.db_to_linear(y)
    report(what, np.abs(lin - P), B + lg)
    assert (y[P == 0] == floor).all(), what                     # bins nothing reaches (zero groups, the sweep's gaps)
    for r in zero_rows:
        assert (y[r] == floor).all(), (what, r)


@pytest.mark.parametrize("BS,nsubs,nmeans,sweep", SPEC_SHAPES)
def test_spectrum_train_per_row_and_bin(tg, BS, nsubs, nmeans, sweep):
    ref, make, f64 = spec_make(tg, BS, nsubs, nmeans, sweep)
    x = R.spectrum_train(BS, nmeans, BS + nsubs)
    nblocks = len(x) // BS
    assert nblocks == 9 * nmeans
    P, B = f64(x)
    tag = f"spectrum {BS}/{nsubs}/{nmeans} {sweep}"
    floor = spec_floor(make, BS, nmeans)
    # (i) one call
    g = make()
    assert g.Ns == ref.Ns == P.shape[1]
    spec_check(tag + " one call", g.step(x), P, B, floor, (2, 7))
    # (ii) block by block
    g = make()
    rows = [g.step(x[b * BS:(b + 1) * BS]) for b in range(nblocks)]
    assert [len(r) for r in rows] == [1 if (b + 1) % nmeans == 0 else 0 for b in range(nblocks)]
    spec_check(tag + " block by block", np.concatenate(rows), P, B, floor, (2, 7))
    # (iii) ragged calls cut inside groups: the loud first group waits on the device, the next call completes it and
    # the quiet group after it
    g = make()
    rows, b = [], 0
    for k in (max(nmeans - 1, 1), nmeans + 1, 1, 2 * nmeans, max(2 * nmeans - 1, 1), 1, nmeans, 9 * nmeans):
        k = min(k, nblocks - b)
        if k > 0:
            rows.append(g.step(x[b * BS:(b + k) * BS]))
            b += k
    assert b == nblocks and g.pending == 0
    spec_check(tag + " ragged calls", np.concatenate(rows), P, B, floor, (2, 7))


@pytest.mark.parametrize("BS,nsubs,nmeans,sweep", [(4096, 4, 2, None), (512, 8, 5, None), (4096, 4, 2, (700, 3, 20)), (4099, 4, 3, None)])
def test_spectrum_reset_after_a_loud_partial_group(tg, BS, nsubs, nmeans, sweep):
    ref, make, f64 = spec_make(tg, BS, nsubs, nmeans, sweep)
    x = R.spectrum_train(BS, nmeans, 7 * BS)                    # group 0: 1e6, group 1: 1e-3
    g = make()
    assert g.step(x[:(nmeans - 1) * BS]).shape[0] == 0 and g.pending == nmeans - 1
    g.reset()
    assert g.pending == 0
    quiet = x[nmeans * BS:2 * nmeans * BS]
    P, B = f64(quiet)
    spec_check(f"spectrum reset {BS}/{nsubs}/{nmeans} {sweep}", g.step(quiet), P, B, spec_floor(make, BS, nmeans))


# ------------------------------------------------------------------------------------------------- detector
DET_SEED = 1000
DET_THRESHOLD = 0.7


def det_keep(d):
    """Samples whose float64 |c|^2 lies within a factor 4 of the 1e-12 cut are left out of the single-valued judgement:
    either side of the cut is a valid float32 answer there (det_scores_check holds them to the two answers instead)."""
    return ~((d["m2"] > 0.25e-12) & (d["m2"] < 4e-12))


def det_scores_check(tag, sc, d, fir_mode):
    """Every score inside the bound of its sample.  A sample on the cut must still be one of the two valid answers: the
    score with the cut taken (0) or not taken, each within its own bound -- so no sample goes unjudged.  The share of
    samples on the cut is printed; in FIR mode it is asserted (at most 0.1 %; 0 on these streams).  Through the OLA
    engine c is 1 / sqrt(N) of the FIR's: the 1e-3 segments of the burst train then sit on the cut themselves (|c|^2 ~
    2e-6 / N), 0.05 % ... 0.4 % of a stream for N = 1024 ... 8192 whatever the seed -- a property of the float64 scores
    alone, which is why those samples are judged against both answers rather than dropped."""
    keep = det_keep(d)
    share = float(1 - keep.mean())
    print(tag, "on the cut", share, "unjudged", 0.0)
    if fir_mode:
        assert share <= 1e-3
    report(tag + " scores", np.where(keep, np.abs(sc - d["s"]), 0.0), d["bound"])
    e_cut, e_unc = np.abs(sc), np.abs(sc - d["s_uncut"])
    either = np.where(e_cut <= d["bound_cut"], 0.0, e_unc)
    report(tag + " scores on the cut", np.where(keep, 0.0, either), d["bound_uncut"])
    return keep


def det_cases():
    out = []
    for mode in (0, 1):
        for M in (31, 200, 513):
            for Ne in (512, 1024, 4096):
                out.append((mode, M, Ne, False))
    # FIR mode in ragged steps, among them steps shorter than the pattern
    return out + [(1, 31, 1024, True), (1, 200, 1024, True), (1, 513, 1024, True)]


@pytest.mark.parametrize("mode,M,Ne,rag", det_cases())
def test_detector_every_sample(tg, mode, M, Ne, rag):
    """Every score of a 2^17-sample burst train with 40 planted patterns inside the bound of its sample, and the peak list
    against the definition.

    The peaks are checked three ways: (1) the reported list is exactly what the definition gives on the DEVICE's own
    score stream (above the threshold, larger than the M - 1 later scores, not smaller than the M - 1 earlier ones):
    every comparison of the search, at every sample; (2) every peak of the float64 scores whose margin exceeds twice the
    local bound is reported, once, at its place, with s0, s_m1, s_p1 and c0 inside the bounds of their samples; (3) no
    reported peak lies outside the float64 list.  In OLA mode (3) -- and "below the threshold inside exact-zero
    stretches" -- is asserted where the bound resolves the question: there the correlation is an FFT product (in the
    reference too), an exact-zero stretch next to a loud segment holds that block's rounding noise over an energy of
    exactly zero, the bound says so (it is far above the threshold there), and a peak reported at such a sample is a
    valid float32 answer.  In FIR mode both are asserted as they stand: zeros in, zeros out."""
    pat, x, edges, kinds, starts = R.detector_stream(DET_SEED + M, M)
    n = len(x)
    N = 1 if mode == 1 else 1 << int(np.ceil(np.log2(Ne + M - 1)))
    if mode == 0 and 2 * M > N:
        with pytest.raises(tg.TsdGpuError):                      # the pattern does not fit the engine's blocks: no such detector
            tg.Detector(pat, Ne, mode, threshold=DET_THRESHOLD)
        return
    det = tg.Detector(pat, Ne, mode, threshold=DET_THRESHOLD)
    assert det.N == N and det.delay == (Ne if mode == 0 else M - 1)
    if rag:
        rng = np.random.default_rng(M)
        sizes, cuts, o = [2, 3, 17, M - 1, M, M + 1, 1000, 4097, 20000], [], 0
        while o < n:
            c = min(int(rng.choice(sizes)), n - o)
            c = c if n - o - c != 1 else c + 1                   # (a step takes at least 2 samples)
            cuts.append((o, o + c))
            o += c
    else:
        blocks = [1, 3, 2, 7]
        cuts, o, k = [], 0, 0
        while o < n:
            c = min(blocks[k % 4] * Ne, n - o)
            cuts.append((o, o + c))
            o, k = o + c, k + 1
    scores, found = [], []
    for a, b in cuts:
        sc, pk = det.step(x[a:b].copy())
        scores.append(sc)
        found += [(a + p.index, p) for p in pk]
    sc = np.concatenate(scores)
    d = R.detector(R.unit_pattern(pat), x, N, Ne=Ne, threshold=DET_THRESHOLD)
    s64, bound = d["s"], d["bound"]
    tag = f"detector mode={mode} M={M} Ne={Ne} ragged={rag}"
    assert np.isfinite(sc).all()
    keep = det_scores_check(tag, sc, d, mode == 1)
    # (1) the search itself, on the device's own scores
    sp = np.concatenate([np.zeros(M - 1, np.float32), sc])
    own = [int(i) for i in np.nonzero(sc[:n - (M - 1)] > np.float32(DET_THRESHOLD))[0]
           if (sc[i + 1:i + M] < sc[i]).all() and (sp[i:i + M - 1] <= sc[i]).all()]
    idx = [g for g, _ in found]
    assert idx == own, (tag, len(idx), len(own))
    # (2) the definition's certain peaks: reported once, at their place, records inside the bounds
    certain = d["peaks"][d["margins"] > 2 * d["local"]]
    print(tag, "peaks reported", len(idx), "definition", len(d["peaks"]), "certain", len(certain))
    assert len(certain) >= (20 if mode == 1 else 8) and len(set(idx)) == len(idx)
    assert set(certain) <= set(idx), (tag, sorted(set(certain) - set(idx))[:5])
    for g, p in found:
        if g in set(certain):
            assert abs(p.s0 - s64[g]) <= bound[g] and p.s0 == sc[g]
            assert abs(p.s_m1 - s64[g - 1]) <= bound[g - 1] or not keep[g - 1]
            assert abs(p.s_p1 - s64[g + 1]) <= bound[g + 1] or not keep[g + 1]
            assert abs(complex(*p.c0) - d["c"][g]) <= d["cb"][g] + 8 * U * abs(d["c"][g])
    # (3) nothing reported outside the definition's list; the first windows and the exact-zero stretches stay below the threshold
    zero = np.zeros(n, bool)
    D = det.delay - (M - 1)
    for (a, b), kd in zip(zip(edges[:-1], edges[1:]), kinds):
        if kd == "zero" and b - a > M:
            zero[a + M - 1 + D:b + D] = True                     # windows that hold nothing but zeros ...
    for s in starts:
        zero[max(s + D, 0):s + 2 * M + D] = False                # ... and no planted pattern
    zero = zero[:n]
    first = np.zeros(n, bool)
    first[D:D + M] = True
    first &= s64 + bound < DET_THRESHOLD
    outside = sorted(set(idx) - set(int(i) for i in d["peaks"]))
    if mode == 1:
        assert outside == [], (tag, outside[:5])
        assert (sc[zero] == 0).all() and (sc[first] < DET_THRESHOLD).all()
    else:
        resolved = s64 + bound < DET_THRESHOLD
        assert not any(resolved[g] for g in outside), (tag, outside[:5])
        assert (sc[zero & resolved] < DET_THRESHOLD).all() and (sc[first] < DET_THRESHOLD).all()


# ------------------------------------------------------------------------------------------------- xcorr, delay_estimate
XC_CASES = [(1024, 512), (1000, 1000), (777, 300), (1531, 1531), (65536, 100), (1 << 20, 64)]
XC_KINDS = ["white", "half80", "quietloud"]


def xcorr_inputs(n, kind):
    """white noise; x's second half 80 dB down; x quiet (1e-3) against y loud (1e6)."""
    rng = np.random.default_rng(n + 7 * XC_KINDS.index(kind))
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    y = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    if kind == "half80":
        x[n // 2:] *= 1e-4
    if kind == "quietloud":
        x, y = x * 1e-3, y * 1e6
    return x.astype(np.complex64), y.astype(np.complex64)


def xcorr_flat_bound(x, y, n, m):
    """L = n + 2m a power of two (radix-2 plans on both sides): 3 C_FFT u log2(L) ||x|| ||y|| / n."""
    L = n + 2 * m
    return 3 * C_FFT * U * np.log2(L) * np.linalg.norm(x.astype(np.complex128)) * np.linalg.norm(y.astype(np.complex128)) / n


@functools.lru_cache(maxsize=None)
def xcorr_refs(n, m, kind, auto):
    """(x, y, float64 biased lags, the oracle's float32 biased lags) -- computed once per case."""
    from oracle import ola_oracle
    x, y = xcorr_inputs(n, kind)
    if auto:
        y = x
    r64 = R.xcorr(x, None if auto else y, m)
    ro = ola_oracle.xcorrb(x, None if auto else y, m)[1]
    for v in (x, y, r64, ro):
        v.setflags(write=False)
    return x, y, r64, ro


def window_max(v, size=64):
    v = np.abs(v)
    return np.array([v[a:a + size].max() for a in range(0, len(v), size)])


def xcorr_ratio(r, r64, ro):
    return float((window_max(r - r64) / np.maximum(window_max(ro - r64), 1e-300)).max())


@pytest.mark.parametrize("n,m", XC_CASES)
def test_xcorr_calibration_white_noise(tg, n, m):
    """White noise, biased, cross-correlation: the ratios that fix C_XC (recorded beside it)."""
    x, y, r64, ro = xcorr_refs(n, m, "white", False)
    r = tg.xcorr(x, y, m, False)
    ratio = xcorr_ratio(r, r64, ro)
    print("xcorr calibration", n, m, "worst per-window ratio to libtsd's own error", ratio)
    assert ratio <= C_XC


# (beyond n = 65536 the oracle leg is slow and runs once: white noise, cross-correlation)
XC_PARAMS = [(n, m, kind, auto) for n, m in XC_CASES for kind in XC_KINDS for auto in (False, True)
             if n <= 65536 or (kind == "white" and not auto)]


@pytest.mark.parametrize("n,m,kind,auto", XC_PARAMS)
def test_xcorr_per_window(tg, n, m, kind, auto):
    import torch
    x, y, r64, ro = xcorr_refs(n, m, kind, auto)
    w = R.xcorr_weights(n, m)
    L = n + 2 * m
    for unbiased in (False, True):
        for resident in (False, True):
            if resident:
                xd = torch.from_numpy(np.array(x)).cuda()
                r = tg.xcorr(xd, None if auto else torch.from_numpy(np.array(y)).cuda(), m, unbiased).cpu().numpy()
            else:
                r = tg.xcorr(x, None if auto else y, m, unbiased)
            ref = r64 / w if unbiased else r64
            orc_ = ro / w if unbiased else ro
            what = f"xcorr n={n} m={m} {kind} auto={auto} unbiased={unbiased} resident={resident}"
            report(what, window_max(r - ref), C_XC * window_max(orc_ - ref) + 8 * U * window_max(ref))
            if L & (L - 1) == 0:
                flat = xcorr_flat_bound(x, y, n, m)
                report(what + " flat", np.abs(r - ref) * (w if unbiased else 1.0), flat + 8 * U * np.abs(r64))


@pytest.mark.parametrize("n,d", [(4096, 0), (4096, 3), (4096, -100), (1 << 18, 1000)])
def test_delay_estimate_and_amplitude_pair(tg, n, d):
    from oracle import ola_oracle as oo
    rng = np.random.default_rng(n + d)
    base = (rng.standard_normal(n + 4096) + 1j * rng.standard_normal(n + 4096)).astype(np.complex64)
    x = base[2048:2048 + n].copy()
    y = base[2048 - d:2048 - d + n].copy()                      # y = x delayed by d samples
    delay, score = tg.delay_estimate(x, y)
    rd, rs = oo.estimation_delais(x, y)
    print("delay_estimate", n, d, delay, score, rd, rs)
    assert abs(delay - rd) <= 1e-3 and abs(score - rs) <= 1e-4
    assert abs(delay - d) <= 0.5 and score > 0.5
    xq, yl = (x * np.float32(1e-3)).astype(np.complex64), (y * np.float32(1e6)).astype(np.complex64)
    d2, s2 = tg.delay_estimate(xq, yl)
    rd2, rs2 = oo.estimation_delais(xq, yl)
    assert abs(d2 - rd2) <= 1e-3 and abs(s2 - rs2) <= 1e-4
    assert abs(s2 - score) <= 1e-5 and abs(d2 - delay) <= 1e-3


# ------------------------------------------------------------------------------------------------- windowed OLA, Rfft
def ola_response(orc, N, M=33):
    """FiltreFFTRIF's H (fourier.cc:963-966) for a 33-tap low-pass, as test_ola_engine builds it."""
    h = orc.design_rif_fen(M, "lp", 0.05)
    h2 = np.zeros(N, np.complex64)
    h2[N - M:] = h
    return (orc.fft(h2, True) * np.float32(np.sqrt(N))).astype(np.complex64)


def ola_w_input(Ne, N):
    n = Ne * max(60, 32768 // Ne)
    return R.burst_train(np.random.default_rng(Ne + N), n, N, True)[0]


def ola_w_bound(x, N, H, win):
    """test_ola_engine's normwise bound with max|win| in it: output t reads the inputs [t - 2 Ne, t + 2 Ne]."""
    return C_FFT * U * np.log2(N) * np.abs(H.astype(np.complex128)).max() * float(np.abs(win).max()) * R.window_norm(x, 2 * N)


@pytest.mark.parametrize("Ne,nz", [(512, 127), (64, 64), (1000, 24), (4096, 0)])
def test_ola_windowed(tg, orc, Ne, nz):
    win = hann(Ne)
    o = tg.Ola(Ne, nz, win)
    N = o.N
    H = ola_response(orc, N)
    o.set_response(H)
    x = ola_w_input(Ne, N)
    rng = np.random.default_rng(Ne)
    y = stream(o.step, x, ragged(rng, len(x)))
    ref = R.ola_windowed(x, Ne, N, H, win)
    assert len(y) == len(ref) == len(x) - Ne
    report(f"windowed ola {Ne} {nz}", np.abs(y - ref), ola_w_bound(x, N, H, win)[: len(ref)])


@pytest.mark.parametrize("n", [1024, 4096, 6144, 32768, 1000])
def test_rfft_rows_and_two_tone(tg, orc, n):
    """test_fft_plans_rows_and_two_tone on RTFRPlan: rows loud, quiet or zero, each held to its own norm (a zero row stays
    exactly zero); two real tones 100 dB apart.  1000 (the reference's float32-chirp Bluestein): the "own error" form."""
    import torch
    rng = np.random.default_rng(n)
    amps = np.array([1e6, 1.0, 0.0, 1e-3, 1e4, 1.0, 0.0, 1e-3])
    x = (rng.standard_normal((8, n)) * amps[:, None]).astype(np.float32)
    y = tg.Rfft(n).step(torch.from_numpy(x).cuda()).cpu().numpy()
    ref = R.rfft(x)
    t = np.arange(n)
    k1, k2 = n // 7, n // 3 + 1
    xt = (np.cos(2 * np.pi * k1 * t / n) + 1e-5 * np.cos(2 * np.pi * k2 * t / n)).astype(np.float32)
    yt = tg.Rfft(n).step(xt[None, :].copy())[0]
    rt = R.rfft(xt)
    assert (y[amps == 0] == 0).all()
    if n != 1000:
        bound = C_FFT * U * np.log2(n) * np.linalg.norm(x.astype(np.float64), axis=1)
        report(f"rfft {n} rows", np.abs(y - ref).max(axis=1), bound)
        report(f"rfft {n} two tones", np.abs(yt - rt), C_FFT * U * np.log2(n) * np.linalg.norm(xt.astype(np.float64)))
    else:
        yo = np.stack([orc.rfft(r) for r in x])
        report(f"rfft {n} rows", np.abs(y - ref).max(axis=1), C_REC * np.abs(yo - ref).max(axis=1) + 8 * U * np.abs(ref).max(axis=1))
        yto = orc.rfft(xt)
        for sl in (slice(k2 - 2, k2 + 3), slice(0, n)):
            eg, eo = np.abs(yt[sl] - rt[sl]).max(), np.abs(yto[sl] - rt[sl]).max()
            print("rfft 1000 two tones", sl, eg, eo)
            assert eg <= C_REC * eo + 8 * U * np.abs(rt[sl]).max()
