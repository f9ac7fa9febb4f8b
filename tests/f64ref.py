"""Float64 statements of the linear operators, written from their definitions (numpy / scipy), and the error
measures the dynamic-range tests use.  Test helper, not a conftest: the inputs and coefficients are the float32
values the GPU receives, widened to float64, so what is left between a kernel and these references is the
kernel's own arithmetic.

Definitions (libtsd's conventions, restated):
  FIR          y[n] = sum_k h[k] x[n-k], zero history
  decimator    FiltreRIFDecim: the taps applied un-reversed to the window ending at input j, one output per R
               inputs, the first at j = R-1; the half-band stage keeps the even taps plus 0.5 x the centre sample
  upsampler    FiltreRIFUps: taps scaled by R, zero-padded to a multiple of R; output i of input j reads the
               window of the last K/R inputs against taps R-1-i, 2R-1-i, ...
  SOS          sections in series, each seeded with its own first input (DF2: both memories = x0; DF1: x1 = x2 =
               y1 = y2 = x0), then the gain or a trailing first-order section from zero state
  FiltreRII    lfilter(numer, denom) from zero state
  resampler    y[j] = sum_t lut[col_j, t] x[idx_j - K + 1 + t] over the (index, phase) schedule
  FFT          unitary: 1/sqrt(n) both ways
  OLA          block b (Ne inputs after Nz zeros) -> ifft(fft(block) H), added at output b Ne + Ne - Nz
  Welch        sum over segments i = 0, N/2, ... (i + N < len) of fftshift(|fft(w x_i)|^2 / N)
"""
import numpy as np
from scipy.signal import lfilter, lfiltic

U = 2.0 ** -24          # unit roundoff of float32


def gamma(m):
    """Wilkinson's gamma_m = m u / (1 - m u): the componentwise bound of an m-term float32 dot product."""
    return m * U / (1.0 - m * U)


def w64(a):
    a = np.asarray(a)
    return a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)


# ------------------------------------------------------------------------------------------------- FIR family
def fir(h, x):
    x = w64(x)
    return np.convolve(w64(h), x)[: len(x)]


def decim(c, x, R, halfband=False):
    c = w64(np.asarray(c, np.float32))
    if halfband:
        R = 2
        c = c.copy()
        c[1::2] = 0
        c[len(c) // 2] += 0.5
    full = np.convolve(c[::-1], w64(x))[: len(x)]
    return full[R - 1:: R]


def ups_taps(c, R):
    """The upsampler's padded taps (float32 products c R, as libtsd stores them)."""
    c = (np.asarray(c, np.float32) * np.float32(R)).astype(np.float32)
    return np.concatenate([c, np.zeros((-len(c)) % R, np.float32)])


def ups(c, x, R):
    cp = w64(ups_taps(c, R))
    x = w64(x)
    W = len(cp) // R
    y = np.zeros(len(x) * R, x.dtype)
    for i in range(R):
        ci = cp[R - 1 - i:: R][:W]                    # tap t of phase i: cp[R-1-i + tR], against x[j-W+1+t]
        y[i::R] = np.convolve(ci[::-1], x)[: len(x)]
    return y


# ------------------------------------------------------------------------------------------------- recursions
def _df2_section(sec, v):
    b0, b1, b2, a1, a2 = sec
    x0 = v[0]
    zi = lfiltic([1.0], [1.0, a1, a2], y=[x0, x0])
    d, _ = lfilter([1.0], [1.0, a1, a2], v, zi=zi.astype(v.dtype))
    dd = np.concatenate([[x0, x0], d])
    return b0 * dd[2:] + b1 * dd[1:-1] + b2 * dd[:-2]


def _df1_section(sec, v):
    b0, b1, b2, a1, a2 = sec
    x0 = v[0]
    zi = lfiltic([b0, b1, b2], [1.0, a1, a2], y=[x0, x0], x=[x0, x0])
    out, _ = lfilter([b0, b1, b2], [1.0, a1, a2], v, zi=zi.astype(v.dtype))
    return out


def _sos_real(coefs, gain, rii1, v, forme):
    step = _df1_section if forme == 1 else _df2_section
    for sec in w64(np.asarray(coefs, np.float32)).reshape(-1, 5):
        v = step(sec, v)
    if rii1 is not None:
        q = w64(np.asarray(rii1, np.float32))
        return lfilter([q[0], q[1]], [1.0, q[2]], v)
    return v * float(np.float32(gain))


def sos(coefs, gain, rii1, x, forme=2):
    """ChaineSOIS over the whole stream (the seeds act on the first sample only); complex data = two real channels."""
    if len(x) == 0:
        return np.zeros(0)
    if np.iscomplexobj(x):
        return _sos_real(coefs, gain, rii1, np.real(x).astype(np.float64), forme) + \
            1j * _sos_real(coefs, gain, rii1, np.imag(x).astype(np.float64), forme)
    return _sos_real(coefs, gain, rii1, w64(x), forme)


def rii(numer, denom, x):
    return lfilter(w64(numer), w64(denom), w64(x))


def rii_bound(numer, denom, x, y64):
    """First-order componentwise bound of ANY float32 evaluation of FiltreRII's literal recursion
    y_n = (num_n - sum_k d_k y_{n-k}) / d_0, num = numer * x:  every step rounds its terms with a relative error of at most
    gamma_m (m = the numerator's and the denominator's terms), so it injects delta_m <= gamma_m (|numer| * |x| + |d| * |y|)_m
    / |d_0| (plus m 2^-150 once the values are subnormal), and the injected errors reach the output through the recursion's impulse response g (1 / A(z)):
    |y - y64|_n <= (|g| * delta)_n.  No rounding realisation is singled out: libtsd's order, with or without FMA, and any
    other order satisfy it (tests/test_f64ref_cpu.py checks the oracle's)."""
    nu, de = np.abs(w64(numer)), w64(denom)
    m = len(nu) + len(de) + 1
    ya = np.abs(w64(y64))
    rho = absconv(nu, np.abs(w64(x))) + np.convolve(np.abs(de[1:]), np.concatenate([[0.0], ya]))[: len(ya)]
    # + the absolute error of a gradual underflow (half the subnormal spacing per rounded term) where the tail gets that small
    delta = (gamma(m) * rho + m * 2.0 ** -150) / abs(de[0])
    imp = np.zeros(1 << 16)
    imp[0] = 1.0
    g = np.abs(lfilter([1.0], de / de[0], imp))
    L = int(np.nonzero(g > 1e-17 * g.max())[0][-1]) + 1
    return np.convolve(g[:L], delta)[: len(delta)]


# ------------------------------------------------------------------------------------------------- resampler
def resample(lut, idx, col, x):
    """The float64 sum of float32 LUT rows x samples over a given (input index, LUT row) schedule."""
    lut = w64(np.asarray(lut, np.float32))
    K = lut.shape[1]
    x = w64(x)
    xp = np.concatenate([np.zeros(K - 1, x.dtype), x])
    win = np.lib.stride_tricks.sliding_window_view(xp, K)          # win[i] = x[i-K+1 .. i]
    return np.einsum("jt,jt->j", lut[col], win[idx])


def resample_bound(lut, idx, col, x):
    """sum_t |lut[col_j, t]| |x[idx_j - K + 1 + t]|: the componentwise scale of each output."""
    lut = np.abs(w64(np.asarray(lut, np.float32)))
    K = lut.shape[1]
    xp = np.concatenate([np.zeros(K - 1), np.abs(w64(x))])
    win = np.lib.stride_tricks.sliding_window_view(xp, K)
    return np.einsum("jt,jt->j", lut[col], win[idx])


# ------------------------------------------------------------------------------------------------- FFT family
def fft(x, forward=True):
    x = w64(x)
    n = x.shape[-1]
    return np.fft.fft(x, axis=-1) / np.sqrt(n) if forward else np.fft.ifft(x, axis=-1) * np.sqrt(n)


def ola(x, Ne, N, H):
    """OLA engine without window, with response H (length N): the whole-block outputs of len(x) inputs."""
    x = w64(np.asarray(x, np.complex64))
    H = w64(np.asarray(H, np.complex64))
    Nz = N - Ne
    B = len(x) // Ne
    y = np.zeros((B + 2) * Ne + N, np.complex128)
    for b in range(B):
        p = np.zeros(N, np.complex128)
        p[Nz:] = x[b * Ne:(b + 1) * Ne]
        o = b * Ne + Ne - Nz
        y[o:o + N] += np.fft.ifft(np.fft.fft(p) * H)
    return y[: B * Ne]


def welch_sum(x, N, window):
    x = w64(np.asarray(x, np.complex64))
    w = w64(np.asarray(window, np.float32))
    starts = np.arange(0, max(len(x) - N, 0), max(N // 2, 1))
    if len(starts) == 0:
        return np.zeros(N), 0
    segs = np.lib.stride_tricks.sliding_window_view(x, N)[starts] * w
    P = np.abs(np.fft.fft(segs, axis=-1)) ** 2 / N
    return np.fft.fftshift(P.sum(axis=0)), len(starts)


# ------------------------------------------------------------------------------------------------- error measures
def region_err(y, ref, edges):
    """Per region [edges[i], edges[i+1]): (max|y - ref|, max|ref|) as two arrays."""
    y, ref = np.asarray(y), np.asarray(ref)
    err = np.empty(len(edges) - 1)
    mag = np.empty(len(edges) - 1)
    for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        err[i] = np.abs(y[a:b] - ref[a:b]).max() if b > a else 0.0
        mag[i] = np.abs(ref[a:b]).max() if b > a else 0.0
    return err, mag


def absconv(habs, xabs):
    """(|h| * |x|)_i over the first len(x) outputs: the componentwise bound's scale."""
    return np.convolve(np.abs(w64(habs)), np.abs(w64(xabs)))[: len(xabs)]


def window_norm(x, N):
    """An upper bound of ||x[i-N+1 : i+N]||_2 for every i (zero outside the vector): the norm over the N-sample blocks
    that window touches (at most 4N samples).  Block sums, not a running cumulative sum: at 120 dB of dynamic range a
    cumulative sum cancels the quiet blocks away."""
    e = np.abs(w64(x)) ** 2
    n = len(e)
    nb = -(-n // N)
    bs = np.zeros(nb + 2)
    bs[1:nb + 1] = np.pad(e, (0, nb * N - n)).reshape(nb, N).sum(axis=1)
    i = np.arange(n)
    lo, hi = np.maximum(i - N + 1, 0) // N, np.minimum(i + N, n - 1) // N      # first / last block touched
    # at most four blocks: sum them directly (no cancellation)
    tot = np.zeros(n)
    for k in range(4):
        b = lo + k
        tot += np.where(b <= hi, bs[np.minimum(b, nb - 1) + 1], 0.0)
    return np.sqrt(tot)


def windows(edges, n, maxlen=2048):
    """The segment edges split further so that no window holds more than maxlen outputs."""
    out = [0]
    for a, b in zip(list(edges[:-1]) + [edges[-1]], list(edges[1:]) + [n]):
        a, b = min(a, n), min(b, n)
        while a < b:
            a = min(b, a + maxlen)
            out.append(a)
    return np.unique(np.array(out))


def burst_train(rng, n, wmax, cplx=False, loud=(1e4, 1e6), quiet=(1.0, 1e-3), lo=300, hi=None):
    """Seeded burst train: loud segments, quiet segments, exact-zero stretches, of random lengths between about 300
    and 3 wmax (`lo`, `hi`: other limits, for streams too short for those).
    -> (x float32/complex64, segment edges, kinds) with kinds in {"loud", "quiet", "zero"}."""
    edges, kinds, amps = [0], [], []
    o = 0
    hi = max(600, 3 * int(wmax)) if hi is None else int(hi)
    while o < n:
        L = int(rng.integers(lo, hi))
        r = rng.random()
        if r < 0.3:
            k, a = "loud", float(rng.choice(loud))
        elif r < 0.85:
            k, a = "quiet", float(rng.choice(quiet))
        else:
            k, a = "zero", 0.0
        o = min(n, o + L)
        edges.append(o)
        kinds.append(k)
        amps.append(a)
    x = np.zeros(n, np.complex128 if cplx else np.float64)
    for (a, b), amp in zip(zip(edges[:-1], edges[1:]), amps):
        v = rng.standard_normal(b - a)
        if cplx:
            v = v + 1j * rng.standard_normal(b - a)
        x[a:b] = amp * v
    return x.astype(np.complex64 if cplx else np.float32), np.array(edges), kinds


# ------------------------------------------------------------------------------------------------- spectral estimators
# Definitions (libtsd's conventions, restated):
#   Spectrum     rt_spectrum: blocks of BS samples, nsubs sub-blocks of Nf = BS // nsubs (the trailing samples dropped),
#                each windowed with the normalised window f, transformed (unitary), |.|^2, fftshift; summed over nmeans
#                blocks (sweep, nsubs > 1: sub-block i masked and added `step` bins further), divided by nmeans nsubs Nf
#                (sweep: and by the contributions mag_cnt); the device returns 10 log10(. + FLT_MIN)
#   xcorr        r[lag] = sum_t x[t] conj(y[t + lag]) / n, lags -(m-1) .. (m-1); unbiased: / ((n - |lag|) / n)
#   detector     c = x filtered by the conjugated reversed unit-energy pattern (/ sqrt(N) through the OLA engine),
#                e = M-tap moving average of |x|^2, s = sqrt(N/M) sqrt(|c|^2 / (e + 1e-20)), c = 0 where |c|^2 <= 1e-12
#   windowed OLA OLA<cfloat>::step_interne's windowed branch (two half-overlapped frames per block, each weighted 1/2)
FLT_MIN = float(np.finfo(np.float32).tiny)


def c_fft():
    """The normwise FFT constant of tests/test_dynamic_range_gpu.py (one definition; imported late: that module imports this one)."""
    from test_dynamic_range_gpu import C_FFT
    return C_FFT


def _lg(N):
    return max(np.log2(N), 1.0)


def _periodograms(segs, N):
    """Rows of windowed segments -> (|X|^2 of the unitary transform, the per-bin bound 2 |X| d + d^2 of a float32 transform
    whose output is within d = C_FFT u log2(N) ||segment||_2 of X: | |X + e|^2 - |X|^2 | <= 2 |X| |e| + |e|^2)."""
    X = np.fft.fft(segs, axis=-1) / np.sqrt(N)
    d = c_fft() * U * _lg(N) * np.linalg.norm(segs, axis=-1)[..., None]
    Xa = np.abs(X)
    return Xa * Xa, 2 * Xa * d + d * d


def welch_parts(x, N, w):
    """-> (P[k], bound[k], nseg) in fftshift order.  bound_k = sum_s (2 |X_sk| d_s + d_s^2) + gamma(nseg + 4) P_k: every
    segment's transform normwise, then |.|^2 (3 roundings), the nseg-term sum of non-negative terms and one more rounding."""
    x = w64(np.asarray(x, np.complex64))
    w = w64(np.asarray(w, np.float32))
    starts = np.arange(0, max(len(x) - N, 0), max(N // 2, 1))
    if len(starts) == 0:
        return np.zeros(N), np.zeros(N), 0
    P, B = np.zeros(N), np.zeros(N)
    view = np.lib.stride_tricks.sliding_window_view(x, N)
    for a in range(0, len(starts), 4096):                         # (chunks: 65535 segments of 64 need not sit in memory at once)
        p, b = _periodograms(view[starts[a:a + 4096]] * w, N)
        P += p.sum(axis=0)
        B += b.sum(axis=0)
    B += gamma(len(starts) + 4) * P
    h = N // 2
    sh = lambda v: np.concatenate([v[N - h:], v[:N - h]])         # fftshift as fourier.hpp:232-248 (odd N too)
    return sh(P), sh(B), len(starts)


def spectrum(x, BS, nsubs, nmeans, f, sweep=None, masque=None, mag_cnt=None):
    """rt_spectrum in float64 over whole blocks: -> (P[rows, Ns] linear (before + FLT_MIN and the dB), bound[rows, Ns]).
    f: the oracle's normalised float32 window (Spectrum.f); sweep: the step in bins or None; masque / mag_cnt: the
    oracle's float32 tables.  nsubs == 1 takes the reference's branch without masque.  Bins nothing reaches: P = bound = 0."""
    x = w64(np.asarray(x, np.complex64))
    f = w64(np.asarray(f, np.float32))
    Nf = BS // nsubs
    h = Nf // 2
    shifted = sweep is not None and nsubs > 1
    step = int(sweep) if shifted else 0
    Ns = Nf + (nsubs - 1) * step
    mk = w64(np.asarray(masque, np.float32)) if shifted else np.ones(Nf)
    rows = (len(x) // BS) // nmeans
    P, B = np.zeros((rows, Ns)), np.zeros((rows, Ns))
    for r in range(rows):
        blk = x[r * nmeans * BS:(r + 1) * nmeans * BS].reshape(nmeans, BS)[:, :nsubs * Nf].reshape(nmeans, nsubs, Nf)
        p, b = _periodograms(blk * f, Nf)
        p = np.concatenate([p[..., Nf - h:], p[..., :Nf - h]], axis=-1).sum(axis=0)
        b = np.concatenate([b[..., Nf - h:], b[..., :Nf - h]], axis=-1).sum(axis=0)
        for i in range(nsubs):
            P[r, i * step:i * step + Nf] += p[i] * mk
            B[r, i * step:i * step + Nf] += b[i] * mk
    div = float(nmeans * nsubs * Nf)
    if sweep is not None:
        div = div * w64(np.asarray(mag_cnt, np.float32))
    P, B = P / div, B / div
    return P, B + gamma(nmeans * nsubs + 4) * P


def spectrum_train(BS, nmeans, seed, amps=(1e6, 1e-3, 0.0, 1.0, 1e4, 1e-3, 1e6, 0.0, 1.0), nf=None):
    """Nine averaging groups (nmeans blocks of BS each) of these amplitudes: complex noise plus a line ten times as
    strong, on another frequency in every group.  A zero group is exact zeros."""
    rng = np.random.default_rng(seed)
    L = nmeans * BS
    t = np.arange(L)
    out = []
    for g, a in enumerate(amps):
        v = rng.standard_normal(L) + 1j * rng.standard_normal(L)
        fr = (0.05 + 0.09 * g) - 0.5
        out.append(a * (v + 10 * np.exp(2j * np.pi * fr * t)))
    return np.concatenate(out).astype(np.complex64)


def db_to_linear(y):
    """The device's dB rows back to linear values and the float32 log10's share of the limit, per bin:
    10^(y/10) - FLT_MIN, and (ln 10 / 10) 4 ulp32(y) 10^(y/10)."""
    y = np.asarray(y, np.float32)
    lin = 10.0 ** (y.astype(np.float64) / 10)
    return lin - FLT_MIN, (np.log(10.0) / 10) * 4 * np.spacing(np.abs(y)).astype(np.float64) * lin


def two_tone(N, n, down_db, k1=None, k2=None):
    """1e3 on bin N // 8 plus a tone down_db below it on bin N // 3 + 1 (exact bins of every hop-N//2 segment)."""
    t = np.arange(n)
    k1 = N // 8 if k1 is None else k1
    k2 = N // 3 + 1 if k2 is None else k2
    return (1e3 * np.exp(2j * np.pi * k1 * t / N) + 1e3 * 10 ** (-down_db / 20) * np.exp(2j * np.pi * k2 * t / N)).astype(np.complex64)


# ------------------------------------------------------------------------------------------------- correlations
def xcorr(x, y=None, m=-1, unbiased=False):
    """The time-domain definition in the oracle's lag order: with c = np.correlate(x, y, "full"),
    c[::-1][n-1-(m-1) : n-1+m] / n, i.e. r[lag] = sum_t x[t] conj(y[t + lag]) / n (one dot product per lag)."""
    x = w64(np.asarray(x, np.complex64))
    y = x if y is None else w64(np.asarray(y, np.complex64))
    n = len(x)
    if m < 0:
        m = n
    r = np.empty(2 * m - 1, np.complex128)
    for i, lag in enumerate(range(-(m - 1), m)):
        r[i] = np.vdot(y[lag:], x[:n - lag]) if lag >= 0 else np.vdot(y[:n + lag], x[-lag:])
    r /= n
    return r / xcorr_weights(n, m) if unbiased else r


def xcorr_weights(n, m):
    """(n - |lag|) / n over the lags -(m-1) .. (m-1)."""
    return (n - np.abs(np.arange(-(m - 1), m))) / float(n)


# ------------------------------------------------------------------------------------------------- detector
def detector(pattern_unit, x, mode_N=1, Ne=None, threshold=0.5):
    """The detector's score stream from its definition, in the stream's own time (score index i of the device):
    mode_N = 1: FIR mode (delay M - 1); mode_N = N > 1: the OLA engine of block Ne and transform N (delay Ne, c / sqrt(N)).
    -> dict(s, c, e, bound, peaks, margins, local, ...): s, c, e, bound per sample (s_uncut / bound_uncut, bound_cut: the
    score and the bounds of the two answers at a sample on the 1e-12 cut -- cut not taken, cut taken and s = 0); peaks: the indices i that the definition
    makes peaks (s[i] > threshold, > the M - 1 later scores, >= the M - 1 earlier ones; scores before the stream are 0;
    decided only where the M - 1 later scores exist); margins: per peak the smallest gap to the threshold and to those
    neighbours; local: per peak the largest bound over the samples compared.

    bound (FIR mode) = sqrt(N/M) sqrt2 gamma(M+2) (|h| * |x|) / sqrt(e + 1e-20) + s (gamma(M+3) / 2 + 8u):
      the M-term complex dot product componentwise (sqrt2: complex x complex products), divided by the exact sqrt(e);
      e is a float32 sum of M non-negative terms of |x|^2 (2 roundings) times the tap (1): relative gamma(M+3), halved by
      the square root; 8u for |c|^2, the division, sqrtf and the float32 ratio.
    OLA mode: the correlation term is test_ola_engine's normwise bound, C_FFT u log2(N) max|H| ||x[t-2N+1 : t+2N]||_2
      (H = conj(FFT(pattern)) / sqrt(N), the response the engine multiplies with; its own float32 rounding, u log2(N)
      per bin relative to max|H|, sits inside C_FFT's margin over the classical constant)."""
    p = w64(np.asarray(pattern_unit, np.complex64))
    x = w64(np.asarray(x, np.complex64))
    M, n = len(p), len(x)
    h = np.conj(p[::-1])
    cf = np.convolve(h, x)[:n]                                    # FIR time: index = pattern start + M - 1
    xa = np.abs(x)
    tap = float(np.float32(1.0 / M))
    ef = np.convolve(np.full(M, tap), xa * xa)[:n]
    if mode_N > 1:
        D = Ne - (M - 1)
        sh = lambda v: np.concatenate([np.zeros(D, v.dtype), v[:n - D]])
        c, e = sh(cf) / np.sqrt(mode_N), sh(ef)
        Hmax = np.abs(np.fft.fft(p, mode_N)).max() / np.sqrt(mode_N)
        cb = c_fft() * U * np.log2(mode_N) * Hmax * window_norm(x, 2 * mode_N)       # (before the delay too: the first block's noise)
    else:
        c, e = cf, ef
        cb = np.sqrt(2.0) * gamma(M + 2) * np.convolve(np.abs(h), xa)[:n]
    m2 = np.abs(c) ** 2
    cut = m2 <= 1e-12
    c = np.where(cut, 0.0, c)
    ratio = np.sqrt(mode_N / M)
    su = ratio * np.sqrt(m2 / (e + 1e-20))                        # the score had the cut not been taken
    s = np.where(cut, 0.0, su)
    b0 = ratio * cb / np.sqrt(e + 1e-20)
    bound = b0 + s * (gamma(M + 3) / 2 + 8 * U)
    bound_u = b0 + su * (gamma(M + 3) / 2 + 8 * U)
    # the definition's peaks
    sp = np.concatenate([np.zeros(M - 1), s])                     # sp[i + M - 1] = s[i]
    bp = np.concatenate([np.zeros(M - 1), bound])
    peaks, margins, local = [], [], []
    for i in np.nonzero(s[:max(n - (M - 1), 0)] > threshold)[0]:
        later, earlier = s[i + 1:i + M], sp[i:i + M - 1]
        if (later < s[i]).all() and (earlier <= s[i]).all():
            peaks.append(int(i))
            margins.append(float(min(s[i] - threshold, s[i] - later.max(), s[i] - earlier.max())))
            local.append(float(max(bound[i:i + M].max(), bp[i:i + M - 1].max())))
    return dict(s=s, c=c, e=e, bound=bound, m2=m2, cb=cb, s_uncut=su, bound_uncut=bound_u, bound_cut=b0, peaks=np.array(peaks, int), margins=np.array(margins), local=np.array(local))


def detector_stream(seed, M, n=1 << 17, wmax=1024, count=40, borders=(512, 1024, 4096)):
    """burst_train(rng, n, wmax, cplx=True) with `count` copies of a random pattern planted at three times the local
    amplitude (1e-2 inside zero stretches): some at random places, some straddling segment edges, some across the block
    borders of every Ne of the tests.  -> (pattern complex64 (raw, not normalised), x complex64, edges, kinds, starts)."""
    rng = np.random.default_rng(seed)
    x, edges, kinds = burst_train(rng, n, wmax, cplx=True)
    pat = (rng.standard_normal(M) + 1j * rng.standard_normal(M)).astype(np.complex64)
    x = x.astype(np.complex128)
    starts = []
    for k in range(count):
        if k % 4 == 0:
            s = int(edges[int(rng.integers(1, len(edges) - 1))]) - int(rng.integers(1, M))             # across a segment edge
        elif k % 4 == 1:
            b = int(rng.choice(borders))
            s = b * int(rng.integers(1, n // b)) - int(rng.integers(0, M))                               # across a block border
        else:
            s = int(rng.integers(0, n - M))
        s = min(max(s, 0), n - M)
        seg = int(np.searchsorted(edges, s, side="right")) - 1
        amp = np.sqrt(np.mean(np.abs(x[edges[seg]:edges[seg + 1]]) ** 2) / 2) if kinds[seg] != "zero" else 0.0
        x[s:s + M] += (3 * amp if amp > 0 else 1e-2) * np.exp(2j * np.pi * rng.random()) * pat
        starts.append(s)
    return pat, x.astype(np.complex64), edges, kinds, sorted(starts)


def unit_pattern(pat):
    """The unit-energy complex64 pattern as the device receives it."""
    p = np.ascontiguousarray(pat, np.complex64)
    return (p / np.float32(np.sqrt(np.sum(np.abs(p.astype(np.complex128)) ** 2)))).astype(np.complex64)


# ------------------------------------------------------------------------------------------------- windowed OLA, rfft
def ola_windowed(x, Ne, N, H, win):
    """ola_oracle.Ola's windowed branch (fourier.cc:880-926) in float64: the whole-block outputs of len(x) inputs
    (the very first block gives none)."""
    x = w64(np.asarray(x, np.complex64))
    H = w64(np.asarray(H, np.complex64))
    fc = w64(np.asarray(win, np.float32))
    Nz, h = N - Ne, Ne // 2
    padded = np.zeros(N, np.complex128)
    last = np.zeros(Ne, np.complex128)
    svg = np.zeros(Ne, np.complex128)
    tf = lambda v: np.fft.ifft(np.fft.fft(v) * H)
    out = []
    for b in range(len(x) // Ne):
        xb = x[b * Ne:(b + 1) * Ne]
        padded[N - h:] = xb[:h]
        padded[N - Ne:] *= fc
        x2 = tf(padded)
        svg[Ne - Nz:] += x2[:Nz]
        last[h:] += svg[:h] / 2
        if b > 0:
            out.append(last.copy())
        last[:h] = svg[h:] / 2
        last[h:] = 0
        svg = x2[N - Ne:].copy()
        padded[N - Ne:] = xb * fc
        x2 = tf(padded)
        svg[Ne - Nz:] += x2[:Nz]
        last += svg / 2
        svg = x2[Nz:Nz + Ne].copy()
        padded[Nz:Nz + h] = xb[h:]
    return np.concatenate(out) if out else np.zeros(0, np.complex128)


def rfft(x):
    """RTFRPlan: the unitary transform of real rows, all n bins."""
    x = np.asarray(x, np.float32).astype(np.float64)
    return np.fft.fft(x, axis=-1) / np.sqrt(x.shape[-1])
