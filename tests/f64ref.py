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
