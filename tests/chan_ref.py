"""Float64 references of the polyphase channelizer (include/tsdgpu.h: tsdgpu_channelizer) and the inputs its tests share.

    y_c[m] = sum_{k<K} h[k] x[n_m - k] exp(-2 pi i c (n_m - k) / M),   n_m = m M + M - 1

`history`: the (P - 1) M samples before x[0], oldest first (P = ceil(K / M)); None = zeros (a fresh stream).  Both functions
return the (M, F) block of a step of F = len(x) / M frames.  With a history, sample positions are counted from the start of x:
a whole number of frames came before, so the phase of the mixer is the same."""
import numpy as np


def _extended(x, h, M, history):
    x = np.asarray(x, np.complex128)
    h = np.asarray(h, np.float64)
    assert x.ndim == 1 and len(x) % M == 0
    P = -(-len(h) // M)
    H = (P - 1) * M
    hist = np.zeros(H, np.complex128) if history is None else np.asarray(history, np.complex128)
    assert hist.shape == (H,)
    return np.concatenate([hist, x]), h, P, H


def definition(x, h, M, history=None):
    """the formula, term by term: small sizes only"""
    xe, h, P, H = _extended(x, h, M, history)
    F = (len(xe) - H) // M
    y = np.zeros((M, F), np.complex128)
    k = np.arange(len(h))
    for m in range(F):
        nm = m * M + M - 1
        pos = nm - k                                   # sample positions, may be negative: history, then zeros
        ok = pos + H >= 0
        xs = np.where(ok, xe[np.clip(pos + H, 0, len(xe) - 1)], 0.0)
        for c in range(M):
            y[c, m] = np.sum(h * xs * np.exp(-2j * np.pi * c * pos / M))
    return y


def polyphase64(x, h, M, history=None):
    """the fast form in double: v_s[m] = sum_p g_p[s] x[(m - p) M + s], g_p[s] = h[p M + M - 1 - s]; y = fft over s"""
    xe, h, P, H = _extended(x, h, M, history)
    F = (len(xe) - H) // M
    hp = np.zeros(P * M)
    hp[: len(h)] = h
    g = hp.reshape(P, M)[:, ::-1]                      # g[p, s]
    fr = xe.reshape(P - 1 + F, M)                      # frame f of the step is row f + P - 1
    v = np.zeros((F, M), np.complex128)
    for p in range(P):
        v += g[p][None, :] * fr[P - 1 - p: P - 1 - p + F]
    return np.ascontiguousarray(np.fft.fft(v, axis=1).T)


def prototype(M, K):
    """Hann-windowed sinc of cutoff 1 / M (float32); [1.0] for K = 1"""
    if K == 1:
        return np.array([1.0], np.float32)
    k = np.arange(K) - (K - 1) / 2
    w = 0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(K) + 1) / (K + 1))
    return (np.sinc(k / M) / M * w).astype(np.float32)


def stream(n, M, seed=0):
    """seeded complex normal samples plus a tone of amplitude 1e3 at 3.3 / M cycles per sample (between two channels: leakage,
    channel order and the sign of the exponent all show)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    x = x + 1e3 * np.exp(2j * np.pi * (3.3 / M) * np.arange(n))
    return x.astype(np.complex64)


def rel_err(y, ref):
    return float(np.abs(np.asarray(y, np.complex128) - ref).max() / np.abs(ref).max())
