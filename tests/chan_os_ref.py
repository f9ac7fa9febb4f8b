"""Float64 references of the oversampled polyphase channelizer (include/tsdgpu.h: tsdgpu_channelizer_create_oversampled).

M channels, oversampling OS, hop D = M / OS, samples counted over the whole stream with zeros before sample 0:

    y_c[m] = sum_{k<K} h[k] x[n_m - k] exp(-2 pi i c (n_m - k) / M),   n_m = m D + D - 1

Both functions return the (M, F) block of a step of F = len(x) / D hops.  `hops0`: the hops the stream consumed before x[0],
so x[0] is sample hops0 D of the stream (only hops0 mod OS matters).  `history`: the P M - D samples before x[0], oldest first
(P = ceil(K / M)); None = zeros.  Inputs and prototypes: chan_ref.stream / chan_ref.prototype."""
import numpy as np


def _extended(x, h, M, OS, history):
    x = np.asarray(x, np.complex128)
    h = np.asarray(h, np.float64)
    assert M % OS == 0
    D = M // OS
    assert x.ndim == 1 and len(x) % D == 0
    P = -(-len(h) // M)
    H = P * M - D
    hist = np.zeros(H, np.complex128) if history is None else np.asarray(history, np.complex128)
    assert hist.shape == (H,)
    return np.concatenate([hist, x]), h, D, P, H


def definition(x, h, M, OS, hops0=0, history=None):
    """the formula, term by term: small sizes only"""
    xe, h, D, P, H = _extended(x, h, M, OS, history)
    F = (len(xe) - H) // D
    y = np.zeros((M, F), np.complex128)
    k = np.arange(len(h))
    for m in range(F):
        pos = m * D + D - 1 - k                        # positions counted from x[0]; negative: history, then zeros
        ok = pos + H >= 0
        xs = np.where(ok, xe[np.clip(pos + H, 0, len(xe) - 1)], 0.0)
        ab = pos + hops0 * D                           # positions in the whole stream: the mixer's phase
        for c in range(M):
            y[c, m] = np.sum(h * xs * np.exp(-2j * np.pi * c * ab / M))
    return y


def polyphase64(x, h, M, OS, hops0=0, history=None):
    """the rotated fast form in double: frame m covers a_s = (m + 1) D - M + s; v_s[m] = sum_p g_p[s] x[a_s - p M],
    g_p[s] = h[p M + M - 1 - s]; y = fft(w), w[a_s mod M] = v_s, a_s counted over the whole stream"""
    xe, h, D, P, H = _extended(x, h, M, OS, history)
    F = (len(xe) - H) // D
    hp = np.zeros(P * M)
    hp[: len(h)] = h
    g = hp.reshape(P, M)[:, ::-1]                      # g[p, s]
    a = (np.arange(F)[:, None] + 1) * D - M + np.arange(M)[None, :]       # a[m, s], from x[0]; a - (P - 1) M >= -H
    v = np.zeros((F, M), np.complex128)
    for p in range(P):
        v += g[p][None, :] * xe[H + a - p * M]
    w = np.zeros((F, M), np.complex128)
    np.put_along_axis(w, (a + hops0 * D) % M, v, axis=1)
    return np.ascontiguousarray(np.fft.fft(w, axis=1).T)
