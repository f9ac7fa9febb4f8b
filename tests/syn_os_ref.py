"""Float64 references of the oversampled polyphase synthesizer (include/tsdgpu.h: tsdgpu_synthesizer_create_oversampled).

M channels, oversampling OS, hop D = M / OS, positions p counted over the whole stream with zeros before frame 0:

    x[p] = sum_{c<M} exp(+2 pi i c p / M) sum_m u_c[m] f[p - m D]

u is the (M, F) block of a step: row c is channel c.  Both functions return the F D samples of the step.  `hops0`: the hops the
stream consumed before u[:, 0], so the step's first sample is position hops0 D of the stream (only hops0 mod OS matters).
`history`: the (M, Q - 1) block of the Q - 1 frames before u[:, 0], oldest first per row (Q = ceil(K / D)); None = zeros.  At
OS = 1 these are syn_ref's.  Inputs and prototypes: syn_ref.rows / chan_ref.prototype."""
import numpy as np

from chan_ref import prototype, rel_err  # noqa: F401  (the tests take them from here)
from syn_ref import rows  # noqa: F401


def _extended(u, f, M, OS, history):
    u = np.asarray(u, np.complex128)
    f = np.asarray(f, np.float64)
    assert u.ndim == 2 and u.shape[0] == M and M % OS == 0
    D = M // OS
    Q = -(-len(f) // D)
    hist = np.zeros((M, Q - 1), np.complex128) if history is None else np.asarray(history, np.complex128)
    assert hist.shape == (M, Q - 1)
    return np.concatenate([hist, u], axis=1), f, D, Q


def definition(u, f, M, OS, hops0=0, history=None):
    """the double sum, term by term: small sizes only"""
    ue, f, D, Q = _extended(u, f, M, OS, history)
    F = ue.shape[1] - (Q - 1)
    c = np.arange(M)
    x = np.zeros(F * D, np.complex128)
    for p in range(F * D):
        inner = np.zeros(M, np.complex128)             # sum_m u_c[m] f[p - m D], frame m of the step is column m + Q - 1
        for m in range(-(Q - 1), F):
            k = p - m * D
            if 0 <= k < len(f):
                inner += ue[:, m + Q - 1] * f[k]
        x[p] = np.sum(np.exp(2j * np.pi * c * (p + hops0 * D) / M) * inner)      # the mixer runs on the stream's position
    return x


def synth64(u, f, M, OS, hops0=0, history=None):
    """the fast form in double: w_r[m] = sum_c u_c[m] e^{+2 pi i c r / M}; x[q D + s'] = sum_j f[j D + s'] w_r[q - j],
    r = ((q + hops0) D + s') mod M"""
    ue, f, D, Q = _extended(u, f, M, OS, history)
    F = ue.shape[1] - (Q - 1)
    fp = np.zeros(Q * D)
    fp[: len(f)] = f
    fp = fp.reshape(Q, D)                              # fp[j, s']
    w = np.fft.ifft(ue.T, axis=1) * M                  # w[m + Q - 1, r]: unscaled inverse transform of each frame
    r = ((np.arange(F)[:, None] + hops0) * D + np.arange(D)[None, :]) % M        # r[q, s']
    x = np.zeros((F, D), np.complex128)
    for j in range(Q):
        x += fp[j][None, :] * np.take_along_axis(w[Q - 1 - j: Q - 1 - j + F], r, axis=1)
    return x.reshape(F * D)
