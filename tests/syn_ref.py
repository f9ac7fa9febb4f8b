"""Float64 references of the polyphase synthesizer (include/tsdgpu.h: tsdgpu_synthesizer) and the inputs its tests share.

    x[p] = sum_{c<M} exp(+2 pi i c p / M) sum_m u_c[m] f[p - m M]

u is the (M, F) block of a step: row c is channel c.  `history`: the (M, P - 1) block of the P - 1 frames before u[:, 0], oldest
first per row (P = ceil(K / M)); None = zeros (a fresh stream).  Both functions return the F M samples of the step.  With a
history, positions are counted from the start of u: whole frames came before, so the phase of the mixer is the same."""
import numpy as np

from chan_ref import prototype, rel_err  # noqa: F401  (the tests take them from here)


def _extended(u, f, history):
    u = np.asarray(u, np.complex128)
    f = np.asarray(f, np.float64)
    assert u.ndim == 2
    M = u.shape[0]
    P = -(-len(f) // M)
    hist = np.zeros((M, P - 1), np.complex128) if history is None else np.asarray(history, np.complex128)
    assert hist.shape == (M, P - 1)
    return np.concatenate([hist, u], axis=1), f, M, P


def definition(u, f, history=None):
    """the double sum, term by term: small sizes only"""
    ue, f, M, P = _extended(u, f, history)
    F = ue.shape[1] - (P - 1)
    c = np.arange(M)
    x = np.zeros(F * M, np.complex128)
    for p in range(F * M):
        inner = np.zeros(M, np.complex128)             # sum_m u_c[m] f[p - m M], frame m of the step is column m + P - 1
        for m in range(-(P - 1), F):
            k = p - m * M
            if 0 <= k < len(f):
                inner += ue[:, m + P - 1] * f[k]
        x[p] = np.sum(np.exp(2j * np.pi * c * p / M) * inner)
    return x


def synth64(u, f, history=None):
    """the fast form in double: w_s[m] = sum_c u_c[m] e^{+2 pi i c s / M}; x[q M + s] = sum_j f[j M + s] w_s[q - j]"""
    ue, f, M, P = _extended(u, f, history)
    F = ue.shape[1] - (P - 1)
    fp = np.zeros(P * M)
    fp[: len(f)] = f
    fp = fp.reshape(P, M)                              # fp[j, s]
    w = np.fft.ifft(ue.T, axis=1) * M                  # w[m + P - 1, s]: unscaled inverse transform of each frame
    x = np.zeros((F, M), np.complex128)
    for j in range(P):
        x += fp[j][None, :] * w[P - 1 - j: P - 1 - j + F]
    return x.reshape(F * M)


def rows(M, F, seed=0):
    """seeded complex normal rows plus a constant 1e3 in row 3: a strong tone at +3 / M of the output rate (channel order and
    the sign of the exponent both show)"""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((M, F)) + 1j * rng.standard_normal((M, F))
    u[3] += 1e3
    return u.astype(np.complex64)
