"""The polyphase banks (Channelizer, Synthesizer; any oversampling) against float64, judged per frame / per output sample: the
float64 statements with their error bounds, a float32 emulation with its mutants, and the inputs the dynamic-range tests share.
Test helper, not a conftest.  The conventions are those of chan_os_ref.py / syn_os_ref.py (OS = 1: chan_ref.py / syn_ref.py), a
whole stream from zero history.  u = 2^-24 and gamma(m) are f64ref's; C_FFT = 8 is test_dynamic_range_gpu.py's constant and
derivation.  No constant is tuned per case.

Channelizer, frame m (the transform mixes the channels of a frame: there is no per-channel bound).  P = ceil(K / M),
A_s[m] = sum_p |g_p[s]| |x[a_s - p M]|:

    max_c |y_c[m] - y64_c[m]| <= gamma(P + 2) sum_s A_s[m] + C_FFT u log2(M) ||A[m]||_2

  first term: every v_s is a P-term float32 dot product, |v_s - v64_s| <= gamma(P) A_s (Wilkinson, any order, with or without
  fma; + 2 as in f64ref's direct paths), and an output is a sum of the M values times unit factors.  Second term: the transform
  of the computed v, |v_s| <= (1 + gamma) A_s.  The rotation of the oversampled bank is a permutation of s and drops out.

Synthesizer, output sample q D + s'.  Q = ceil(K / D), r = (q D + s') mod M, w64 = the float64 unscaled inverse transform of
each frame:

    |x - x64| <= sum_j |f[j D + s']| ( C_FFT u log2(M) ||u[:, q - j]||_2 + gamma(Q + 2) |w64_r[q - j]| )

  the computed w_r of a frame is within C_FFT u log2(M) ||u[:, frame]||_2 of w64_r; the Q-term float32 chain over them adds
  gamma(Q) sum_j |f_j| |w_j|.

The FFT term is the normwise constant of the unitary transform (||e||_2 <= C u log2(M) ||v||_2) applied to every output of the
UNSCALED transform: the rms figure of its M outputs held by each of them, sqrt(M) below the worst case of a single output.  A
float32 chain plus a complex64 scipy.fft sits at 0.08 ... 0.12 of the whole bound on the inputs below, a dropped edge tap 1e2 ...
1e6 over it (tests/test_poly_f64_cpu.py); the kernels measured 0.15 ... 0.36 (profiles/r13_polyphase_f64_ratios.txt).

A frame / sample whose bound is 0 read nothing but exact zeros and must come out exactly 0."""
import numpy as np
import scipy.fft

import f64ref as R

C_FFT = 8.0
STEPS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 33, 100)     # frames per call: around the 8-frame halves and 16-frame units; odd: the phase moves


# --------------------------------------------------------------------------------------------------------- tap tables
def chan_table(h, M):
    """g[p, s] = h[p M + M - 1 - s], zero-padded: (P, M) float32"""
    h = np.asarray(h, np.float32)
    P = -(-len(h) // M)
    hp = np.zeros(P * M, np.float32)
    hp[: len(h)] = h
    return np.ascontiguousarray(hp.reshape(P, M)[:, ::-1])


def syn_table(f, D):
    """fp[j, s'] = f[j D + s'], zero-padded: (Q, D) float32"""
    f = np.asarray(f, np.float32)
    Q = -(-len(f) // D)
    fp = np.zeros(Q * D, np.float32)
    fp[: len(f)] = f
    return fp.reshape(Q, D)


def mutants(taps, table, L, s0):
    """The three wrong tables of a bank (table = chan_table with L = M, or syn_table with L = D): the first tap dropped, the last
    tap dropped, branch s0's taps one frame late."""
    first, last = np.array(taps, np.float32), np.array(taps, np.float32)
    first[0] = 0
    last[-1] = 0
    late = table(taps, L)
    late[1:, s0] = late[:-1, s0].copy()
    late[0, s0] = 0
    return {"h[0] dropped": table(first, L), "h[K-1] dropped": table(last, L), f"branch {s0} one frame late": late}


# --------------------------------------------------------------------------------------------------------- channelizer
def chan(x, g, M, OS, emulate=None):
    """x (complex64, whole hops) through the table g from zero history.
    -> (y64 (M, F), bound (F,)); with emulate = a table (g itself or a mutant) also the float32 run of THAT table: chains oldest
    tap first, then scipy.fft in complex64."""
    x = np.asarray(x, np.complex64)
    g = np.asarray(g, np.float32)
    P, D = g.shape[0], M // OS
    assert g.shape == (P, M) and x.ndim == 1 and len(x) % D == 0
    F = len(x) // D
    H = P * M - D
    xe = np.concatenate([np.zeros(H, np.complex64), x])
    a = (np.arange(F)[:, None] + 1) * D - M + np.arange(M)[None, :]             # a[m, s], from x[0]
    v = np.zeros((F, M), np.complex128)
    A = np.zeros((F, M))
    v32 = np.zeros((F, M), np.complex64) if emulate is not None else None
    g64, e32 = g.astype(np.float64), None if emulate is None else np.asarray(emulate, np.float32)
    for p in range(P - 1, -1, -1):
        xs = xe[H + a - p * M]
        v += g64[p][None, :] * xs
        A += np.abs(g64[p])[None, :] * np.abs(xs.astype(np.complex128))
        if emulate is not None:
            v32 = (v32 + (e32[p][None, :] * xs).astype(np.complex64)).astype(np.complex64)
    rot = a % M

    def out(val):
        w = np.zeros_like(val)
        np.put_along_axis(w, rot, val, axis=1)
        return w
    y64 = np.ascontiguousarray(np.fft.fft(out(v), axis=1).T)
    bound = R.gamma(P + 2) * A.sum(axis=1) + C_FFT * R.U * np.log2(M) * np.sqrt((A * A).sum(axis=1))
    if emulate is None:
        return y64, bound
    y32 = scipy.fft.fft(out(v32), axis=1)
    assert y32.dtype == np.complex64
    return y64, bound, np.ascontiguousarray(y32.T)


def chan_judge(y, y64, bound, what=""):
    """-> worst err / bound over the frames; asserts the shape and that zero-bound frames are exactly zero"""
    y = np.asarray(y)
    assert y.shape == y64.shape, (what, y.shape, y64.shape)
    err = np.abs(y.astype(np.complex128) - y64).max(axis=0)
    dead = bound == 0
    assert not y[:, dead].any(), (what, "a frame of exact zeros came out non-zero")
    return float((err[~dead] / bound[~dead]).max(initial=0.0))


# --------------------------------------------------------------------------------------------------------- synthesizer
def syn(u, fp, M, OS, emulate=None):
    """u (M, F) complex64 through the table fp from zero history.
    -> (x64 (F D,), bound (F D,)); with emulate = a table also the float32 run of that table: scipy.fft in complex64, then chains
    oldest frame first."""
    u = np.asarray(u, np.complex64)
    fp = np.asarray(fp, np.float32)
    D = M // OS
    Q = fp.shape[0]
    assert fp.shape == (Q, D) and u.ndim == 2 and u.shape[0] == M
    F = u.shape[1]
    ue = np.concatenate([np.zeros((M, Q - 1), np.complex64), u], axis=1)
    w = np.fft.ifft(ue.T.astype(np.complex128), axis=1) * M                      # w[m + Q - 1, r]
    nrm = np.sqrt((np.abs(ue.astype(np.complex128)) ** 2).sum(axis=0))          # ||u[:, m]||_2, m + Q - 1
    r = (np.arange(F)[:, None] * D + np.arange(D)[None, :]) % M                 # r[q, s']
    f64 = fp.astype(np.float64)
    x = np.zeros((F, D), np.complex128)
    bound = np.zeros((F, D))
    if emulate is not None:
        w32 = scipy.fft.ifft(np.ascontiguousarray(ue.T), axis=1, norm="forward")
        assert w32.dtype == np.complex64
        e32, x32 = np.asarray(emulate, np.float32), np.zeros((F, D), np.complex64)
    cf, gq = C_FFT * R.U * np.log2(M), R.gamma(Q + 2)
    for j in range(Q - 1, -1, -1):
        rows = slice(Q - 1 - j, Q - 1 - j + F)
        wj = np.take_along_axis(w[rows], r, axis=1)
        x += f64[j][None, :] * wj
        bound += np.abs(f64[j])[None, :] * (cf * nrm[rows][:, None] + gq * np.abs(wj))
        if emulate is not None:
            x32 = (x32 + (e32[j][None, :] * np.take_along_axis(w32[rows], r, axis=1)).astype(np.complex64)).astype(np.complex64)
    if emulate is None:
        return x.reshape(-1), bound.reshape(-1)
    return x.reshape(-1), bound.reshape(-1), x32.reshape(-1)


def syn_judge(x, x64, bound, what=""):
    """-> worst err / bound over the samples; asserts the shape and that zero-bound samples are exactly zero"""
    x = np.asarray(x)
    assert x.shape == x64.shape, (what, x.shape, x64.shape)
    err = np.abs(x.astype(np.complex128) - x64)
    dead = bound == 0
    assert not x[dead].any(), (what, "a sample of exact zeros came out non-zero")
    return float((err[~dead] / bound[~dead]).max(initial=0.0))


# --------------------------------------------------------------------------------------------------------- inputs
def taps(rng, K):
    """every tap counts: standard normal, float32"""
    return rng.standard_normal(K).astype(np.float32)


def chan_input(rng, n, M):
    """f64ref.burst_train (loud 1e4 / 1e6, quiet 1 / 1e-3, exact zeros; segments up to 12 M samples, shorter where the stream is
    short, so that it holds a dozen of them) with at least four zero stretches, and in four of them a lone sample of 1e6: an
    impulse reads every tap back on its own.  Two sit at the start of their stretch (zeros follow: the last taps stand alone) and
    two at its end (zeros came before: the first taps do)."""
    hi = max(64, min(max(600, 12 * M), n // 6))
    x, edges, kinds = R.burst_train(rng, n, 4 * M, cplx=True, lo=min(300, hi // 4), hi=hi)
    x, kinds = x.copy(), list(kinds)
    live = [i for i, k in enumerate(kinds) if k != "zero"]
    short = 4 - (len(kinds) - len(live))
    if short > 0:
        for i in rng.choice(live, min(short, len(live) - 1), replace=False):
            x[edges[i]:edges[i + 1]] = 0
            kinds[i] = "zero"
    zeros = [i for i, k in enumerate(kinds) if k == "zero"]
    for j, i in enumerate(rng.permutation(zeros)[:4]):
        a, b = int(edges[i]), int(edges[i + 1])
        o = int(rng.integers(0, min(b - a, 4)))
        x[a + o if j % 2 == 0 else b - 1 - o] = 1e6
    return x


def syn_input(rng, M, F):
    """(M, F) complex normal rows times a per-frame envelope of the burst kinds, segments of 1 ... 40 frames (quiet frames start
    just before and after 8-frame halves, 16-frame units and sub-run starts); one row a further 1e4 louder"""
    env = np.zeros(F)
    o = 0
    while o < F:
        L = int(rng.integers(1, 41))
        q = rng.random()
        amp = float(rng.choice((1e4, 1e6))) if q < 0.3 else float(rng.choice((1.0, 1e-3))) if q < 0.85 else 0.0
        env[o:o + L] = amp
        o += L
    u = (rng.standard_normal((M, F)) + 1j * rng.standard_normal((M, F))) * env[None, :]
    u[int(rng.integers(M))] *= 1e4
    return u.astype(np.complex64)


def ragged(rng, F):
    """frame counts of ragged steps that add up to F"""
    out, o = [], 0
    while o < F:
        c = min(int(rng.choice(STEPS)), F - o)
        out.append(c)
        o += c
    return out


# --------------------------------------------------------------------------------------------------------- GPU runs
def chan_stream(tg, h, M, OS, xd, steps):
    """a fresh Channelizer over the device stream xd in steps of the given frame counts, its phase checked after each
    -> the (M, F) block (host)"""
    import torch
    ch = tg.Channelizer(h, M, oversample=OS)
    D, outs, a = M // OS, [], 0
    assert ch.hop == D
    for f in steps:
        outs.append(ch.step(xd[a * D:(a + f) * D]))
        a += f
        assert ch.phase == a % OS, (M, OS, len(h), a)
    y = torch.cat(outs, dim=1).cpu().numpy()
    ch.close()
    return y


def syn_stream(tg, f, M, OS, ud, steps):
    """a fresh Synthesizer over the device rows ud in steps of the given frame counts, its phase checked after each
    -> the F D samples (host)"""
    import torch
    sy = tg.Synthesizer(f, M, oversample=OS)
    outs, a = [], 0
    assert sy.hop == M // OS
    for n in steps:
        outs.append(sy.step(ud[:, a:a + n]))
        a += n
        assert sy.phase == a % OS, (M, OS, len(f), a)
    x = torch.cat(outs).cpu().numpy()
    sy.close()
    return x
