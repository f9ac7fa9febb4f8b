"""Float64 references of the real-input polyphase channelizer (include/tsdgpu.h: tsdgpu_channelizer_create_real), a float32
emulation of its scheme, and the inputs its tests share.  Test helper, not a conftest.

The operator is the complex channelizer's restricted to a real stream, rows 0 .. M / 2 only:

    y_c[m] = sum_{k<K} h[k] x[n_m - k] exp(-2 pi i c (n_m - k) / M),   n_m = m M + M - 1,   c <= M / 2

so the references are chan_ref.definition / chan_ref.polyphase64 on the stream widened to complex, rows [: M // 2 + 1]; the
per-frame float64 statement and bound are poly_f64.chan's on the widened stream, with M the REAL frame length (the N = M / 2
point transform plus the untangling step are its log2 M levels).

The scheme (channelizer_real.hip): the M real branch sums v of a frame are read as N = M / 2 complex positions
z_j = v_2j + i v_2j+1, Z = DFT_N(z), Z[N] = Z[0], and for c = 0 .. N

    E = (Z[c] + conj Z[N - c]) / 2,   O = (Z[c] - conj Z[N - c]) / (2 i),   y_c = E + W_M^c O."""
import numpy as np
import scipy.fft

import chan_ref
import poly_f64 as PF


def rows(M):
    return M // 2 + 1


def widen(x):
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 1
    return x.astype(np.complex64)


def definition(x, h, M, history=None):
    hist = None if history is None else np.asarray(history, np.float64)
    return chan_ref.definition(widen(x), h, M, hist)[: rows(M)]


def polyphase64(x, h, M, history=None):
    hist = None if history is None else np.asarray(history, np.float64)
    return chan_ref.polyphase64(widen(x), h, M, hist)[: rows(M)]


def stream(n, M, seed=0):
    """the real part of chan_ref.stream: normal samples plus a cosine of amplitude 1e3 at 3.3 / M cycles per sample"""
    return np.ascontiguousarray(chan_ref.stream(n, M, seed).real)


def untangle(v, dtype=np.complex128):
    """(F, M) real branch sums -> the (F, M / 2 + 1) rows by the scheme above, in `dtype` (complex128, or complex64: every
    operation of the transform and of the untangling step rounded to float32)"""
    v = np.asarray(v)
    M = v.shape[1]
    N = M // 2
    real = np.float64 if dtype == np.complex128 else np.float32
    z = (v[:, 0::2].astype(real) + 1j * v[:, 1::2].astype(real)).astype(dtype)
    Z = scipy.fft.fft(z, axis=1)
    assert Z.dtype == dtype
    c = np.arange(N)
    Zr = np.conj(Z[:, (N - c) % N])
    w = np.exp(-2j * np.pi * c / M).astype(dtype)                       # generated in double, rounded once
    half, mhalfi = dtype(0.5), dtype(-0.5j)
    y = half * (Z + Zr) + w[None, :] * (mhalfi * (Z - Zr))
    nyq = (Z[:, 0].real - Z[:, 0].imag).astype(dtype)
    out = np.concatenate([y, nyq[:, None]], axis=1)
    assert out.dtype == dtype
    return out


def branch_sums(x, g, dtype):
    """x (float32, whole frames) through the (P, M) table g from zero history, oldest tap first: (F, M) in `dtype` (float64, or
    float32 with every product and sum rounded)"""
    x = np.asarray(x, np.float32)
    g = np.asarray(g, np.float32)
    P, M = g.shape
    F = len(x) // M
    fr = np.concatenate([np.zeros((P - 1) * M, np.float32), x]).reshape(P - 1 + F, M).astype(dtype)
    v = np.zeros((F, M), dtype)
    for p in range(P - 1, -1, -1):
        v = (v + (g[p].astype(dtype)[None, :] * fr[P - 1 - p: P - 1 - p + F]).astype(dtype)).astype(dtype)
    return v


def emulate32(x, g, M):
    """the float32 run of the scheme with the table g (the right one or a mutant): float32 chains, an N-point complex64
    scipy.fft, a float32 untangle -> (M / 2 + 1, F) complex64"""
    assert np.asarray(g).shape[1] == M
    return np.ascontiguousarray(untangle(branch_sums(x, g, np.float32), np.complex64).T)


def f64_case(x, h, M):
    """-> (y64 (M / 2 + 1, F), bound (F,)) of poly_f64.chan on the widened stream, rows 0 .. M / 2"""
    y64, bound = PF.chan(widen(x), PF.chan_table(h, M), M, 1)
    return y64[: rows(M)], bound


def f64_input(rng, n, M):
    """the real part of poly_f64.chan_input (the lone samples of 1e6 are real)"""
    return np.ascontiguousarray(PF.chan_input(rng, n, M).real)


def two_tap_counts(rng, M, P):
    """as test_polyphase_dynamic_range_gpu.py: inside the last row (zero-padded taps), and filling it"""
    return (P - 1) * M + 1 + int(rng.integers(0, M - 1)), P * M


def rel_err(y, ref):
    return chan_ref.rel_err(y, ref)


# ------------------------------------------------------------------------------------------------------------- GPU runs
def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(y):
    import torch
    torch.cuda.synchronize()
    return y.cpu().numpy()


def run(ch, xd, M, frames):
    """the stream through the handle in steps of the given frame counts -> the (M / 2 + 1, sum(frames)) block (host)"""
    import torch
    outs, a = [], 0
    for f in frames:
        outs.append(ch.step(xd[a * M:(a + f) * M]))
        a += f
    return host(torch.cat(outs, dim=1))


def fresh_run(tg, h, M, xd, frames):
    ch = tg.RealChannelizer(h, M)
    y = run(ch, xd, M, frames)
    ch.close()
    return y


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)
