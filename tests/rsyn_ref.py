"""Float64 references of the real-output polyphase synthesizer (include/tsdgpu.h: tsdgpu_synthesizer_create_real), a float32
emulation of its scheme, and the inputs its tests share.  Test helper, not a conftest.

The operator takes the rows c = 0 .. N = M / 2 of a block whose other rows are conjugates, row M - c = conj(row c), and is the
complex synthesizer's on the extended block, which is exactly real:

    x[p] = sum_m f[p - m M] ( Re u_0[m] + (-1)^p Re u_N[m] + 2 sum_{0<c<N} Re( u_c[m] exp(+2 pi i c p / M) ) )

so the references are syn_ref.definition / syn_ref.synth64 on extend(u), real part; the per-sample float64 statement and bound
are poly_f64.syn's on extend(u), with M the REAL frame length (the tangling step plus the N-point transform are its log2 M
levels) and ||u[:, m]||_2 over the M extended rows.  The imaginary parts of rows 0 and N are not used: extend() drops them.

The scheme (synthesizer_real.hip), the untangling of rchan_ref.py backwards: per frame, with U_c = u_c[m], c < N,

    Z_c = (U_c + conj U_{N-c}) + i conj(W_M^c) (U_c - conj U_{N-c}),   z = IDFT_N(Z) (unscaled),   w_2j = Re z_j, w_2j+1 = Im z_j
    x[q M + s] = sum_{j<P} f[j M + s] w_s[q - j]."""
import numpy as np
import scipy.fft

import poly_f64 as PF
import syn_ref
from rchan_ref import bits, dev, host, rows  # noqa: F401  (the tests take them from here)


def extend(u):
    """(M / 2 + 1, F) -> (M, F): the imaginary parts of rows 0 and N set to zero, then the rows conj(N - 1 .. 1)"""
    u = np.array(u)
    assert u.ndim == 2 and np.iscomplexobj(u)
    N = u.shape[0] - 1
    u[0] = u[0].real
    u[N] = u[N].real
    return np.concatenate([u, np.conj(u[N - 1:0:-1])], axis=0)


def definition(u, f, history=None):
    hist = None if history is None else extend(np.asarray(history, np.complex128))
    return syn_ref.definition(extend(u), f, hist).real


def synth64(u, f, history=None):
    hist = None if history is None else extend(np.asarray(history, np.complex128))
    return syn_ref.synth64(extend(u), f, hist).real


def f64_case(u, f, M):
    """-> (x64 (F M,) real, bound (F M,)) of poly_f64.syn on the extended block"""
    x64, bound = PF.syn(extend(np.asarray(u, np.complex64)), PF.syn_table(f, M), M, 1)
    return x64.real, bound


def input(rng, M, F):
    """rows 0 .. M / 2 of poly_f64.syn_input"""
    return np.ascontiguousarray(PF.syn_input(rng, M, F)[: rows(M)])


def tangle(u, dtype=np.complex128):
    """(N + 1, F) rows -> the (F, N) inputs Z of the half-length inverse transform, in `dtype` (complex64: every operation
    rounded to float32)"""
    u = np.asarray(u)
    N = u.shape[0] - 1
    M = 2 * N
    t = np.ascontiguousarray(u.T).astype(dtype)
    t[:, 0] = t[:, 0].real
    t[:, N] = t[:, N].real
    c = np.arange(N)
    a, b = t[:, c], np.conj(t[:, N - c])
    w = np.exp(2j * np.pi * c / M).astype(dtype)                        # conj W_M^c, generated in double, rounded once
    Z = (a + b) + dtype(1j) * (w[None, :] * (a - b))
    assert Z.dtype == dtype
    return Z


def emulate32(u, fp, M):
    """the float32 run of the scheme with the table fp (P, M) (the right one or a mutant) from zero history: a float32 tangle, an
    N-point complex64 scipy.fft.ifft(norm="forward"), float32 chains oldest frame first -> F M float32"""
    u = np.asarray(u, np.complex64)
    fp = np.asarray(fp, np.float32)
    P = fp.shape[0]
    assert fp.shape == (P, M) and u.shape[0] == rows(M)
    F = u.shape[1]
    ue = np.concatenate([np.zeros((rows(M), P - 1), np.complex64), u], axis=1)
    z = scipy.fft.ifft(tangle(ue, np.complex64), axis=1, norm="forward")
    assert z.dtype == np.complex64
    w = np.empty((F + P - 1, M), np.float32)
    w[:, 0::2] = z.real
    w[:, 1::2] = z.imag
    x = np.zeros((F, M), np.float32)
    for j in range(P - 1, -1, -1):
        x = (x + (fp[j][None, :] * w[P - 1 - j: P - 1 - j + F]).astype(np.float32)).astype(np.float32)
    return x.reshape(F * M)


def rel_err(x, ref):
    return syn_ref.rel_err(x, ref)


# ------------------------------------------------------------------------------------------------------------- GPU runs
def run(sy, ud, frames):
    """the device rows through the handle in steps of the given frame counts -> the F M floats (host)"""
    import torch
    outs, a = [], 0
    for f in frames:
        outs.append(sy.step(ud[:, a:a + f]))
        a += f
    return host(torch.cat(outs))


def fresh_run(tg, f, M, ud, frames):
    sy = tg.RealSynthesizer(f, M)
    x = run(sy, ud, frames)
    sy.close()
    return x
