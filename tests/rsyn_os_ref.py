"""Float64 references of the oversampled real-output polyphase synthesizer (include/tsdgpu.h:
tsdgpu_synthesizer_create_real_oversampled), a float32 emulation of its scheme, and the runs its tests share.  Test helper, not a
conftest; built on rsyn_ref, syn_os_ref and poly_f64.

The operator takes the rows c = 0 .. N = M / 2 of a block whose other rows are conjugates and is the oversampled complex
synthesizer's on the extended block, which is exactly real: with hop D = M / OS and p counted over the whole stream

    x[p] = sum_m f[p - m D] ( Re u_0[m] + (-1)^p Re u_N[m] + 2 sum_{0<c<N} Re( u_c[m] exp(+2 pi i c p / M) ) )

so the references are syn_os_ref.definition / syn_os_ref.synth64 on rsyn_ref.extend(u), real part; the per-sample float64
statement and bound are poly_f64.syn's on the extended block at that OS, with M the REAL frame length.

The scheme (synthesizer_real_os.hip): per frame rsyn_ref.tangle and an N-point inverse transform give the M real values
w_2j = Re z_j, w_2j+1 = Im z_j; then, Q = ceil(K / D),

    x[q D + s'] = sum_{j<Q} f[j D + s'] w_r[q - j],   r = ((hops0 + q) D + s') mod M."""
import numpy as np
import scipy.fft

import poly_f64 as PF
import rsyn_ref as R
import syn_os_ref as O
from rsyn_ref import bits, dev, extend, host, rel_err, rows, tangle  # noqa: F401  (shared with the tests)

input = R.input


def _hist(history):
    return None if history is None else extend(np.asarray(history, np.complex128))


def definition(u, f, M, OS, hops0=0, history=None):
    """the double sum on the extended block, term by term -> F D float64"""
    return O.definition(extend(u), f, M, OS, hops0, _hist(history)).real


def synth64(u, f, M, OS, hops0=0, history=None):
    """syn_os_ref.synth64 (an M-point transform of the extended block) -> F D float64"""
    return O.synth64(extend(u), f, M, OS, hops0, _hist(history)).real


def _frames(u, Q, history, dtype):
    """(history ++ u) tangled and transformed at N points -> the (F + Q - 1, M) real values of every frame, in `dtype`'s precision"""
    u = np.asarray(u)
    C = u.shape[0]
    M = 2 * (C - 1)
    hist = np.zeros((C, Q - 1), u.dtype) if history is None else np.asarray(history)
    assert hist.shape == (C, Q - 1)
    ue = np.concatenate([hist.astype(dtype), u.astype(dtype)], axis=1)
    z = scipy.fft.ifft(tangle(ue, dtype), axis=1, norm="forward")
    assert z.dtype == dtype
    w = np.empty((ue.shape[1], M), z.real.dtype)
    w[:, 0::2] = z.real
    w[:, 1::2] = z.imag
    return w


def fast64(u, f, M, OS, hops0=0, history=None):
    """the scheme in double: tangle, N-point inverse transform, chains at the positions r -> F D float64"""
    f = np.asarray(f, np.float64)
    D = M // OS
    Q = -(-len(f) // D)
    F = np.asarray(u).shape[1]
    fp = np.zeros(Q * D)
    fp[: len(f)] = f
    fp = fp.reshape(Q, D)
    w = _frames(np.asarray(u, np.complex128), Q, history, np.complex128)
    r = ((np.arange(F)[:, None] + hops0) * D + np.arange(D)[None, :]) % M
    x = np.zeros((F, D))
    for j in range(Q):
        x += fp[j][None, :] * np.take_along_axis(w[Q - 1 - j: Q - 1 - j + F], r, axis=1)
    return x.reshape(F * D)


def emulate32(u, fp, M, OS):
    """the float32 run of the scheme with the table fp (Q, D) (the right one or a mutant) from zero history and phase 0: a float32
    tangle, an N-point complex64 scipy.fft.ifft(norm="forward"), float32 chains oldest frame first at the positions r
    -> F D float32"""
    u = np.asarray(u, np.complex64)
    fp = np.asarray(fp, np.float32)
    D = M // OS
    Q = fp.shape[0]
    assert fp.shape == (Q, D) and u.shape[0] == rows(M)
    F = u.shape[1]
    w = _frames(u, Q, None, np.complex64)
    assert w.dtype == np.float32
    r = (np.arange(F)[:, None] * D + np.arange(D)[None, :]) % M
    x = np.zeros((F, D), np.float32)
    for j in range(Q - 1, -1, -1):
        wj = np.take_along_axis(w[Q - 1 - j: Q - 1 - j + F], r, axis=1)
        x = (x + (fp[j][None, :] * wj).astype(np.float32)).astype(np.float32)
    return x.reshape(F * D)


def f64_case(u, f, M, OS):
    """-> (x64 (F D,) real, bound (F D,)) of poly_f64.syn on the extended block at OS, M the real frame length"""
    x64, bound = PF.syn(extend(np.asarray(u, np.complex64)), PF.syn_table(f, M // OS), M, OS)
    return x64.real, bound


# ------------------------------------------------------------------------------------------------------------- GPU runs
def run(sy, ud, frames, check_phase=True):
    """the device rows through the handle in steps of the given frame counts, the phase checked after each -> the F D floats
    (host)"""
    import torch
    OS, p0 = sy.oversample, sy.phase
    outs, a = [], 0
    for f in frames:
        outs.append(sy.step(ud[:, a:a + f]))
        a += f
        if check_phase:
            assert sy.phase == (p0 + a) % OS, (sy.channels, OS, a)
    return host(torch.cat(outs))


def fresh_run(tg, f, M, OS, ud, frames):
    sy = tg.RealSynthesizer.oversampled(f, M, OS)
    x = run(sy, ud, frames)
    sy.close()
    return x
