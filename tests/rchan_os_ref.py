"""Float64 references of the oversampled real-input polyphase channelizer (include/tsdgpu.h:
tsdgpu_channelizer_create_real_oversampled), a float32 emulation of its scheme, and the runs its tests share.  Test helper, not a
conftest; built on rchan_ref, chan_os_ref and poly_f64.

The operator is the oversampled complex channelizer's restricted to a real stream, rows 0 .. M / 2 only:

    y_c[m] = sum_{k<K} h[k] x[n_m - k] exp(-2 pi i c (n_m - k) / M),   n_m = m D + D - 1,   D = M / OS,   c <= M / 2

so the references are chan_os_ref.definition / chan_os_ref.polyphase64 on the stream widened to complex, rows [: M // 2 + 1]; the
per-frame float64 statement and bound are poly_f64.chan's on the widened stream at that OS, with M the REAL frame length.

The scheme (channelizer_real_os.hip): the M real branch sums of frame m, v_s = sum_p g_p[s] x[(m + 1) D - M + s - p M], are read
as N = M / 2 pairs; pair j goes to pair slot (j + rot / 2) mod N, rot = ((m + 1) D) mod M (even at every served shape); the N-point
transform of the slots and rchan_ref.untangle give the rows."""
import numpy as np

import chan_os_ref as O
import poly_f64 as PF
import rchan_ref as R
from rchan_ref import bits, dev, host, rows, widen  # noqa: F401  (shared with the tests)


def definition(x, h, M, OS, hops0=0, history=None):
    hist = None if history is None else np.asarray(history, np.float64)
    return O.definition(widen(x), h, M, OS, hops0, hist)[: rows(M)]


def polyphase64(x, h, M, OS, hops0=0, history=None):
    hist = None if history is None else np.asarray(history, np.float64)
    return O.polyphase64(widen(x), h, M, OS, hops0, hist)[: rows(M)]


def emulate32(x, g, M, OS):
    """the float32 run of the scheme with the table g (the right one or a mutant), from zero history and phase 0: float32 chains
    oldest first, the PAIRS rotated, an N-point complex64 scipy.fft, a float32 untangle -> (M / 2 + 1, F) complex64"""
    x = np.asarray(x, np.float32)
    g = np.asarray(g, np.float32)
    P, D = g.shape[0], M // OS
    assert g.shape == (P, M) and len(x) % D == 0
    F, H, N = len(x) // D, P * M - D, M // 2
    xe = np.concatenate([np.zeros(H, np.float32), x])
    a = (np.arange(F)[:, None] + 1) * D - M + np.arange(M)[None, :]
    v = np.zeros((F, M), np.float32)
    for p in range(P - 1, -1, -1):
        v = (v + g[p][None, :] * xe[H + a - p * M]).astype(np.float32)
    rot = ((np.arange(F) + 1) * D) % M
    assert (rot % 2 == 0).all()
    pj = (np.arange(N)[None, :] + (rot // 2)[:, None]) % N
    w = np.zeros_like(v)
    fr = np.arange(F)[:, None]
    w[fr, 2 * pj] = v[:, 0::2]
    w[fr, 2 * pj + 1] = v[:, 1::2]
    return np.ascontiguousarray(R.untangle(w, np.complex64).T)


def f64_case(x, h, M, OS):
    """-> (y64 (M / 2 + 1, F), bound (F,)) of poly_f64.chan on the widened stream at OS, rows 0 .. M / 2"""
    y64, bound = PF.chan(widen(x), PF.chan_table(h, M), M, OS)
    return y64[: rows(M)], bound


# ------------------------------------------------------------------------------------------------------------- GPU runs
def run(ch, xd, hops, check_phase=True):
    """the stream through the handle in steps of the given hop counts, the phase checked after each -> the
    (M / 2 + 1, sum(hops)) block (host)"""
    import torch
    D, OS = ch.hop, ch.oversample
    p0 = ch.phase
    outs, a = [], 0
    for f in hops:
        outs.append(ch.step(xd[a * D:(a + f) * D]))
        a += f
        if check_phase:
            assert ch.phase == (p0 + a) % OS, (ch.channels, OS, a)
    return host(torch.cat(outs, dim=1))


def fresh_run(tg, h, M, OS, xd, hops):
    ch = tg.RealChannelizer.oversampled(h, M, OS)
    y = run(ch, xd, hops)
    ch.close()
    return y
