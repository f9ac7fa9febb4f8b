"""What the OLA, Welch and spectrum entry points refuse (include/tsdgpu.h: tsdgpu_ola_*, tsdgpu_welch, tsdgpu_spectrum_*), through the
C ABI: the status and the whole text of tsdgpu_last_error().  Every check below runs before the first HIP call, so no GPU is needed.
The texts are part of the interface (the adaptors and the callers' logs show them): they are literals here, not rebuilt from the
code's rules."""
import ctypes as C

import numpy as np
import pytest

# the status in the tables: 1 = TSDGPU_ERR_INVALID


def refused(entry, *args):
    import libtsd_amd as t
    L = t.lib()
    rc = getattr(L, f"tsdgpu_{entry}")(*args)
    return rc, L.tsdgpu_last_error().decode()


# a check that comes after the NULL-handle one never looks into the handle: a block of zeros stands for it
NO_HANDLE = np.zeros(4096, np.uint8)

OLA_CREATE = [
    # out given, block_len, min_zeros, window length (0: none)
    (False, 512, 0, 0, 1, 'ola_create: out is NULL'),
    (True, 512, -1, 0, 1, 'ola_create: negative zero count'),
    (True, (1 << 24) + 1, 0, 0, 1, 'ola_create: FFT size 33554432 too large'),
    (True, 10, 100, 0, 1, 'ola_create: Nz = 118 zeros exceed the block size Ne = 10'),
    (True, 511, 1, 511, 1, 'ola_create: the windowed mode needs an even block size (Ne = 511)'),
]


@pytest.mark.parametrize("out_given, block_len, min_zeros, nwin, status, text", OLA_CREATE)
def test_ola_create_refuses(out_given, block_len, min_zeros, nwin, status, text):
    h = C.c_void_p()
    w = np.ones(nwin, np.float32) if nwin else None
    assert refused('ola_create', C.byref(h) if out_given else None, block_len, min_zeros, None if w is None else w.ctypes.data) == (status, text)
    assert not h.value


def _ola_null_args(entry):
    x, y = np.zeros(16, np.complex64), np.zeros(16, np.complex64)
    n_out, sp, nf = C.c_int64(0), C.c_void_p(), C.c_int(0)
    return {
        'ola_step': (None, x.ctypes.data, 16, y.ctypes.data, C.byref(n_out), None),
        'ola_analyse': (None, x.ctypes.data, 16, C.byref(sp), C.byref(nf), None),
        'ola_synthese': (None, y.ctypes.data, C.byref(n_out), None),
        'ola_set_response': (None, x.ctypes.data),
        'ola_apply_response': (None, None),
        'ola_read_spectra': (None, y.ctypes.data, None),
        'ola_write_spectra': (None, x.ctypes.data, None),
    }[entry], (x, y)


OLA_NULL = [
    ('ola_step', 1, 'ola_step: NULL handle'),
    ('ola_analyse', 1, 'ola_analyse: NULL handle'),
    ('ola_synthese', 1, 'ola_synthese: NULL handle'),
    ('ola_set_response', 1, 'ola_set_response: NULL handle'),
    ('ola_apply_response', 1, 'ola_apply_response: nothing analysed'),
    ('ola_read_spectra', 1, 'ola_read_spectra: nothing analysed'),
    ('ola_write_spectra', 1, 'ola_write_spectra: nothing analysed'),
]


@pytest.mark.parametrize("entry, status, text", OLA_NULL)
def test_ola_null_handle_is_refused(entry, status, text):
    args, keep = _ola_null_args(entry)
    assert refused(entry, *args) == (status, text)


def test_ola_sizes_of_null_are_minus_one():
    import libtsd_amd as t
    L = t.lib()
    assert L.tsdgpu_ola_fft_size(None) == -1
    assert L.tsdgpu_ola_block_len(None) == -1
    assert L.tsdgpu_ola_max_out(None, 512) == -1


WELCH = [
    # N, n, window given, S given
    (0, 64, True, True, 1, 'welch: N = 0'),
    ((1 << 24) + 1, 64, True, True, 1, 'welch: N = 16777217'),
    (16, -1, True, True, 1, 'welch: bad arguments'),
    (16, 64, False, True, 1, 'welch: bad arguments'),
    (16, 64, True, False, 1, 'welch: bad arguments'),
]


@pytest.mark.parametrize("N, n, window_given, S_given, status, text", WELCH)
def test_welch_refuses(N, n, window_given, S_given, status, text):
    x, w, S = np.zeros(64, np.complex64), np.ones(16, np.float32), np.zeros(16, np.float32)
    nseg = C.c_int64(0)
    assert refused('welch', x.ctypes.data, n, N, w.ctypes.data if window_given else None, S.ctypes.data if S_given else None,
                   C.byref(nseg), None) == (status, text)


SPECTRUM_CREATE = [
    # out given, BS, nsubs, nmeans, window given, sweep active, sweep step
    (False, 64, 1, 1, True, 0, 0, 1, 'spectrum_create: out is NULL'),
    (True, 0, 1, 1, True, 0, 0, 1, 'spectrum_create: BS = 0, nsubs = 1, nmeans = 1'),
    (True, 64, 0, 1, True, 0, 0, 1, 'spectrum_create: BS = 64, nsubs = 0, nmeans = 1'),
    (True, 3, 4, 1, True, 0, 0, 1, 'spectrum_create: BS = 3, nsubs = 4, nmeans = 1'),
    (True, 64, 1, 1, False, 0, 0, 1, 'spectrum_create: NULL window'),
    (True, 64, 4, 1, True, 1, -1, 1, 'spectrum_create: sweep step -1'),
]


@pytest.mark.parametrize("out_given, BS, nsubs, nmeans, window_given, sweep, step, status, text", SPECTRUM_CREATE)
def test_spectrum_create_refuses(out_given, BS, nsubs, nmeans, window_given, sweep, step, status, text):
    h = C.c_void_p()
    w = np.ones(64, np.float32)
    assert refused('spectrum_create', C.byref(h) if out_given else None, BS, nsubs, nmeans, w.ctypes.data if window_given else None,
                   sweep, step, None) == (status, text)
    assert not h.value


SPECTRUM_STEP = [
    (False, 1, 1, 'spectrum_step: NULL handle'),
    (True, -1, 1, 'spectrum_step: negative block count'),
]


@pytest.mark.parametrize("handle_given, nblocks, status, text", SPECTRUM_STEP)
def test_spectrum_step_refuses(handle_given, nblocks, status, text):
    x, y = np.zeros(64, np.complex64), np.zeros(64, np.float32)
    got = C.c_int64(0)
    assert refused('spectrum_step', NO_HANDLE.ctypes.data if handle_given else None, x.ctypes.data, nblocks, y.ctypes.data, 1,
                   C.byref(got), None) == (status, text)


def test_spectrum_sizes_of_null_are_minus_one():
    import libtsd_amd as t
    assert t.lib().tsdgpu_spectrum_bins(None) == -1
    assert t.lib().tsdgpu_spectrum_pending(None) == -1


@pytest.mark.parametrize("entry", ["ola_destroy", "spectrum_destroy"])
def test_destroying_null_is_fine(entry):
    import libtsd_amd as t
    assert getattr(t.lib(), f"tsdgpu_{entry}")(None) == 0
