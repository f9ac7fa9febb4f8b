"""What the single-stream rate changers refuse (include/tsdgpu.h: tsdgpu_resampler_*, tsdgpu_polyfir_*), through the C ABI: the
status and the whole text of tsdgpu_last_error().  Every check below runs before the first HIP call, so no GPU is needed.  The
texts are part of the interface (the adaptors and the callers' logs show them): they are literals here, not rebuilt from the code's
rules.  (The refusals that need a device -- a capacity too small, a NULL output, the LDS limits -- are in test_resample_gpu.py and
test_polyphase_gpu.py.)"""
import ctypes as C

import numpy as np
import pytest

# the status in the tables: 1 = TSDGPU_ERR_INVALID, 3 = TSDGPU_ERR_UNSUPPORTED
F32, C64 = 0, 1
DECIM, HALFBAND, UPS, PICK = 0, 1, 2, 3


def refused(entry, *args):
    import libtsd_amd as t
    L = t.lib()
    rc = getattr(L, f"tsdgpu_{entry}")(*args)
    return rc, L.tsdgpu_last_error().decode()


# a check that comes after the NULL-handle one never looks into the handle: a block of zeros stands for it
NO_HANDLE = np.zeros(4096, np.uint8)
LUT = np.zeros(257 * 256, np.float32)

RESAMPLER_CREATE = [
    # out given, data_type, ratio, lut given, K, nphases
    (False, C64, 1.5, True, 15, 256, 1, 'resampler_create: out is NULL'),
    (True, 7, 1.5, True, 15, 256, 1, 'resampler_create: bad data_type 7'),
    (True, C64, 1.5, False, 15, 256, 1, 'resampler_create: NULL lut'),
    (True, C64, 0.0, True, 15, 256, 1, 'resampler_create: invalid ratio 0'),
    (True, C64, -1.0, True, 15, 256, 1, 'resampler_create: invalid ratio -1'),
    (True, C64, float('nan'), True, 15, 256, 1, 'resampler_create: invalid ratio nan'),
    (True, C64, float('inf'), True, 15, 256, 1, 'resampler_create: invalid ratio inf'),
    (True, C64, 8.5, True, 15, 256, 3,
     'resampler_create: ratio 8.5 outside [1/64, 8] (filtre_reechan folds ratios into [0.5,2) with half-band stages first)'),
    (True, C64, 0.01, True, 15, 256, 3,
     'resampler_create: ratio 0.01 outside [1/64, 8] (filtre_reechan folds ratios into [0.5,2) with half-band stages first)'),
    (True, C64, 1.5, True, 0, 256, 3, 'resampler_create: K=0 nphases=256 unsupported (K <= 256, nphases <= 8191)'),
    (True, C64, 1.5, True, 257, 256, 3, 'resampler_create: K=257 nphases=256 unsupported (K <= 256, nphases <= 8191)'),
    (True, C64, 1.5, True, 15, 0, 3, 'resampler_create: K=15 nphases=0 unsupported (K <= 256, nphases <= 8191)'),
    (True, C64, 1.5, True, 15, 8192, 3, 'resampler_create: K=15 nphases=8192 unsupported (K <= 256, nphases <= 8191)'),
]


@pytest.mark.parametrize("out_given, data_type, ratio, lut_given, K, nphases, status, text", RESAMPLER_CREATE)
def test_resampler_create_refuses(out_given, data_type, ratio, lut_given, K, nphases, status, text):
    h = C.c_void_p()
    assert refused('resampler_create', C.byref(h) if out_given else None, data_type, ratio, LUT.ctypes.data if lut_given else None, K,
                   nphases) == (status, text)
    assert not h.value


RESAMPLER_ANALYTIC = [
    # out given, kind, degree
    (False, 1, 3, 1, 'resampler_create_analytic: out is NULL'),
    (True, 0, 3, 1, 'resampler_create_analytic: kind 0'),
    (True, 3, 3, 1, 'resampler_create_analytic: kind 3'),
    (True, 2, 0, 1, 'resampler_create_analytic: Lagrange degree 0 (1..31)'),
    (True, 2, 32, 1, 'resampler_create_analytic: Lagrange degree 32 (1..31)'),
]


@pytest.mark.parametrize("out_given, kind, degree, status, text", RESAMPLER_ANALYTIC)
def test_resampler_create_analytic_refuses(out_given, kind, degree, status, text):
    h = C.c_void_p()
    assert refused('resampler_create_analytic', C.byref(h) if out_given else None, C64, 1.5, kind, degree) == (status, text)
    assert not h.value


STEP = [
    # handle given, n, x given
    ('resampler', False, 4, True, 1, 'resampler_step: NULL handle'),
    ('resampler', True, -1, True, 1, 'resampler_step: negative length'),
    ('resampler', True, 4, False, 1, 'resampler_step: NULL input'),
    ('polyfir', False, 4, True, 1, 'polyfir_step: NULL handle'),
    ('polyfir', True, -1, True, 1, 'polyfir_step: negative length'),
]


@pytest.mark.parametrize("op, handle_given, n, x_given, status, text", STEP)
def test_step_refuses(op, handle_given, n, x_given, status, text):
    x, y = np.zeros(16, np.complex64), np.zeros(64, np.complex64)
    got = C.c_int64(7)
    assert refused(op + '_step', NO_HANDLE.ctypes.data if handle_given else None, x.ctypes.data if x_given else None, n, y.ctypes.data, 64,
                   C.byref(got), None) == (status, text)


@pytest.mark.parametrize("op", ["resampler", "polyfir"])
def test_step_of_nothing_writes_a_zero_count(op):
    import libtsd_amd as t
    x, y = np.zeros(16, np.complex64), np.zeros(64, np.complex64)
    got = C.c_int64(7)
    assert getattr(t.lib(), f"tsdgpu_{op}_step")(NO_HANDLE.ctypes.data, x.ctypes.data, 0, y.ctypes.data, 64, C.byref(got), None) == 0
    assert got.value == 0


def test_null_handles_are_refused():
    assert refused('resampler_reset', None) == (1, 'resampler_reset: NULL handle')
    assert refused('resampler_seek', None, 0, None, None) == (1, 'resampler_seek: bad argument')
    assert refused('resampler_seek', NO_HANDLE.ctypes.data, -1, None, None) == (1, 'resampler_seek: bad argument')
    assert refused('polyfir_reset', None) == (1, 'polyfir_reset: NULL handle')


def test_counts_of_null_are_minus_one():
    import libtsd_amd as t
    L = t.lib()
    assert L.tsdgpu_resampler_out_count(None, 4) == -1
    assert L.tsdgpu_resampler_out_offset(None) == -1
    assert L.tsdgpu_polyfir_out_count(None, 4) == -1
    assert L.tsdgpu_polyfir_out_count(NO_HANDLE.ctypes.data, -1) == -1


@pytest.mark.parametrize("entry", ["resampler_destroy", "polyfir_destroy"])
def test_destroying_null_is_fine(entry):
    import libtsd_amd as t
    assert getattr(t.lib(), f"tsdgpu_{entry}")(None) == 0


POLYFIR_CREATE = [
    # out given, kind, data_type, taps given, ntaps, R
    (False, DECIM, C64, True, 15, 2, 1, 'polyfir_create: out is NULL'),
    (True, -1, C64, True, 15, 2, 1, 'polyfir_create: bad kind -1'),
    (True, 4, C64, True, 15, 2, 1, 'polyfir_create: bad kind 4'),
    (True, DECIM, 5, True, 15, 2, 1, 'polyfir_create: bad data_type 5'),
    (True, DECIM, C64, True, 15, 0, 1, 'polyfir_create: bad rate 0'),
    (True, DECIM, C64, True, 15, 4097, 1, 'polyfir_create: bad rate 4097'),
    (True, DECIM, C64, False, 15, 2, 1, 'polyfir_create: K > 0 required'),
    (True, DECIM, C64, True, 0, 2, 1, 'polyfir_create: K > 0 required'),
    (True, UPS, C64, True, 0, 2, 1, 'polyfir_create: K > 0 required'),
]


@pytest.mark.parametrize("out_given, kind, data_type, taps_given, ntaps, R, status, text", POLYFIR_CREATE)
def test_polyfir_create_refuses(out_given, kind, data_type, taps_given, ntaps, R, status, text):
    h = C.c_void_p()
    taps = np.ones(16, np.float32)
    assert refused('polyfir_create', C.byref(h) if out_given else None, kind, data_type, taps.ctypes.data if taps_given else None, ntaps,
                   R) == (status, text)
    assert not h.value
