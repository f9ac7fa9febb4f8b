"""What the FFT entry points refuse (include/tsdgpu.h: tsdgpu_fft_*, tsdgpu_rfft_*, tsdgpu_fftshift), through the C ABI: the status
and the whole text of tsdgpu_last_error().  Every check below runs before the first HIP call, so no GPU is needed.  The texts are
part of the interface (the adaptors and the callers' logs show them): they are literals here, not rebuilt from the code's rules."""
import ctypes as C

import numpy as np
import pytest

# the status in the tables: 1 = TSDGPU_ERR_INVALID


def refused(entry, *args):
    import libtsd_amd as t
    L = t.lib()
    rc = getattr(L, f"tsdgpu_{entry}")(*args)
    return rc, L.tsdgpu_last_error().decode()


CREATE = [
    ('fft_create', False, (0, 0), 1, 'fft_create: out is NULL'),
    ('fft_create', True, (0, 0), 1, 'fft_create: n must be >= 1 (got 0)'),
    ('fft_create', True, ((1 << 28) + 1, 0), 1, 'fft_create: n = 268435457 too large (limit 2^28)'),
    ('rfft_create', False, (0,), 1, 'rfft_create: out is NULL'),
    ('rfft_create', True, (0,), 1, 'rfft_create: n must be >= 1 (got 0)'),
]


@pytest.mark.parametrize("entry, out_given, rest, status, text", CREATE)
def test_create_refuses(entry, out_given, rest, status, text):
    h = C.c_void_p()
    assert refused(entry, C.byref(h) if out_given else None, *rest) == (status, text)
    assert not h.value


# a step looks at the plan only once its other arguments have passed: the negative batch is refused on a handle that is no plan
STEP = [
    ('fft_step', False, 1, 1, 'fft_step: NULL plan'),
    ('fft_step', True, -1, 1, 'fft_step: negative batch'),
    ('rfft_step', False, 1, 1, 'rfft_step: NULL plan'),
    ('rfft_step', True, -1, 1, 'rfft_step: negative batch'),
]


@pytest.mark.parametrize("entry, plan_given, batch, status, text", STEP)
def test_step_refuses(entry, plan_given, batch, status, text):
    no_plan = np.zeros(4096, np.uint8)
    x, y = np.zeros(16, np.complex64), np.zeros(16, np.complex64)
    args = (no_plan.ctypes.data if plan_given else None, x.ctypes.data, y.ctypes.data, batch) + ((1, None) if entry == 'fft_step' else (None,))
    assert refused(entry, *args) == (status, text)


SHIFT = [
    (-1, False, 1, 'fftshift: negative length'),
    (16, True, 1, 'fftshift: needs distinct non-NULL buffers'),
]


@pytest.mark.parametrize("n, same, status, text", SHIFT)
def test_fftshift_refuses(n, same, status, text):
    x, y = np.zeros(16, np.complex64), np.zeros(16, np.complex64)
    assert refused('fftshift', x.ctypes.data, (x if same else y).ctypes.data, n, 1, None) == (status, text)


def test_size_of_null_is_minus_one():
    import libtsd_amd as t
    assert t.lib().tsdgpu_fft_size(None) == -1


@pytest.mark.parametrize("entry", ["fft_destroy", "rfft_destroy"])
def test_destroying_null_is_fine(entry):
    import libtsd_amd as t
    assert getattr(t.lib(), f"tsdgpu_{entry}")(None) == 0
