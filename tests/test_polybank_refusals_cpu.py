"""What the polyphase banks refuse (include/tsdgpu.h: tsdgpu_channelizer_*, tsdgpu_synthesizer_*), through the C ABI: the status
and the whole text of tsdgpu_last_error().  Every check below runs before the first HIP call, so no GPU is needed.  The texts are
part of the interface (the adaptors and the callers' logs show them): they are literals here, not rebuilt from the code's rules."""
import ctypes as C

import numpy as np
import pytest

# the statuses in the tables: 1 = TSDGPU_ERR_INVALID, 3 = TSDGPU_ERR_UNSUPPORTED
COMPLEX = ("create_oversampled",)
REAL = ("create_real", "create_real_oversampled")


def create_cases():
    """(operator, entry, out given, channels, oversample, K) of every refused create"""
    rows = []
    for op in ("channelizer", "synthesizer"):
        for entry in COMPLEX + REAL:
            least = 16 if entry in REAL else 8
            rows += [(op, entry, False, 16, 1, 4), (op, entry, True, 0, 1, 4), (op, entry, True, 16, 0, 4), (op, entry, True, 16, 1, 0),
                     (op, entry, True, 24, 1, 4), (op, entry, True, least // 2, 1, 4), (op, entry, True, 2048, 1, 4),
                     (op, entry, True, 16, 3, 4)]
            if entry == "create_real":
                rows.append((op, entry, True, 16, 2, 4))
            rows.append((op, entry, True, 16, 1, 16 * 16 + 1))
            if entry != "create_real":
                rows += [(op, entry, True, 16, 2, 16 * 8 + 1), (op, entry, True, 16, 4, 16 * 4 + 1)]
    return rows


def create(op, entry, out_given, channels, oversample, K):
    import libtsd_amd as t
    L = t.lib()
    taps = np.ones(max(K, 1), np.float32)
    h = C.c_void_p()
    rc = getattr(L, f"tsdgpu_{op}_{entry}")(C.byref(h) if out_given else None, channels, oversample, taps.ctypes.data, K)
    assert not h.value
    return rc, L.tsdgpu_last_error().decode()


CREATE = [
    ('channelizer', 'create_oversampled', False, 16, 1, 4, 1,
     'channelizer_create: out is NULL'),
    ('channelizer', 'create_oversampled', True, 0, 1, 4, 1,
     'channelizer_create: channels = 0, need at least one'),
    ('channelizer', 'create_oversampled', True, 16, 0, 4, 1,
     'channelizer_create: oversample = 0, need at least one'),
    ('channelizer', 'create_oversampled', True, 16, 1, 0, 1,
     'channelizer_create: K > 0 taps required'),
    ('channelizer', 'create_oversampled', True, 24, 1, 4, 3,
     'channelizer_create: channels = 24: served are the powers of two from 8 to 1024'),
    ('channelizer', 'create_oversampled', True, 4, 1, 4, 3,
     'channelizer_create: channels = 4: served are the powers of two from 8 to 1024'),
    ('channelizer', 'create_oversampled', True, 2048, 1, 4, 3,
     'channelizer_create: channels = 2048: served are the powers of two from 8 to 1024'),
    ('channelizer', 'create_oversampled', True, 16, 3, 4, 3,
     'channelizer_create: oversample = 3: served are 1, 2 and 4'),
    ('channelizer', 'create_oversampled', True, 16, 1, 257, 3,
     'channelizer_create: 257 taps over 16 channels: served are up to 16 taps per channel (256 taps)'),
    ('channelizer', 'create_oversampled', True, 16, 2, 129, 3,
     'channelizer_create: 129 taps over 16 channels at hop 8: served are up to 16 taps per hop sample (128 taps)'),
    ('channelizer', 'create_oversampled', True, 16, 4, 65, 3,
     'channelizer_create: 65 taps over 16 channels at hop 4: served are up to 16 taps per hop sample (64 taps)'),
    ('channelizer', 'create_real', False, 16, 1, 4, 1,
     'channelizer_create_real: out is NULL'),
    ('channelizer', 'create_real', True, 0, 1, 4, 1,
     'channelizer_create_real: channels = 0, need at least one'),
    ('channelizer', 'create_real', True, 16, 0, 4, 1,
     'channelizer_create_real: oversample = 0, need at least one'),
    ('channelizer', 'create_real', True, 16, 1, 0, 1,
     'channelizer_create_real: K > 0 taps required'),
    ('channelizer', 'create_real', True, 24, 1, 4, 3,
     'channelizer_create_real: channels = 24: served are the powers of two from 16 to 1024'),
    ('channelizer', 'create_real', True, 8, 1, 4, 3,
     'channelizer_create_real: channels = 8: served are the powers of two from 16 to 1024'),
    ('channelizer', 'create_real', True, 2048, 1, 4, 3,
     'channelizer_create_real: channels = 2048: served are the powers of two from 16 to 1024'),
    ('channelizer', 'create_real', True, 16, 3, 4, 3,
     'channelizer_create_real: oversample = 3: served is 1 (tsdgpu_channelizer_create_real_oversampled serves 2 and 4)'),
    ('channelizer', 'create_real', True, 16, 2, 4, 3,
     'channelizer_create_real: oversample = 2: served is 1 (tsdgpu_channelizer_create_real_oversampled serves 2 and 4)'),
    ('channelizer', 'create_real', True, 16, 1, 257, 3,
     'channelizer_create_real: 257 taps over 16 channels: served are up to 16 taps per channel (256 taps)'),
    ('channelizer', 'create_real_oversampled', False, 16, 1, 4, 1,
     'channelizer_create_real_oversampled: out is NULL'),
    ('channelizer', 'create_real_oversampled', True, 0, 1, 4, 1,
     'channelizer_create_real_oversampled: channels = 0, need at least one'),
    ('channelizer', 'create_real_oversampled', True, 16, 0, 4, 1,
     'channelizer_create_real_oversampled: oversample = 0, need at least one'),
    ('channelizer', 'create_real_oversampled', True, 16, 1, 0, 1,
     'channelizer_create_real_oversampled: K > 0 taps required'),
    ('channelizer', 'create_real_oversampled', True, 24, 1, 4, 3,
     'channelizer_create_real_oversampled: channels = 24: served are the powers of two from 16 to 1024'),
    ('channelizer', 'create_real_oversampled', True, 8, 1, 4, 3,
     'channelizer_create_real_oversampled: channels = 8: served are the powers of two from 16 to 1024'),
    ('channelizer', 'create_real_oversampled', True, 2048, 1, 4, 3,
     'channelizer_create_real_oversampled: channels = 2048: served are the powers of two from 16 to 1024'),
    ('channelizer', 'create_real_oversampled', True, 16, 3, 4, 3,
     'channelizer_create_real_oversampled: oversample = 3: served are 1, 2 and 4'),
    ('channelizer', 'create_real_oversampled', True, 16, 1, 257, 3,
     'channelizer_create_real_oversampled: 257 taps over 16 channels at hop 16: served are up to 16 taps per hop sample (256 taps)'),
    ('channelizer', 'create_real_oversampled', True, 16, 2, 129, 3,
     'channelizer_create_real_oversampled: 129 taps over 16 channels at hop 8: served are up to 16 taps per hop sample (128 taps)'),
    ('channelizer', 'create_real_oversampled', True, 16, 4, 65, 3,
     'channelizer_create_real_oversampled: 65 taps over 16 channels at hop 4: served are up to 16 taps per hop sample (64 taps)'),
    ('synthesizer', 'create_oversampled', False, 16, 1, 4, 1,
     'synthesizer_create: out is NULL'),
    ('synthesizer', 'create_oversampled', True, 0, 1, 4, 1,
     'synthesizer_create: channels = 0, need at least one'),
    ('synthesizer', 'create_oversampled', True, 16, 0, 4, 1,
     'synthesizer_create: oversample = 0, need at least one'),
    ('synthesizer', 'create_oversampled', True, 16, 1, 0, 1,
     'synthesizer_create: K > 0 taps required'),
    ('synthesizer', 'create_oversampled', True, 24, 1, 4, 3,
     'synthesizer_create: channels = 24: served are the powers of two from 8 to 1024'),
    ('synthesizer', 'create_oversampled', True, 4, 1, 4, 3,
     'synthesizer_create: channels = 4: served are the powers of two from 8 to 1024'),
    ('synthesizer', 'create_oversampled', True, 2048, 1, 4, 3,
     'synthesizer_create: channels = 2048: served are the powers of two from 8 to 1024'),
    ('synthesizer', 'create_oversampled', True, 16, 3, 4, 3,
     'synthesizer_create: oversample = 3: served are 1, 2 and 4'),
    ('synthesizer', 'create_oversampled', True, 16, 1, 257, 3,
     'synthesizer_create: 257 taps over 16 channels: served are up to 16 taps per channel (256 taps)'),
    ('synthesizer', 'create_oversampled', True, 16, 2, 129, 3,
     'synthesizer_create: 129 taps over 16 channels at hop 8: served are up to 16 taps per hop sample (128 taps)'),
    ('synthesizer', 'create_oversampled', True, 16, 4, 65, 3,
     'synthesizer_create: 65 taps over 16 channels at hop 4: served are up to 16 taps per hop sample (64 taps)'),
    ('synthesizer', 'create_real', False, 16, 1, 4, 1,
     'synthesizer_create_real: out is NULL'),
    ('synthesizer', 'create_real', True, 0, 1, 4, 1,
     'synthesizer_create_real: channels = 0, need at least one'),
    ('synthesizer', 'create_real', True, 16, 0, 4, 1,
     'synthesizer_create_real: oversample = 0, need at least one'),
    ('synthesizer', 'create_real', True, 16, 1, 0, 1,
     'synthesizer_create_real: K > 0 taps required'),
    ('synthesizer', 'create_real', True, 24, 1, 4, 3,
     'synthesizer_create_real: channels = 24: served are the powers of two from 16 to 1024'),
    ('synthesizer', 'create_real', True, 8, 1, 4, 3,
     'synthesizer_create_real: channels = 8: served are the powers of two from 16 to 1024'),
    ('synthesizer', 'create_real', True, 2048, 1, 4, 3,
     'synthesizer_create_real: channels = 2048: served are the powers of two from 16 to 1024'),
    ('synthesizer', 'create_real', True, 16, 3, 4, 3,
     'synthesizer_create_real: oversample = 3: this entry serves 1 only (2 and 4: synthesizer_create_real_oversampled)'),
    ('synthesizer', 'create_real', True, 16, 2, 4, 3,
     'synthesizer_create_real: oversample = 2: this entry serves 1 only (2 and 4: synthesizer_create_real_oversampled)'),
    ('synthesizer', 'create_real', True, 16, 1, 257, 3,
     'synthesizer_create_real: 257 taps over 16 channels: served are up to 16 taps per channel (256 taps)'),
    ('synthesizer', 'create_real_oversampled', False, 16, 1, 4, 1,
     'synthesizer_create_real_oversampled: out is NULL'),
    ('synthesizer', 'create_real_oversampled', True, 0, 1, 4, 1,
     'synthesizer_create_real_oversampled: channels = 0, need at least one'),
    ('synthesizer', 'create_real_oversampled', True, 16, 0, 4, 1,
     'synthesizer_create_real_oversampled: oversample = 0, need at least one'),
    ('synthesizer', 'create_real_oversampled', True, 16, 1, 0, 1,
     'synthesizer_create_real_oversampled: K > 0 taps required'),
    ('synthesizer', 'create_real_oversampled', True, 24, 1, 4, 3,
     'synthesizer_create_real_oversampled: channels = 24: served are the powers of two from 16 to 1024'),
    ('synthesizer', 'create_real_oversampled', True, 8, 1, 4, 3,
     'synthesizer_create_real_oversampled: channels = 8: served are the powers of two from 16 to 1024'),
    ('synthesizer', 'create_real_oversampled', True, 2048, 1, 4, 3,
     'synthesizer_create_real_oversampled: channels = 2048: served are the powers of two from 16 to 1024'),
    ('synthesizer', 'create_real_oversampled', True, 16, 3, 4, 3,
     'synthesizer_create_real_oversampled: oversample = 3: served are 1, 2 and 4'),
    ('synthesizer', 'create_real_oversampled', True, 16, 1, 257, 3,
     'synthesizer_create_real_oversampled: 257 taps over 16 channels at hop 16: served are up to 16 taps per hop sample (256 taps)'),
    ('synthesizer', 'create_real_oversampled', True, 16, 2, 129, 3,
     'synthesizer_create_real_oversampled: 129 taps over 16 channels at hop 8: served are up to 16 taps per hop sample (128 taps)'),
    ('synthesizer', 'create_real_oversampled', True, 16, 4, 65, 3,
     'synthesizer_create_real_oversampled: 65 taps over 16 channels at hop 4: served are up to 16 taps per hop sample (64 taps)'),
]


def test_the_table_holds_every_case():
    assert [row[:6] for row in CREATE] == create_cases()


@pytest.mark.parametrize("op, entry, out_given, channels, oversample, K, status, text", CREATE)
def test_create_refuses(op, entry, out_given, channels, oversample, K, status, text):
    assert create(op, entry, out_given, channels, oversample, K) == (status, text)


@pytest.mark.parametrize("op", ["channelizer", "synthesizer"])
def test_plain_create_is_the_oversampled_entry_at_one(op):
    import libtsd_amd as t
    L = t.lib()
    taps = np.ones(16 * 16 + 1, np.float32)
    for channels, K in ((24, 4), (4, 4), (16, 16 * 16 + 1)):
        h = C.c_void_p()
        rc = getattr(L, f"tsdgpu_{op}_create")(C.byref(h), channels, taps.ctypes.data, K)
        assert not h.value
        assert (rc, L.tsdgpu_last_error().decode()) == create(op, "create_oversampled", True, channels, 1, K)


NULL_STATUS_OPS = ("step", "reset", "set_phase", "get_state", "set_state")


def null_op(op, name):
    import libtsd_amd as t
    L = t.lib()
    buf = np.zeros(64, np.complex64)
    p, got = buf.ctypes.data, C.c_int64(7)
    args = {"step": (None, p, 16, p, 16, 16, C.byref(got), None), "reset": (None,), "set_phase": (None, 1),
            "get_state": (None, p, None), "set_state": (None, p, None)}[name]
    rc = getattr(L, f"tsdgpu_{op}_{name}")(*args)
    assert got.value == 7      # (a refused step does not touch n_out)
    return rc, L.tsdgpu_last_error().decode()


NULL_OPS = [
    ('channelizer', 'step', 1, 'channelizer_step: NULL handle'),
    ('channelizer', 'reset', 1, 'channelizer_reset: NULL handle'),
    ('channelizer', 'set_phase', 1, 'channelizer_set_phase: NULL handle'),
    ('channelizer', 'get_state', 1, 'channelizer_get_state: NULL handle'),
    ('channelizer', 'set_state', 1, 'channelizer_set_state: NULL handle'),
    ('synthesizer', 'step', 1, 'synthesizer_step: NULL handle'),
    ('synthesizer', 'reset', 1, 'synthesizer_reset: NULL handle'),
    ('synthesizer', 'set_phase', 1, 'synthesizer_set_phase: NULL handle'),
    ('synthesizer', 'get_state', 1, 'synthesizer_get_state: NULL handle'),
    ('synthesizer', 'set_state', 1, 'synthesizer_set_state: NULL handle'),
]


def test_null_table_holds_every_case():
    assert [row[:2] for row in NULL_OPS] == [(op, name) for op in ("channelizer", "synthesizer") for name in NULL_STATUS_OPS]


@pytest.mark.parametrize("op, name, status, text", NULL_OPS)
def test_null_handle_is_refused(op, name, status, text):
    assert null_op(op, name) == (status, text)


@pytest.mark.parametrize("op", ["channelizer", "synthesizer"])
def test_null_handle_counts_are_minus_one(op):
    import libtsd_amd as t
    L = t.lib()
    assert getattr(L, f"tsdgpu_{op}_out_count")(None, 5) == -1
    for name in ("hop", "history_len", "get_phase", "rows", "is_real"):
        assert getattr(L, f"tsdgpu_{op}_{name}")(None) == -1, name


@pytest.mark.parametrize("op", ["channelizer", "synthesizer"])
def test_destroying_null_is_fine(op):
    import libtsd_amd as t
    assert getattr(t.lib(), f"tsdgpu_{op}_destroy")(None) == 0
