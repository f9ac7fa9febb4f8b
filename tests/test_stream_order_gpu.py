"""The stream promise of include/tsdgpu.h ("calls with device pointers are asynchronous on that stream"), held on NON-BLOCKING
side streams: every Python class and function of libtsd_amd/capi.py that reaches a kernel with device pointers, compared bit
for bit with a synchronised run on the default stream (tests/stream_order.py: the harness, the operator table and CONTRACT, the
table of DESIGN.md "The stream contract").

  A  one side stream, three ragged steps back to back behind the delay, no host wait between them
  B  step 1 on s1 behind the delay, an event, steps 2 and 3 on s2
  C  the layouts that take private copies: in place, a view one sample past a 16-byte boundary, a row stride larger than n
  D  one Fft / Rfft plan stepped from two streams with no caller event (StepOrder)
  E  step, reset_on, step on one stream
  F  the state read out behind the delay and fed to a fresh handle on a second stream
  G  a host-array call on a second handle / a stateless call on another stream while a side stream sleeps with a step pending

Every case prints the calibrated delay and whether `gate` was still pending when each call under test returned."""
import numpy as np
import pytest

import stream_order as so

pytestmark = pytest.mark.gpu

import libtsd_amd as _t          # noqa: E402  (no device is touched at import: the library loads on first use)

OPS = so.operators(_t)
BY_NAME = {o.name: o for o in OPS}
_REF = {}


def ref_of(op, warmed, layout="plain"):
    """the reference run of (operator, warm or cold, layout): computed once, shared, never changed"""
    key = (op.name, warmed, layout)
    if key not in _REF:
        _REF[key] = so.reference(op, warmed, layout)
    return _REF[key]


@pytest.fixture(scope="module")
def delay():
    import torch
    assert torch.cuda.is_available() and _t.device_count() >= 1
    d = so.Delay()
    print(f"[stream-order] delay: {d.kind}({d.arg}) measured {d.ms:.1f} ms (target {so.TARGET_MS} ms)")
    assert d.ms >= so.MIN_MS, f"the device-side delay reached {d.ms:.1f} ms only"
    return d


@pytest.fixture(scope="module")
def side():
    import torch
    return torch.cuda.Stream(), torch.cuda.Stream()


# ------------------------------------------------------------------------------------------------ the harness itself
def test_side_streams_are_non_blocking(side):
    """torch's side streams must be non-blocking, or the null stream would order everything and the module would prove nothing.
    hipStreamGetFlags through ctypes on the runtime already loaded; a runtime whose symbol cannot be reached is reported, not
    assumed (DESIGN.md names this case)."""
    for s in side:
        flags, why = so.stream_flags(s)
        print(f"[stream-order] side stream {s.cuda_stream:#x}: flags {flags} {why or ''}")
        assert flags is not None, f"hipStreamGetFlags could not be reached: {why}"
        assert flags & 1, f"torch.cuda.Stream() is a BLOCKING stream here (flags {flags})"


def _fake(call):
    x = [so.rand(n, False, n) for n in so.STEPS]
    return so.Op("fake", lambda: None, x, call, lambda a: (a.shape, a.dtype), None)


def test_harness_catches_work_on_the_default_stream(delay, side):
    """a torch-only fake step that does its arithmetic on the default stream: it reads x before the producer behind the delay
    has written it (NaN poison, nothing else), and the bit comparison must fail"""
    import torch

    def call(h, x, y, cs):
        with torch.cuda.stream(torch.cuda.default_stream()):
            torch.mul(x, 2.0, out=y)
        return y
    op = _fake(call)
    want = so.reference(op, False)
    r, got = so.under_test(op, [side[0]] * 3, delay, False)
    with pytest.raises(AssertionError, match="bits differ"):
        so.check("fake on the default stream", want, got, r.pending, delay, True)
    assert all(r.pending), "the fake does not wait on the host: gate must still be pending"


def test_harness_catches_a_host_wait(delay, side):
    """a torch-only fake step that synchronises its stream: the bits are right, the gate assertion must fail"""
    import torch

    def call(h, x, y, cs):
        torch.mul(x, 2.0, out=y)
        torch.cuda.current_stream().synchronize()
        return y
    op = _fake(call)
    want = so.reference(op, False)
    r, got = so.under_test(op, [side[0]] * 3, delay, False)
    so.check("fake with a host wait, bits only", want, got, r.pending, delay, None)
    with pytest.raises(AssertionError, match="host wait"):
        so.check("fake with a host wait", want, got, r.pending, delay, True)


def test_expectations_come_from_the_contract():
    """every operator of the table names an entry point of CONTRACT, and DESIGN.md's table says the same (the full comparison,
    header included, runs without a GPU in test_stream_contract_cpu.py)"""
    for op in OPS:
        assert op.entry in so.CONTRACT, op.name


# ------------------------------------------------------------------------------------------------------ A and B
@pytest.mark.parametrize("name", [o.name for o in OPS])
def test_a_one_side_stream(name, delay, side):
    op = BY_NAME[name]
    r, got = so.under_test(op, [side[0]] * len(op.xs), delay, True)
    so.check(f"A {name}", ref_of(op, True), got, r.pending, delay, op.expect_async)


@pytest.mark.parametrize("name", [o.name for o in OPS])
def test_a_cold_first_step(name, delay, side):
    """the handle's very first step behind the delay (first-use memsets and uploads on the wrong stream): bits only"""
    op = BY_NAME[name]
    r, got = so.under_test(op, [side[0]] * len(op.xs), delay, False)
    so.check(f"A cold {name}", ref_of(op, False), got, r.pending, delay, None)


@pytest.mark.parametrize("name", [o.name for o in OPS])
def test_b_hand_over_between_streams(name, delay, side):
    op = BY_NAME[name]
    r, got = so.under_test(op, [side[0]] + [side[1]] * (len(op.xs) - 1), delay, True)
    so.check(f"B {name}", ref_of(op, True), got, r.pending, delay, op.expect_async)


# ------------------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("name,layout", [(o.name, l) for o in OPS for l in o.layouts])
def test_c_layouts_with_private_copies(name, layout, delay, side):
    op = BY_NAME[name]
    r, got = so.under_test(op, [side[0]] * len(op.xs), delay, True, layout)
    so.check(f"C {name} {layout}", ref_of(op, True, layout), got, r.pending, delay, op.expect_async)


# ------------------------------------------------------------------------------------------------------------- D
# (kind, n, batch): plans that own scratch or counters, at batches of 2^21 .. 2^24 points, so that a step lasts long enough to
# meet the other stream's; 2^20 x 16 is the smallest step that takes the two-pass kernel's dynamic tile hand-out (64 tiles per
# transform against 4 x the CU count), the device counters whose base the plan tracks on the host
D_PLANS = [("fft", 1 << 15, 128), ("fft", 3 << 10, 1024), ("fft", 1000, 4096), ("fft", 1001, 2048), ("rfft", 4096, 1024),
           ("fft", 1 << 20, 16)]


@pytest.mark.parametrize("how", ["s2-free", "together"])
@pytest.mark.parametrize("kind,n,batch", D_PLANS)
def test_d_one_plan_two_streams_no_caller_event(kind, n, batch, how, delay, side):
    """StepOrder: the plan's scratch and tile counters are shared, so the step on s2 must wait for the one on s1 by itself.
    s2-free: s1 sleeps the delay and s2 does not, so nothing but the plan's own event keeps the second step from running FIRST
    (a tile counter whose base the host advanced at enqueue time then hands out nothing).  together: s2 waits for `gate`, the
    event recorded on s1 BEHIND the delay and IN FRONT of s1's producer and step, so both streams become runnable at the same
    instant and the two steps may meet on the plan's scratch.  (What a scratch build whose StepOrder::enter does not wait
    makes of these cases: DESIGN.md, "The stream contract".)"""
    cplx = kind == "fft"
    x1 = so.rand2(batch, n, cplx, 300 + n)
    xs = [x1, np.ascontiguousarray(np.roll(x1, 1, axis=1) * np.float32(0.5))]
    make = (lambda: _t.Fft(n)) if cplx else (lambda: _t.Rfft(n))
    call = so._fft_step if cplx else so._step
    op = so.Op(f"{kind}-{n}-two-streams", make, xs, call, lambda x: (x.shape, np.complex64), f"tsdgpu_{kind}_step")
    want = so.reference(op, True)
    h = op.make()
    so.warm(op, h)
    r = so.Run(op)
    s1, s2 = side
    r.head(s1, delay)
    if how == "together":
        s2.wait_event(r.gate)
    r.step(h, 0, s1)
    r.step(h, 1, s2)
    s1.synchronize()
    s2.synchronize()
    so.check(f"D {op.name} {how}", want, r.results(), r.pending, delay, True)


# ------------------------------------------------------------------------------------------------------------- E
@pytest.mark.parametrize("name", [o.name for o in OPS if o.family in ("fir", "sos", "spectrum")])
def test_e_reset_on_the_stream(name, delay, side):
    """step, reset_on (Spectrum: reset(stream), its reset_on), step on one stream behind the delay: the second output is a
    fresh handle's"""
    import torch
    op = BY_NAME[name]
    xs = [op.xs[0], op.xs[2]]
    one = lambda x: so.Op(op.name, op.make, [x], op.call, op.ycap, op.entry, op.reset)
    want = so.reference(one(xs[0]), True) + so.reference(one(xs[1]), True)
    h = op.make()
    so.warm(op, h)
    r = so.Run(op, xs=xs)
    s = side[0]
    r.head(s, delay)
    r.step(h, 0, s)
    with torch.cuda.stream(s):
        if op.family == "spectrum":
            h.reset(stream=s.cuda_stream)
        else:
            h.reset_on(stream=s.cuda_stream)
        r.note()
    r.step(h, 1, s)
    s.synchronize()
    so.check(f"E {name}", want, r.results(), r.pending, delay, True)


# ------------------------------------------------------------------------------------------------------------- F
def _state_io(op, h):
    """(shape, numpy dtype, get(h, dst, cs) -> host part, put(h, src, host part, cs)) of the family's device-side state move"""
    fam, x = op.family, op.xs[0]
    def get_hist(h, d, cs):
        h.get_history(d, stream=cs)

    def put_hist(h, d, e, cs):
        h.set_history(d, stream=cs)
    if fam == "fir":
        return (h.K - 1,), x.dtype, get_hist, put_hist
    if fam == "firbank":
        return (h.channels, h.K - 1), x.dtype, get_hist, put_hist
    if fam == "polyfirbank":
        return (h.channels, h.history_len), x.dtype, (lambda h, d, cs: h.get_state(d, stream=cs)[1]), \
            (lambda h, d, e, cs: h.set_state(d, e, stream=cs))

    def get(h, d, cs):
        h.get_state(d, stream=cs)
        return getattr(h, "phase", 0)

    def put(h, d, e, cs):
        h.set_state(d, stream=cs)
        if hasattr(type(h), "phase"):
            h.phase = e
    if fam in ("channelizer", "rchannelizer"):
        return (h.history_len,), x.dtype, get, put
    if fam == "synthesizer":
        return (h.channels, h.frames_kept), np.complex64, get, put
    if fam == "rsynthesizer":
        return (h.rows, h.frames_kept), np.complex64, get, put
    raise KeyError(fam)


# the schemes whose bits do not depend on where the stream was cut (the direct FIR, the rate banks, the polyphase banks): the
# moved stream is ALSO the uninterrupted one, bit for bit.  The overlap-save, long and partitioned plans promise that to 1e-5
# only (their transforms see a longer history than the K - 1 samples that move), so they are held to the same move made
# synchronously on the default stream.
F_UNCUT = [o.name for o in OPS if o.family in ("firbank", "polyfirbank", "channelizer", "rchannelizer", "synthesizer", "rsynthesizer")
           and "ols" not in o.name] + ["fir-direct31-f32", "fir-direct31-c64", "fir-direct31-c64-ctaps"]
F_DEVICE = F_UNCUT + [o.name for o in OPS if o.family in ("fir", "firbank") and o.name not in F_UNCUT]


def _state_move(op, s1, s2, delay):
    """step 1 on handle a (s1), its state into a device buffer on s1, an event, the state into the fresh handle b on s2,
    steps 2 and 3 on b.  delay None: the synchronised reference on the default stream."""
    import torch
    sync = torch.cuda.synchronize if delay is None else (lambda: None)
    a, b = op.make(), op.make()
    so.warm(op, a)
    so.warm(op, b)
    shape, dt, get, put = _state_io(op, a)
    st_dev = so.alloc(shape, dt, "plain", so.POISON_X)
    r = so.Run(op)
    r.extra += [a, b, st_dev]
    if delay is not None:
        r.head(s1, delay)
    r.step(a, 0, s1, sync=delay is None)
    with torch.cuda.stream(s1):
        extra = get(a, st_dev, s1.cuda_stream)
        r.note()
        sync()
    if s1 is not s2:
        r.hand_over(s1, s2)
    with torch.cuda.stream(s2):
        put(b, st_dev, extra, s2.cuda_stream)
        r.note()
        sync()
    r.step(b, 1, s2, sync=delay is None)
    r.step(b, 2, s2, sync=delay is None)
    s1.synchronize()
    s2.synchronize()
    return r, r.results()


@pytest.mark.parametrize("name", F_DEVICE)
def test_f_state_moves_with_device_destinations(name, delay, side):
    """get_history / get_state into a device buffer behind the delay on s1, an event, set_history / set_state of a fresh
    handle on s2, which continues: the bits of the same move made synchronously on the default stream and, for the schemes of
    F_UNCUT, of the uninterrupted stream"""
    op = BY_NAME[name]
    d = so.default_stream()
    _, want = _state_move(op, d, d, None)
    r, got = _state_move(op, side[0], side[1], delay)
    so.check(f"F {name}", want, got, r.pending, delay, True)
    if name in F_UNCUT:
        so.check(f"F {name} against the uninterrupted stream", ref_of(op, True), got, r.pending, delay, True)


@pytest.mark.parametrize("name", ["resampler-k15-c64", "resampler-k31-f32", "resampler-k127-c64", "resampler-lagrange3-f32"])
def test_f_resampler_seek_with_a_device_history(name, delay, side):
    """tsdgpu_resampler_seek with a device history is ordered on the stream: the K - 1 samples before position n0 are produced
    behind the delay, a fresh handle seeks to n0 with them and takes steps 2 and 3: the uninterrupted stream, bit for bit (the
    sharding hook: position, phase and output offset follow the recurrence)"""
    import torch
    op = BY_NAME[name]
    b = op.make()
    so.warm(op, b)
    n0, K = op.xs[0].shape[0], b.K
    src = torch.from_numpy(np.ascontiguousarray(op.xs[0][n0 - (K - 1):])).cuda()
    hist = so.alloc((K - 1,), op.xs[0].dtype, "plain", so.POISON_X)
    r = so.Run(op)
    s = side[0]
    r.head(s, delay)
    with torch.cuda.stream(s):
        hist.copy_(src)
        b.seek(n0, hist, stream=s.cuda_stream)
        r.note()
    r.step(b, 1, s)
    r.step(b, 2, s)
    with torch.cuda.stream(s):
        hist.fill_(float("nan"))
    s.synchronize()
    want = [None] + ref_of(op, True)[1:]
    so.check(f"F seek {name}", want, r.results(), r.pending, delay, True)


@pytest.mark.parametrize("name", ["fir-ols127-f32", "fir-ols127-c64", "resampler-k15-f32", "resampler-k15-c64"])
def test_tile_counters_with_a_host_tracked_base(name, delay, side, monkeypatch):
    """the dynamic tile hand-out (device counters whose base the host tracks from launch to launch, a memset when the counter
    count changes) starts at sizes far above these; the developer switches, read at every step, bring it down to them
    (tests/test_fir_gpu.py and tests/test_resample_gpu.py hold its parity the same way).  Scenarios A and B."""
    monkeypatch.setenv("TSDGPU_OLS_DYN_MIN", "0")
    monkeypatch.setenv("TSDGPU_RS_DYN_MIN", "0")
    op = BY_NAME[name]
    want = so.reference(op, True)
    for tag, streams in (("A", [side[0]] * 3), ("B", [side[0], side[1], side[1]])):
        r, got = so.under_test(op, streams, delay, True)
        so.check(f"{tag} dynamic hand-out {name}", want, got, r.pending, delay, True)


@pytest.mark.parametrize("name", ["sos-butter12-f32", "sos-butter12-c64", "sosbank-butter12-c64"])
def test_f_state_moves_through_the_host(name, delay, side):
    """tsdgpu_sos_get_state / set_state and the bank's take HOST vectors: host-synchronous by contract, so only the order is
    held -- the state read on s1 behind the delay is the state after step 1, and the continued stream has the reference bits"""
    import torch
    op = BY_NAME[name]
    a, b = op.make(), op.make()
    so.warm(op, a)
    so.warm(op, b)
    r = so.Run(op)
    s1, s2 = side
    r.head(s1, delay)
    r.step(a, 0, s1)
    chans = range(a.channels) if op.family == "sosbank" else [None]
    with torch.cuda.stream(s1):
        states = [a.get_state(stream=s1.cuda_stream) if c is None else a.get_state(c, stream=s1.cuda_stream) for c in chans]
    with torch.cuda.stream(s2):
        for c, st in zip(chans, states):
            if c is None:
                b.set_state(st, stream=s2.cuda_stream)
            else:
                b.set_state(c, st, stream=s2.cuda_stream)
    r.step(b, 1, s2)
    r.step(b, 2, s2)
    s2.synchronize()
    so.check(f"F host {name}", ref_of(op, True), r.results(), r.pending, delay, None)


# ------------------------------------------------------------------------------------------------------------- G
def _families():
    seen, out = set(), []
    for o in OPS:
        if o.family in seen or o.ycap(o.xs[0]) is None or o.family in ("fir_after", "vec_op", "sos_skip"):
            continue
        seen.add(o.family)
        out.append(o.name)
    return out


@pytest.mark.parametrize("name", _families())
def test_g_host_call_while_a_side_stream_sleeps(name, delay, side):
    """a step pending behind the delay on s; meanwhile a HOST-array call on a second handle of the same kind on the default
    stream (the per-thread bounce buffers, the handle-independent scratch): both right"""
    op = BY_NAME[name]
    one = so.Op(op.name, op.make, [op.xs[0]], op.call, op.ycap, op.entry, op.reset)
    want_host = np.asarray(op.call(op.make(), op.xs[0].copy(), None, None))
    h, h2 = op.make(), op.make()
    so.warm(one, h)
    r = so.Run(one)
    s = side[0]
    r.head(s, delay)
    r.step(h, 0, s)
    got_host = np.asarray(op.call(h2, op.xs[0].copy(), None, None))
    still = not r.gate.query()
    s.synchronize()
    print(f"[stream-order] G {name}: side stream still asleep after the host call: {still}")
    so.check(f"G {name}", so.reference(one, True), r.results(), r.pending, delay, op.expect_async)
    assert np.array_equal(so.bits(want_host), so.bits(got_host)), f"G {name}: the host-array call on the default stream went wrong"


@pytest.mark.parametrize("name", ["xcorr", "welch", "delay_estimate"])
def test_g_stateless_call_on_another_stream(name, delay, side):
    """the stateless entry points hand their context (plan, scratch) from one call to the next through a reserve: a FIR step
    pending behind the delay on s1, the entry point once on the default stream and once more on s2 (the context of the first
    call is reused): both results right, and the pending step keeps the reference bits"""
    import torch
    op, fir = BY_NAME[name], BY_NAME["fir-ols127-c64"]
    one = so.Op(fir.name, fir.make, [fir.xs[0]], fir.call, fir.ycap, fir.entry, fir.reset)
    want = so.reference(op, True)
    h = fir.make()
    so.warm(one, h)
    so.warm(op, None)
    r, q1, q2 = so.Run(one), so.Run(op), so.Run(op)
    s1, s2 = side
    r.head(s1, delay)
    r.step(h, 0, s1)
    for i in range(len(op.xs)):
        q1.step(None, i, so.default_stream())
        q2.step(None, i, s2)
    s1.synchronize()
    s2.synchronize()
    so.check(f"G {name}: the pending FIR step", so.reference(one, True), r.results(), r.pending, delay, True)
    so.check(f"G {name} on the default stream", want, q1.results(), q1.pending, delay, None)
    so.check(f"G {name} on a second stream", want, q2.results(), q2.pending, delay, None)
