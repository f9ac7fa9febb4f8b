"""Stream-order harness: one operator, one input, two runs compared bit for bit.  Test helper, not a conftest.

include/tsdgpu.h promises that a call with device pointers is asynchronous on the caller's stream (the table of DESIGN.md,
"The stream contract"; CONTRACT below is the same table).  On torch's default stream the runtime serialises everything whatever
the library does, so the runs under test go to NON-BLOCKING side streams, behind a device-side delay:

  reference run    a fresh handle on the default stream, a device synchronise after every action.
  run under test   a fresh handle; every tensor allocated (and poisoned) before the run and kept alive until after the last
                   synchronise (no record_stream).  On the side stream: delay, event `gate`, then per step
                       producer  x_dev.copy_(x_src)         x_dev held NaN, y_dev a NaN of another payload
                       the call under test                  gate.query() read directly after it returns
                       consumer  y_keep.copy_(y_dev)
                       x_dev.fill_(nan)                     a step that still reads x after returning reads poison
                   and one synchronise at the very end.

What the bits catch: an internal launch, copy or memset on the null stream (it runs while the side stream still sleeps, reads
the NaN poison or an old state, or is overtaken), state updated outside the stream, x used after the return.  What `gate`
catches: gate.query() is False while the delay still runs, so False proves the call was enqueued before its input existed and
did not wait on the host; a call the contract lists as asynchronous must leave it False.  The asynchrony assertion is made on
a WARM handle (one pass of the same shapes, then back to the fresh state: first-use allocation may wait on the device); the
bits are also compared COLD, on the handle's very first step.

Nothing here faults: the poison is NaN in buffers that stay allocated; a racing step reads wrong values, never unmapped memory."""
import ctypes as C
import math

import numpy as np

ASYNC, SYNC = "asynchronous", "host-synchronous"

# One row per entry point that takes a `stream` ("The stream contract": the same rows, checked by
# tests/test_stream_contract_cpu.py).  ASYNC: with device pointers the call returns without waiting for the stream.  SYNC: the
# call waits on the host whatever the pointers are; the reason stands in DESIGN.md.
CONTRACT = {
    "tsdgpu_memcpy": ASYNC, "tsdgpu_memset": ASYNC, "tsdgpu_zero_imag": ASYNC, "tsdgpu_synchronize": SYNC,
    "tsdgpu_vec_op": ASYNC, "tsdgpu_vec_reduce": SYNC,
    "tsdgpu_fir_step": ASYNC, "tsdgpu_fir_step_after": ASYNC, "tsdgpu_fir_reset_on": ASYNC,
    "tsdgpu_fir_get_history": ASYNC, "tsdgpu_fir_set_history": ASYNC,
    "tsdgpu_fft_step": ASYNC, "tsdgpu_rfft_step": ASYNC, "tsdgpu_fftshift": ASYNC,
    "tsdgpu_ola_step": ASYNC, "tsdgpu_ola_analyse": ASYNC, "tsdgpu_ola_synthese": ASYNC, "tsdgpu_ola_apply_response": ASYNC,
    "tsdgpu_ola_read_spectra": SYNC, "tsdgpu_ola_write_spectra": SYNC,
    "tsdgpu_welch": SYNC,
    "tsdgpu_sos_step": ASYNC, "tsdgpu_sos_step_skip": ASYNC, "tsdgpu_sos_reset_on": ASYNC,
    "tsdgpu_sos_get_state": SYNC, "tsdgpu_sos_set_state": SYNC,
    "tsdgpu_fir_bank_step": ASYNC, "tsdgpu_fir_bank_get_history": ASYNC, "tsdgpu_fir_bank_set_history": ASYNC,
    "tsdgpu_sos_bank_step": ASYNC, "tsdgpu_sos_bank_get_state": SYNC, "tsdgpu_sos_bank_set_state": SYNC,
    "tsdgpu_polyfir_bank_step": ASYNC, "tsdgpu_polyfir_bank_get_state": ASYNC, "tsdgpu_polyfir_bank_set_state": ASYNC,
    "tsdgpu_channelizer_step": ASYNC, "tsdgpu_channelizer_get_state": ASYNC, "tsdgpu_channelizer_set_state": ASYNC,
    "tsdgpu_synthesizer_step": ASYNC, "tsdgpu_synthesizer_get_state": ASYNC, "tsdgpu_synthesizer_set_state": ASYNC,
    "tsdgpu_resampler_step": ASYNC, "tsdgpu_resampler_seek": ASYNC,
    "tsdgpu_polyfir_step": ASYNC, "tsdgpu_rii_step": ASYNC,
    "tsdgpu_detector_step": SYNC, "tsdgpu_xcorr": SYNC, "tsdgpu_delay_estimate": SYNC,
    "tsdgpu_spectrum_step": ASYNC, "tsdgpu_spectrum_reset": ASYNC,
}

POISON_X, POISON_Y = 0x7FC0_0A11, 0x7FC0_0B22      # two quiet NaNs of different payloads
STEPS = (4099, 1, 20000)                           # ~22 overlap-save blocks of 896, the SOS 8192-chunk layout, 16-frame units
TARGET_MS, MIN_MS = 50.0, 20.0


def bits(a):
    """the uint32 image of a float32 / complex64 / float64 array (NaN-safe exact comparison)"""
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ the delay
class Delay:
    """A device-side delay of about TARGET_MS on the current stream: torch.cuda._sleep, or, where that does not delay on
    the device, a chain of large float32 matmuls.  Calibrated once with events."""

    def __init__(self):
        import torch
        self.kind, self.arg, self.ms = None, 0, 0.0
        self._a = None
        if hasattr(torch.cuda, "_sleep"):
            ms = self._time(lambda: torch.cuda._sleep(20_000_000))
            if ms >= 1.0:
                self.kind, self.arg = "torch.cuda._sleep", int(20_000_000 * TARGET_MS / ms)
        if self.kind is None:
            self._a = torch.randn(4096, 4096, device="cuda")
            self._b = torch.empty_like(self._a)
            self._chain(2)
            ms = self._time(lambda: self._chain(8)) / 8
            self.kind, self.arg = "matmul chain", max(1, int(math.ceil(TARGET_MS / max(ms, 1e-3))))
        self.ms = self._time(self)
        if self.ms < 0.9 * TARGET_MS:       # (the first figure includes the clock's ramp: one correction, then measured again)
            self.arg = max(1, int(self.arg * min(3.0, TARGET_MS / max(self.ms, 1e-3))))
            self.ms = self._time(self)
        torch.cuda.synchronize()

    def _chain(self, k):
        import torch
        for _ in range(k):
            torch.mm(self._a, self._a, out=self._b)

    @staticmethod
    def _time(fn):
        import torch
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def __call__(self):
        import torch
        if self.kind == "torch.cuda._sleep":
            torch.cuda._sleep(self.arg)
        else:
            self._chain(self.arg)


# ------------------------------------------------------------------------------------------------------ stream flags
def stream_flags(stream):
    """(flags, None) of a torch stream through hipStreamGetFlags of the HIP runtime ALREADY loaded in this process, or
    (None, why) when the symbol cannot be reached.  hipStreamNonBlocking is 0x1."""
    path = None
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    path = line.split()[-1]
                    break
    except OSError as e:
        return None, f"cannot list the loaded libraries: {e}"
    if path is None:
        return None, "no libamdhip64 among the loaded libraries"
    try:
        fn = C.CDLL(path).hipStreamGetFlags
    except (OSError, AttributeError) as e:
        return None, f"hipStreamGetFlags not reachable in {path}: {e}"
    fn.argtypes, fn.restype = [C.c_void_p, C.POINTER(C.c_uint)], C.c_int
    out = C.c_uint(0xFFFFFFFF)
    rc = fn(C.c_void_p(stream.cuda_stream), C.byref(out))
    if rc != 0:
        return None, f"hipStreamGetFlags returned {rc}"
    return int(out.value), None


# ------------------------------------------------------------------------------------------------------------- specs
class Op:
    """One operator configuration.
    make()                -> a fresh handle (None for the stateless entry points)
    xs                    the host inputs of the steps (numpy)
    call(h, x, y, cs)     the call under test: x, y device tensors (y None: the entry point returns to the host) and cs the raw
                          stream, or x a numpy array with y None, cs None (the host path).  Returns the valid view of y, or a
                          numpy array for what came back to the host.
    ycap(x)               (shape, numpy dtype) of the room the output of input x needs, None for host results
    entry                 the C entry point, the key of CONTRACT
    reset(h)              puts a handle back to its fresh state (host-synchronous is fine: it runs before the run under
                          test); None: the handle has no reset and the warm pass simply continues the stream on both sides
    inplace               y may be x
    layouts               the other layouts of scenario C the operator serves: offset1, strided, overlap (x and y the heads of
                          one buffer, for the operators whose output length differs from the input's)"""

    def __init__(self, name, make, xs, call, ycap, entry, reset=None, inplace=False, family=None, layouts=()):
        self.name, self.make, self.xs, self.call, self.ycap, self.entry = name, make, list(xs), call, ycap, entry
        self.reset, self.inplace, self.family = reset, inplace, family or name.split("-")[0]
        self.layouts = (("inplace",) if inplace else ()) + tuple(layouts)        # scenario C: the layouts that take private copies

    @property
    def expect_async(self):
        return self.entry is None or CONTRACT[self.entry] == ASYNC        # (entry None: the fakes of the harness's own tests)

    def __repr__(self):
        return self.name


def _torch_dtype(dt):
    import torch
    return {np.dtype(np.float32): torch.float32, np.dtype(np.complex64): torch.complex64}[np.dtype(dt)]


def alloc(shape, dtype, layout, poison):
    """a poisoned device tensor of the layout: plain | offset1 (one sample past a 16-B boundary) | strided (2-D: a row
    stride larger than n; 1-D: plain)"""
    import torch
    shape = tuple(int(s) for s in shape)
    tdt = _torch_dtype(dtype)
    pad = {"plain": 0, "inplace": 0, "offset1": 1, "strided": 5 if len(shape) == 2 else 0}[layout]
    base = torch.empty(shape[:-1] + (shape[-1] + pad,), dtype=tdt, device="cuda")
    flat = torch.view_as_real(base) if base.is_complex() else base
    flat.view(torch.int32).fill_(poison)
    if layout == "offset1":
        return base[..., 1:]
    if layout == "strided" and pad:
        return base[..., : shape[-1]]
    return base


class Run:
    """The tensors of one run (allocated and poisoned up front, alive until the object dies) and its actions."""

    def __init__(self, op, layout="plain", xs=None):
        import torch
        self.op, self.layout = op, layout
        self.xs = list(op.xs if xs is None else xs)
        self.x_src = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in self.xs]
        self.x_dev = [None if layout == "overlap" else alloc(x.shape, x.dtype, layout, POISON_X) for x in self.xs]
        self.y_dev, self.y_keep = [], []
        for i, x in enumerate(self.xs):
            cap = op.ycap(x)
            if layout == "overlap":
                # x and y are the heads of ONE buffer (y is x's address, their lengths differ): the footprints overlap
                assert tuple(cap[0][:-1]) == tuple(x.shape[:-1]) and np.dtype(cap[1]) == x.dtype
                base = alloc(tuple(x.shape[:-1]) + (max(x.shape[-1], cap[0][-1]),), x.dtype, "plain", POISON_Y)
                self.x_dev[i] = base[..., : x.shape[-1]]
                self.y_dev.append(base[..., : cap[0][-1]])
                self.y_keep.append(alloc(cap[0], cap[1], "plain", POISON_Y))
            elif cap is None:
                self.y_dev.append(None)
                self.y_keep.append(None)
            elif layout == "inplace":
                assert op.inplace and tuple(cap[0]) == tuple(x.shape) and np.dtype(cap[1]) == x.dtype
                self.y_dev.append(self.x_dev[i])
                self.y_keep.append(alloc(cap[0], cap[1], "plain", POISON_Y))
            else:
                self.y_dev.append(alloc(cap[0], cap[1], layout, POISON_Y))
                self.y_keep.append(alloc(cap[0], cap[1], "plain", POISON_Y))
        self.extra = []                     # whatever else must outlive the run (events, state buffers, returned views)
        self.gate = None
        self.pending = []                   # per call under test: was `gate` still pending when the call returned
        self.host = {}                      # step -> numpy result that came back to the host
        self.valid = {}                     # step -> shape of the valid view
        torch.cuda.synchronize()

    def head(self, st, delay):
        import torch
        with torch.cuda.stream(st):
            delay()
            if self.gate is None:
                self.gate = torch.cuda.Event()
                self.gate.record(st)

    def hand_over(self, a, b):
        import torch
        ev = torch.cuda.Event()
        ev.record(a)
        b.wait_event(ev)
        self.extra.append(ev)

    def note(self):
        self.pending.append(None if self.gate is None else (not self.gate.query()))

    def step(self, h, i, st, sync=False):
        import torch
        wait = torch.cuda.synchronize if sync else (lambda: None)
        with torch.cuda.stream(st):
            self.x_dev[i].copy_(self.x_src[i])
            wait()
            out = self.op.call(h, self.x_dev[i], self.y_dev[i], st.cuda_stream)
            self.note()
            wait()
            if isinstance(out, np.ndarray):
                self.host[i] = out
            else:
                self.valid[i] = tuple(out.shape)
                self.extra.append(out)
                self.y_keep[i].copy_(self.y_dev[i])
            wait()
            self.x_dev[i].fill_(float("nan"))
            wait()

    def results(self):
        """after the final synchronise: per step the uint32 image of the WHOLE kept buffer (the valid view and the poison
        around it), or of the host result"""
        import torch
        torch.cuda.synchronize()
        out = []
        for i in range(len(self.xs)):
            if i in self.host:
                out.append(bits(self.host[i]))
            elif i in self.valid:
                k = self.y_keep[i]
                out.append(np.concatenate([np.asarray(self.valid[i], np.uint32),
                                           bits((torch.view_as_real(k) if k.is_complex() else k).cpu().numpy())]))
            else:
                out.append(None)
        return out


def default_stream():
    import torch
    return torch.cuda.default_stream()


def warm(op, h, layout="plain"):
    """one synchronised pass of the same shapes and layout on the default stream, then back to the fresh state (or, without a reset,
    onward: the reference handle takes the same pass)"""
    import torch
    r = Run(op, layout)
    for i in range(len(r.xs)):
        r.step(h, i, default_stream(), sync=True)
    torch.cuda.synchronize()
    if op.reset is not None and h is not None:
        op.reset(h)
        torch.cuda.synchronize()


def reference(op, warmed, layout="plain", xs=None):
    """the reference run: a fresh handle, the default stream, a device synchronise after every action"""
    h = op.make()
    if warmed:
        warm(op, h, layout)
    r = Run(op, layout, xs)
    for i in range(len(r.xs)):
        r.step(h, i, default_stream(), sync=True)
    return r.results()


def under_test(op, streams, delay, warmed, layout="plain", xs=None):
    """the run under test: step i on streams[i], the delay in front of the first, an event between two streams -> (Run, bits)"""
    import torch
    h = op.make()
    if warmed:
        warm(op, h, layout)
    r = Run(op, layout, xs)
    torch.cuda.synchronize()
    r.head(streams[0], delay)
    for i in range(len(r.xs)):
        if i and streams[i] is not streams[i - 1]:
            r.hand_over(streams[i - 1], streams[i])
        r.step(h, i, streams[i])
    for s in set(streams):
        s.synchronize()
    got = r.results()
    r.handle = h
    return r, got


def report(label, delay, pending):
    print(f"[stream-order] {label}: delay {delay.ms:.1f} ms ({delay.kind}); gate pending after each call: {pending}")


def check(label, want, got, pending, delay, expect_async):
    """the two assertions of a case: the bits, then -- for calls the contract lists as asynchronous, on a warm handle --
    that `gate` was still pending when every call under test returned.  expect_async None: bits only."""
    report(label, delay, pending)
    assert len(want) == len(got)
    for i, (w, g) in enumerate(zip(want, got)):
        assert (w is None) == (g is None), f"{label}: step {i} ran in one run only"
        if w is None:
            continue
        same = w.shape == g.shape and bool(np.array_equal(w, g))
        if not same:
            bad = int(np.count_nonzero(w != g)) if w.shape == g.shape else -1
            raise AssertionError(f"{label}: bits differ from the reference run at step {i} ({bad} of {w.size} words)")
    if expect_async:
        assert all(p is True for p in pending), \
            f"{label}: gate no longer pending when a call listed as asynchronous returned (host wait): {pending}"


# ------------------------------------------------------------------------------------------------- operators
def rand(n, cplx, seed):
    rng = np.random.default_rng(seed)
    if cplx:
        return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    return rng.standard_normal(n).astype(np.float32)


def rand2(C_, n, cplx, seed):
    return rand(C_ * n, cplx, seed).reshape(C_, n)


def lowpass(K, fc=0.1):
    k = np.arange(K) - (K - 1) / 2
    return (2 * fc * np.sinc(2 * fc * k) * np.hanning(K + 2)[1:-1]).astype(np.float32)


def _same(x):
    return x.shape, x.dtype


def _ragged(hop):
    return [int(math.ceil(n / hop)) * hop for n in STEPS]


def _step(h, x, y, cs):
    return h.step(x) if isinstance(x, np.ndarray) else h.step(x, y, stream=cs)


def _fft_step(h, x, y, cs):
    return h.step(x) if isinstance(x, np.ndarray) else h.step(x, True, y, stream=cs)


def _dt(t, cplx):
    return t.C64 if cplx else t.F32


def _lib():
    import libtsd_amd.capi as capi
    return capi


def polyfir_call(h, x, y, cs):
    """PolyFir.step into a caller's buffer (the wrapper allocates its own)"""
    if isinstance(x, np.ndarray):
        return h.step(x)
    capi = _lib()
    got = C.c_int64(0)
    capi._check(capi.lib().tsdgpu_polyfir_step(h._h, capi._ptr(x), int(x.shape[0]), capi._ptr(y), int(y.shape[0]), C.byref(got), cs))
    return y[: got.value]


def fftshift_call(h, x, y, cs):
    capi = _lib()
    if isinstance(x, np.ndarray):
        return capi.fftshift(x)
    capi._check(capi.lib().tsdgpu_fftshift(capi._ptr(x), capi._ptr(y), int(x.shape[0]), capi._dtype_code(x), cs))
    return y


def ola_bracket_call(h, x, y, cs):
    """analyse + synthese with nothing edited in between (no response: the identity engine), into a caller's buffer"""
    capi = _lib()
    if isinstance(x, np.ndarray):
        h.analyse(x)
        return h.synthese()
    h.analyse(x, stream=cs)
    got = C.c_int64(0)
    capi._check(capi.lib().tsdgpu_ola_synthese(h._h, capi._ptr(y), C.byref(got), cs))
    return y[: got.value]


def sos_coefs(order, wn):
    from scipy.signal import butter
    sos = butter(order, wn, output="sos")
    return np.array([[s[0], s[1], s[2], s[4], s[5]] for s in sos], np.float32)


def operators(t):
    """every configuration the module runs (scenarios A and B for each)"""
    ops = []
    add = ops.append
    rst = lambda h: h.reset()

    # ---- Fir: direct K = 31, the 1024-point overlap-save plan K = 127, ols_long K = 600, partitioned K = 12290
    for K, method, tag in ((31, t.FIR_DIRECT, "direct31"), (127, t.FIR_OVERLAP_SAVE, "ols127"), (600, t.FIR_OVERLAP_SAVE, "olslong600"),
                           (12290, t.FIR_AUTO, "part12290")):
        for cplx in (False, True):
            taps = lowpass(K, 0.05)
            add(Op(f"fir-{tag}-{'c64' if cplx else 'f32'}", (lambda taps=taps, cplx=cplx, method=method: t.Fir(taps, _dt(t, cplx), method)),
                   [rand(n, cplx, 10 + n) for n in STEPS], _step, _same, "tsdgpu_fir_step", rst, inplace=True))
    ctaps = (lowpass(31, 0.05) * np.exp(0.3j * np.arange(31))).astype(np.complex64)
    add(Op("fir-direct31-c64-ctaps", lambda: t.Fir(ctaps, t.C64, t.FIR_DIRECT), [rand(n, True, 20 + n) for n in STEPS], _step, _same,
           "tsdgpu_fir_step", rst, inplace=True))
    # step_after: the delay line taken from the head of x itself
    for K, method, tag in ((31, t.FIR_DIRECT, "direct31"), (127, t.FIR_OVERLAP_SAVE, "ols127")):
        taps = lowpass(K, 0.05)

        def after(h, x, y, cs):
            if isinstance(x, np.ndarray):
                raise NotImplementedError("step_after takes device buffers")
            h.step_after(x, y, h.lead, stream=cs)
            return y
        add(Op(f"fir-after-{tag}", (lambda taps=taps, method=method: t.Fir(taps, t.C64, method)), [rand(n, True, 30 + n) for n in (4099, 20000)],
               after, _same, "tsdgpu_fir_step_after", rst, family="fir_after"))

    # ---- Sos: the 12th-order cascade at fc 0.25; a long-memory smoother whose 20000-sample step takes the exact carry
    for tag, co in (("butter12", sos_coefs(12, 0.5)), ("longmem", sos_coefs(2, 2e-4))):
        for cplx in (False, True):
            add(Op(f"sos-{tag}-{'c64' if cplx else 'f32'}", (lambda co=co, cplx=cplx: t.Sos(co, 1.0, _dt(t, cplx))),
                   [rand(n, cplx, 40 + n) + np.float32(0.5) for n in STEPS], _step, _same, "tsdgpu_sos_step", rst, inplace=True))

    def skip_call(h, x, y, cs):
        if isinstance(x, np.ndarray):
            raise NotImplementedError("step_skip takes device buffers")
        return h.step_skip(x, y, 8, stream=cs)              # (y[:8] keeps its poison in both runs)
    add(Op("sos-skip-butter12-c64", lambda: t.Sos(sos_coefs(12, 0.5), 1.0, t.C64), [rand(n, True, 45 + n) for n in (4099, 8, 20000)], skip_call, _same,
           "tsdgpu_sos_step_skip", rst, family="sos_skip"))

    # ---- Rii: FIR kernel + block-parallel sections (path 1), the literal recursion (path 2), first-order complex sections (path 3)
    de1 = np.real(np.poly([0.8 * np.exp(0.5j), 0.8 * np.exp(-0.5j), 0.6, -0.3])).astype(np.float32)
    nu1 = np.array([1.0, 0.4, 0.2, 0.1, 0.05], np.float32)
    add(Op("rii-sections", lambda: t.Rii(nu1, de1, t.F32), [rand(n, False, 50 + n) for n in STEPS], _step, _same, "tsdgpu_rii_step", None, inplace=True))
    de2 = np.poly([1.0005, 0.5, -0.3]).astype(np.float32)
    add(Op("rii-literal", lambda: t.Rii([1.0, 0.2, 0.1, 0.3], de2, t.F32), [rand(n, False, 60 + n) for n in (515, 1, 2000)], _step, _same,
           "tsdgpu_rii_step", None, inplace=True))
    de3 = (np.poly(np.array([0.6 * np.exp(0.7j), 0.5 * np.exp(2.1j), 0.3 + 0j])) * (1.5 - 0.5j)).astype(np.complex64)
    nu3 = np.array([0.3 + 0.1j, -0.2j, 0.5, 0.1 - 0.4j], np.complex64)
    add(Op("rii-complex", lambda: t.Rii(nu3, de3, t.C64), [rand(n, True, 70 + n) for n in STEPS], _step, _same, "tsdgpu_rii_step", None, inplace=True))

    # ---- the banks
    Cb = 3
    for K, method, tag in ((31, t.FIR_DIRECT, "direct31"), (127, t.FIR_OVERLAP_SAVE, "ols127")):
        for cplx in (False, True):
            taps = lowpass(K, 0.05)
            add(Op(f"firbank-{tag}-{'c64' if cplx else 'f32'}", (lambda taps=taps, cplx=cplx, method=method: t.FirBank(taps, _dt(t, cplx), Cb, method)),
                   [rand2(Cb, n, cplx, 80 + n) for n in STEPS], _step, _same, "tsdgpu_fir_bank_step", rst, inplace=True))
    co12 = sos_coefs(12, 0.5)
    for cplx in (False, True):
        add(Op(f"sosbank-butter12-{'c64' if cplx else 'f32'}", (lambda cplx=cplx: t.SosBank(co12, 1.0, _dt(t, cplx), Cb)),
               [rand2(Cb, n, cplx, 90 + n) for n in STEPS], _step, _same, "tsdgpu_sos_bank_step", rst, inplace=True))

    # ---- PolyFir / PolyFirBank: decimator, half-band, upsampler
    kinds = (("decim", t.POLY_DECIM, lowpass(24, 0.12), 3, lambda n: n // 3 + 1),
             ("decim48", t.POLY_DECIM, lowpass(48, 0.06), 5, lambda n: n // 5 + 1),
             ("halfband", t.POLY_HALFBAND, lowpass(15, 0.25), 2, lambda n: n // 2 + 1),
             ("ups", t.POLY_UPS, lowpass(24, 0.12), 3, lambda n: n * 3))
    for tag, kind, taps, R, cap in kinds:
        for cplx in (False, True):
            sfx = "c64" if cplx else "f32"
            add(Op(f"polyfir-{tag}-{sfx}", (lambda kind=kind, taps=taps, R=R, cplx=cplx: t.PolyFir(kind, _dt(t, cplx), taps, R)),
                   [rand(n, cplx, 100 + n) for n in STEPS], polyfir_call, (lambda x, cap=cap: ((cap(x.shape[0]),), x.dtype)),
                   "tsdgpu_polyfir_step", rst))
            add(Op(f"polyfirbank-{tag}-{sfx}", (lambda kind=kind, taps=taps, R=R, cplx=cplx: t.PolyFirBank(kind, _dt(t, cplx), Cb, taps, R)),
                   [rand2(Cb, n, cplx, 110 + n) for n in STEPS], _step, (lambda x, cap=cap: ((Cb, cap(x.shape[1])), x.dtype)),
                   "tsdgpu_polyfir_bank_step", rst))

    # ---- Resampler: K = 15 fused, K = 31 generic, K = 127 long, one analytic interpolator
    def luts(K, ratio):
        return dict(K=K, lut=t.itrp_sinc_lut(K, 256, float(min(np.float32(0.4), np.float32(ratio) / np.float32(2)))))
    for tag, kw, ratio in (("k15", luts(15, 1.3), 1.3), ("k31", luts(31, 0.77), 0.77), ("k127", luts(127, 1.1), 1.1),
                           ("lagrange3", dict(analytic=("lagrange", 3)), 1.3)):
        for cplx in (False, True):
            add(Op(f"resampler-{tag}-{'c64' if cplx else 'f32'}", (lambda kw=kw, ratio=ratio, cplx=cplx: t.Resampler(ratio, _dt(t, cplx), **kw)),
                   [rand(n, cplx, 120 + n) for n in STEPS], _step, (lambda x, ratio=ratio: ((int(x.shape[0] * ratio) + 4,), x.dtype)),
                   "tsdgpu_resampler_step", rst))

    # ---- Fft / Rfft (stateless plans: the three "steps" are three batches), fftshift, vec_op
    for n, batches in ((1 << 15, (1, 2, 3)), (3 << 10, (3, 1, 8)), (1000, (5, 1, 20)), (1001, (5, 1, 20)), (64, (65, 1, 300))):
        add(Op(f"fft-{n}", (lambda n=n: t.Fft(n)), [rand2(b, n, True, 130 + b) for b in batches], _fft_step, _same, "tsdgpu_fft_step", None, inplace=True))
    for n, batches in ((4096, (2, 1, 5)), (1000, (5, 1, 20)), (1001, (5, 1, 20))):
        add(Op(f"rfft-{n}", (lambda n=n: t.Rfft(n)), [rand2(b, n, False, 140 + b) for b in batches], _step,
               (lambda x: (x.shape, np.complex64)), "tsdgpu_rfft_step", None))
    for cplx in (False, True):
        add(Op(f"fftshift-{'c64' if cplx else 'f32'}", lambda: None, [rand(n, cplx, 150 + n) for n in STEPS], fftshift_call, _same, "tsdgpu_fftshift", None))
    for opname, two in (("reverse", False), ("scale", False), ("mul", True), ("abs2", False), ("conj", False)):
        def vcall(h, x, y, cs, opname=opname, two=two):
            if isinstance(x, np.ndarray):
                raise NotImplementedError("vec_op takes resident vectors")
            return t.vec_op(opname, x, x if two else None, 1.5 - 0.5j, out=y)
        add(Op(f"vec_op-{opname}", lambda: None, [rand(n, True, 160 + n) for n in STEPS], vcall,
               (lambda x, opname=opname: (x.shape, np.float32 if opname == "abs2" else x.dtype)), "tsdgpu_vec_op", None, family="vec_op",
               inplace=opname in ("scale", "mul", "conj")))          # (dst may be a or b except for reverse)

    # ---- Ola: step with a response (fast path Ne = 896 / N = 1024 and a general geometry), windowed, analyse + synthese
    def ola_make(Ne, zeros, windowed, response):
        def mk():
            h = t.Ola(Ne, zeros, np.hanning(Ne + 1)[:-1].astype(np.float32) if windowed else None)
            if response:
                h.set_response(np.fft.fft(np.concatenate([lowpass(zeros + 1, 0.1), np.zeros(h.N - zeros - 1)])).astype(np.complex64))
            return h
        return mk
    ocap = lambda Ne: (lambda x: ((x.shape[0] + Ne,), x.dtype))
    ola_x = [rand(n, True, 170 + n) for n in STEPS]
    add(Op("ola-step-896", ola_make(896, 128, False, True), ola_x, _step, ocap(896), "tsdgpu_ola_step", None))
    add(Op("ola-step-500", ola_make(500, 12, False, True), ola_x, _step, ocap(500), "tsdgpu_ola_step", None))
    add(Op("ola-step-windowed512", ola_make(512, 0, True, True), ola_x, _step, ocap(512), "tsdgpu_ola_step", None))
    add(Op("ola-bracket-500", ola_make(500, 12, False, False), ola_x, ola_bracket_call, ocap(500), "tsdgpu_ola_synthese", None, family="ola_bracket"))
    add(Op("ola-bracket-windowed512", ola_make(512, 0, True, False), ola_x, ola_bracket_call, ocap(512), "tsdgpu_ola_synthese", None, family="ola_bracket"))

    # ---- Spectrum: blocks of BS = 2 x 256, a spectrum every 3 blocks, plain and sweep
    BS = 512
    w = np.hanning(256).astype(np.float32)
    w = (w * np.sqrt(256 / np.sum(w.astype(np.float64) ** 2))).astype(np.float32)
    sp_x = [rand(b * BS, True, 180 + b) for b in (8, 1, 39)]
    for tag, sweep, Ns in (("plain", None, 256), ("sweep", (64, None), 320)):
        add(Op(f"spectrum-{tag}", (lambda sweep=sweep: t.Spectrum(BS, 2, 3, w, sweep)), sp_x, _step,
               (lambda x, Ns=Ns: ((x.shape[0] // BS // 3 + 1, Ns), np.float32)), "tsdgpu_spectrum_step", rst))

    # ---- the polyphase analysis / synthesis banks
    for M in (16, 64):
        h4 = lowpass(4 * M, 0.5 / M)
        for OS in (1, 2):
            hop = M // OS
            ns = _ragged(hop)
            add(Op(f"channelizer-M{M}-os{OS}", (lambda M=M, OS=OS, h4=h4: t.Channelizer(h4, M, OS)), [rand(n, True, 190 + n) for n in ns], _step,
                   (lambda x, M=M, hop=hop: ((M, x.shape[0] // hop), np.complex64)), "tsdgpu_channelizer_step", rst))
            add(Op(f"synthesizer-M{M}-os{OS}", (lambda M=M, OS=OS, h4=h4: t.Synthesizer(h4, M, OS)), [rand2(M, n // hop, True, 200 + n) for n in ns], _step,
                   (lambda u, hop=hop: ((u.shape[1] * hop,), np.complex64)), "tsdgpu_synthesizer_step", rst))
            add(Op(f"rchannelizer-M{M}-os{OS}", (lambda M=M, OS=OS, h4=h4: t.RealChannelizer.oversampled(h4, M, OS) if OS > 1 else t.RealChannelizer(h4, M)),
                   [rand(n, False, 210 + n) for n in ns], _step, (lambda x, M=M, hop=hop: ((M // 2 + 1, x.shape[0] // hop), np.complex64)),
                   "tsdgpu_channelizer_step", rst))
        nsM = _ragged(M)
        add(Op(f"rsynthesizer-M{M}", (lambda M=M, h4=h4: t.RealSynthesizer(h4, M)), [rand2(M // 2 + 1, n // M, True, 220 + n) for n in nsM], _step,
               (lambda u, M=M: ((u.shape[1] * M,), np.float32)), "tsdgpu_synthesizer_step", rst))

    # ---- what returns to the host: ordering only
    def welch_call(h, x, y, cs):
        S, nseg = t.welch(x, 256, w)
        return np.concatenate([S, np.array([nseg], np.float32)])

    def xcorr_call(h, x, y, cs):
        r = t.xcorr(x, None, 64, True)
        return r if isinstance(r, np.ndarray) else r.cpu().numpy()

    def delay_call(h, x, y, cs):
        n = x.shape[0] // 2
        return np.array(t.delay_estimate(x[:n], x[n: 2 * n]), np.float32)

    def reduce_call(h, x, y, cs):
        if isinstance(x, np.ndarray):
            raise NotImplementedError("vec_reduce takes resident vectors")
        s, mx, mn, im = t.vec_reduce(x)
        return np.array([s.real, s.imag, mx, mn, im], np.float64)

    def detector_call(h, x, y, cs):
        sc, pk = h.step(x)
        sc = sc if isinstance(sc, np.ndarray) else sc.cpu().numpy()
        return np.concatenate([sc, np.array([p.index for p in pk] + [len(pk)], np.float32)])

    none = lambda x: None
    host_x = [rand(n, True, 230 + n) for n in (4099, 20000)]
    add(Op("welch", lambda: None, host_x, welch_call, none, "tsdgpu_welch", None))
    add(Op("xcorr", lambda: None, host_x, xcorr_call, none, "tsdgpu_xcorr", None))
    dly = rand(4096, True, 7)
    add(Op("delay_estimate", lambda: None, [np.concatenate([dly, np.roll(dly, 5)]), np.concatenate([dly[:1000], np.roll(dly[:1000], 3)])], delay_call, none,
           "tsdgpu_delay_estimate", None))
    add(Op("vec_reduce", lambda: None, [rand(n, False, 240 + n) for n in STEPS], reduce_call, none, "tsdgpu_vec_reduce", None))
    pat = rand(200, True, 9)
    det_x = []
    for b in range(3):
        xb = (0.01 * rand(1024, True, 250 + b)).astype(np.complex64)
        xb[300 + 100 * b: 500 + 100 * b] += pat
        det_x.append(xb)
    for mode in (0, 1):
        add(Op(f"detector-mode{mode}", (lambda mode=mode: t.Detector(pat, 1024, mode, threshold=0.8)), det_x, detector_call, none, "tsdgpu_detector_step", None))
    names = [o.name for o in ops]
    assert len(set(names)) == len(names)
    for o in ops:
        o.layouts += EXTRA_LAYOUTS.get(o.family, ())
    return ops


# scenario C beyond y is x: a view one sample past a 16-byte boundary (packed staging, the narrow paths) and, for the 2-D
# blocks of the banks, a row stride larger than n
EXTRA_LAYOUTS = {
    "fir": ("offset1",), "fir_after": ("offset1",), "sos": ("offset1",), "sos_skip": ("offset1",), "rii": ("offset1",), "fftshift": ("offset1",), "vec_op": ("offset1",),
    "firbank": ("offset1", "strided"), "sosbank": ("offset1", "strided"), "polyfirbank": ("offset1", "strided", "overlap"),
    "ola": ("overlap",),
    "channelizer": ("offset1", "strided"), "rchannelizer": ("offset1", "strided"), "synthesizer": ("offset1", "strided"),
    "rsynthesizer": ("offset1", "strided"),
}
