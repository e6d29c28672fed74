"""GPU: what every call of a stream must RETURN.  The other stream tests compare surfaces with each other and with the
one-shot result; here a model in Python integers says, call by call, how many frames are due — a brute-force count of the
outputs k with floor(k M / L) + T/2 <= N - 1 from the plan's L / M / taps, the plan's out_len at the flush — and the C
entries (soxr_amd._native, explicit olen) must return min(due, olen) (a deferred stream: what was due one call earlier),
delay() must equal n_in L / M - handed_out exactly, and the concatenated output must be the one-shot result bit for bit.

One script, 48000 -> 32000 "LQ" (small L, M and tap count), on every surface that takes it:
  a  chunks of 1, 0, 7 and 441 frames        host ring; empty calls; a call too short to emit
  b  twenty chunks of 441 with olen = 100     a backlog drained by olen
  c  one chunk above 64 KiB                   the host ring moves to device memory (20000 float32 frames; int16: 40000)
  d  chunks of 4410 past the ring's capacity twice    device compaction
  e  an empty call, then the flush with olen = 64 until it returns 0
The tail of this conversion is 21 frames (64 taps), so after e's empty call has drained the backlog the flush hands it out
in ONE piece of olen = 64 (a deferred stream's backlog does come out in pieces of 64); one more host case flushes with
olen = 8, where the tail comes in three pieces.
Counts are integers and results are bits: no tolerances."""
import ctypes as C

import numpy as np
import pytest

from vr_sim import VrSim

pytestmark = pytest.mark.gpu

IN_RATE, OUT_RATE, QUALITY = 48000, 32000, "LQ"
BIG = 32768  # an olen that never caps a call of the script (the most due at once: step c's chunk plus b's backlog, < 31000)


def _sig(rng, shape, dtype):
    if np.issubdtype(dtype, np.integer):
        return (rng.standard_normal(shape) * 5000).astype(dtype)
    return (rng.standard_normal(shape) * 0.25).astype(dtype)


def _steps(dtype, which):
    """[(ilen or None for end of input, olen)] of the script's steps `which`; the flush is added by the driver loop."""
    c_frames = 20000 if np.dtype(dtype).itemsize >= 4 else 40000  # above 64 KiB of mono samples
    # d: the ring's capacity is a power of two times 1024 that holds what is kept plus four chunks (sixteen small ones or
    # 64 Ki frames of device chunks) — below 2 * (4 * c_frames + 8192) on every path here; twice that in 4410-frame chunks
    d_calls = 2 * (2 * (4 * c_frames + 8192) // 4410 + 1)
    steps = {"a": [(1, BIG), (0, BIG), (7, BIG), (441, BIG)], "b": [(441, 100)] * 20, "c": [(c_frames, BIG)],
             "d": [(4410, BIG)] * d_calls, "e": [(0, BIG)]}
    return [s for w in which for s in steps[w]]


class Model:
    """The schedule of a constant-rate stream in integers."""

    def __init__(self, n, h):
        info = n.PlanInfo()
        self.plan = n.lib.hipsoxr_stream_plan(h)
        n.check(n.lib.hipsoxr_plan_info(self.plan, C.byref(info)))
        assert not info.interpolated
        self.n, self.L, self.M, self.T = n, int(info.L), int(info.M), int(info.taps)
        self.n_in = self.k_avail = self.k_done = self.handed = self.pend = 0
        self.ended = False

    def _avail(self):  # brute force, resumed where the last call left it: the condition is monotonic in k and in N
        while (self.k_avail * self.M) // self.L + self.T // 2 <= self.n_in - 1:
            self.k_avail += 1
        return self.k_avail

    def _k_end(self):
        return int(self.n.lib.hipsoxr_plan_out_len(self.plan, self.n_in)) if self.ended else self._avail()

    def call(self, ilen, olen):
        """Synchronous surfaces: everything due, as far as olen reaches."""
        if ilen is None:
            self.ended = True
        else:
            self.n_in += ilen
        got = min(max(self._k_end() - self.k_done, 0), olen)
        self.k_done += got
        self.handed += got
        return got

    def call_deferred(self, ilen, olen):
        """DEFER: the call hands out what the previous call launched; it launches (everything due) once that is handed out.
        End of input: the pending result, then — in the same call — the tail."""
        got = min(self.pend, olen)
        self.pend -= got
        if ilen is None:
            if self.pend == 0 and got < olen:
                self.ended = True
                tail = min(max(self._k_end() - self.k_done, 0), olen - got)
                self.k_done += tail
                got += tail
        else:
            self.n_in += ilen
            if self.pend == 0:
                self.pend = max(self._avail() - self.k_done, 0)
                self.k_done += self.pend
        self.handed += got
        return got

    def delay(self):
        return max(self.n_in * self.L / self.M - self.handed, 0.0)


class HostStream:
    """hipsoxr_stream_process on numpy memory; split=True: one plane per channel on both sides."""

    def __init__(self, n, dtype, ch=1, split=False, flags=0, total_out=0):
        self.n, self.ch, self.split, self.dtype = n, ch, split, np.dtype(dtype)
        self.h = C.c_void_p()
        elem = {np.dtype(np.float32): n.FLOAT32_I, np.dtype(np.int16): n.INT16_I}[self.dtype] | (4 if split else 0)
        n.check(n.lib.hipsoxr_stream_create(float(IN_RATE), float(OUT_RATE), ch, elem, n.LQ, flags, C.byref(self.h)))
        self.out = np.zeros((ch, total_out) if split else (total_out, ch), self.dtype)
        self.pos = 0
        self.done = C.c_size_t(0)

    def close(self):
        self.n.lib.hipsoxr_stream_delete(self.h)

    def process(self, x, olen):
        """x: [frames, ch] or None (end of input) -> frames returned; they land in self.out behind the earlier ones."""
        es = self.dtype.itemsize
        assert self.pos + olen <= (self.out.shape[1] if self.split else self.out.shape[0])
        if self.split:
            planes = None if x is None else np.ascontiguousarray(x.T)
            ins = None if x is None else (C.c_void_p * self.ch)(*[planes.ctypes.data + c * planes.shape[1] * es for c in range(self.ch)])
            outs = (C.c_void_p * self.ch)(*[self.out.ctypes.data + (c * self.out.shape[1] + self.pos) * es for c in range(self.ch)])
            in_ptr, out_ptr, n_in = (None if x is None else C.cast(ins, C.c_void_p)), C.cast(outs, C.c_void_p), (0 if x is None else x.shape[0])
        else:
            xc = None if x is None else np.ascontiguousarray(x)
            in_ptr = None if x is None else (xc.ctypes.data if len(xc) else self.out.ctypes.data)  # (an empty call is not the end of input)
            out_ptr, n_in = self.out.ctypes.data + self.pos * self.ch * es, (0 if x is None else len(xc))
        self.n.check(self.n.lib.hipsoxr_stream_process(self.h, in_ptr, n_in, out_ptr, olen, C.byref(self.done)))
        self.pos += self.done.value
        return self.done.value

    def delay(self):
        return float(self.n.lib.hipsoxr_stream_delay(self.h))

    def result(self):
        return self.out.T[:self.pos] if self.split else self.out[:self.pos]


class DeviceStream:
    """hipsoxr_stream_process_device on torch memory (mono), on the current torch stream."""

    def __init__(self, n, dtype, total_out, flags=0):
        import torch
        self.n, self.torch = n, torch
        self.h = C.c_void_p()
        tdtype = {np.dtype(np.float32): torch.float32, np.dtype(np.int16): torch.int16}[np.dtype(dtype)]
        elem = {torch.float32: n.FLOAT32_I, torch.int16: n.INT16_I}[tdtype]
        n.check(n.lib.hipsoxr_stream_create(float(IN_RATE), float(OUT_RATE), 1, elem, n.LQ, flags, C.byref(self.h)))
        self.out = torch.zeros(total_out, dtype=tdtype, device="cuda")
        self.es, self.pos, self.done, self.keep = self.out.element_size(), 0, C.c_size_t(0), []

    def close(self):
        self.torch.cuda.synchronize()
        self.n.lib.hipsoxr_stream_delete(self.h)

    def process(self, x, olen):
        assert self.pos + olen <= self.out.shape[0]
        out_ptr = self.out.data_ptr() + self.pos * self.es
        in_ptr, n_in = None, 0
        if x is not None:
            xd = self.torch.from_numpy(np.ascontiguousarray(x[:, 0])).cuda()
            self.keep.append(xd)  # (the call is asynchronous: the chunk lives until the stream has read it)
            in_ptr, n_in = (xd.data_ptr() if len(xd) else out_ptr), len(xd)
        stream = self.torch.cuda.current_stream().cuda_stream
        self.n.check(self.n.lib.hipsoxr_stream_process_device(self.h, in_ptr, n_in, out_ptr, olen, C.byref(self.done), stream))
        self.pos += self.done.value
        return self.done.value

    def delay(self):
        return float(self.n.lib.hipsoxr_stream_delay(self.h))

    def result(self):
        self.torch.cuda.synchronize()
        return self.out[:self.pos].cpu().numpy()[:, None]


def _run_script(soxr, stream, model_call, model, x, steps, flush_olen=64):
    """Drive `stream` through `steps` and the flush; every call against the model; the whole against the one-shot result."""
    at = 0
    for i, (ilen, olen) in enumerate(steps):
        got = stream.process(x[at:at + ilen], olen)
        at += ilen
        assert got == model_call(ilen, olen), f"call {i}: {ilen} frames in, olen {olen}"
        assert stream.delay() == model.delay(), f"delay after call {i}"
    assert at == len(x)
    pieces = 0
    for i in range(len(x)):  # the flush, flush_olen frames at a time, until the stream is dry
        got = stream.process(None, flush_olen)
        assert got == model_call(None, flush_olen), f"flush call {i}"
        assert stream.delay() == model.delay(), f"delay after flush call {i}"
        if got == 0:
            break
        pieces += 1
    want = soxr.resample(x if x.shape[1] > 1 else x[:, 0], IN_RATE, OUT_RATE, quality=QUALITY)
    got = stream.result()
    assert np.array_equal(got if x.shape[1] > 1 else got[:, 0], want)
    return pieces


def _total(steps):
    return sum(s[0] for s in steps)


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_host_stream_returns_what_is_due(soxr, dtype):
    from soxr_amd import _native as n
    steps = _steps(dtype, "abcde")
    x = _sig(np.random.default_rng(31), (_total(steps), 1), dtype)
    s = HostStream(n, dtype, total_out=len(x) + BIG)
    try:
        m = Model(n, s.h)
        _run_script(soxr, s, m.call, m, x, steps)
    finally:
        s.close()


def test_host_stream_hands_out_the_tail_in_pieces(soxr):
    """Steps a and e with a flush of olen = 8, below the tail's 21 frames: three pieces, then 0."""
    from soxr_amd import _native as n
    steps = _steps(np.float32, "ae")
    x = _sig(np.random.default_rng(37), (_total(steps), 1), np.float32)
    s = HostStream(n, np.float32, total_out=len(x) + BIG)
    try:
        m = Model(n, s.h)
        assert _run_script(soxr, s, m.call, m, x, steps, flush_olen=8) == 3
    finally:
        s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_deferred_stream_returns_what_was_due_one_call_earlier(soxr, dtype):
    from soxr_amd import _native as n
    steps = _steps(dtype, "abe")
    x = _sig(np.random.default_rng(32), (_total(steps), 1), dtype)
    s = HostStream(n, dtype, flags=n.DEFER, total_out=len(x) + BIG)
    try:
        m = Model(n, s.h)
        _run_script(soxr, s, m.call_deferred, m, x, steps)
        assert m.pend == 0 and m.handed == m.k_done
    finally:
        s.close()


@pytest.mark.parametrize("first", ["small", "large"])
def test_split_stream_returns_what_is_due(soxr, first):
    """Two planes per side.  A small first chunk puts the stream behind the interleaving adapter, a large one on the planar
    device ring: the calls return the same counts either way."""
    from soxr_amd import _native as n
    steps = _steps(np.float32, "abcde" if first == "small" else "cabde")
    x = _sig(np.random.default_rng(33), (_total(steps), 2), np.float32)
    s = HostStream(n, np.float32, ch=2, split=True, total_out=len(x) + BIG)
    try:
        m = Model(n, s.h)
        _run_script(soxr, s, m.call, m, x, steps)
    finally:
        s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_device_chunks_return_what_is_due(soxr, dtype):
    from soxr_amd import _native as n
    steps = _steps(dtype, "ade")
    x = _sig(np.random.default_rng(34), (_total(steps), 1), dtype)
    s = DeviceStream(n, dtype, total_out=len(x) + BIG)
    try:
        m = Model(n, s.h)
        _run_script(soxr, s, m.call, m, x, steps)
    finally:
        s.close()


def test_grouped_device_chunks_return_what_is_due(soxr):
    """Three streams in one call (hipsoxr_streams_process_device): three calls of 441 frames in one launch, then a call with
    more than 4096 outputs due per stream, which the entry serves handle by handle — the same counts."""
    import torch
    from soxr_amd import _native as n
    calls = [441, 441, 441, 8000]
    x = _sig(np.random.default_rng(35), (3, sum(calls), 1), np.float32)
    streams = [DeviceStream(n, np.float32, total_out=sum(calls) + BIG) for _ in range(3)]
    try:
        models = [Model(n, s.h) for s in streams]
        handles = (C.c_void_p * 3)(*[s.h.value for s in streams])
        xd = torch.from_numpy(x[:, :, 0].copy()).cuda()
        at = 0
        for ilen in calls:
            ins = np.array([xd[i].data_ptr() + at * 4 for i in range(3)], np.uint64)
            outs = np.array([s.out.data_ptr() + s.pos * 4 for s in streams], np.uint64)
            ilens, olens, dones = np.full(3, ilen, np.uint64), np.full(3, BIG, np.uint64), np.zeros(3, np.uint64)
            n.check(n.lib.hipsoxr_streams_process_device(handles, 3, ins.ctypes.data, ilens.ctypes.data, outs.ctypes.data, olens.ctypes.data,
                                                         dones.ctypes.data, torch.cuda.current_stream().cuda_stream))
            at += ilen
            for s, m, d in zip(streams, models, dones):
                assert int(d) == m.call(ilen, BIG), f"{ilen}-frame call"
                s.pos += int(d)
                assert s.delay() == m.delay()
        assert models[0].handed > 4096
        for i, (s, m) in enumerate(zip(streams, models)):
            while True:
                got = s.process(None, 64)
                assert got == m.call(None, 64)
                assert s.delay() == m.delay()
                if got == 0:
                    break
            assert np.array_equal(s.result()[:, 0], soxr.resample(x[i, :, 0], IN_RATE, OUT_RATE, quality=QUALITY)), i
    finally:
        for s in streams:
            s.close()


def _vr_sim_call(sim, chunk, olen, last):
    """VrSim.feed with an olen: up to olen of the outputs due, one position law per stretch (a stretch ends with a slew)."""
    sim.x = np.concatenate([sim.x, np.asarray(chunk, np.float64)])
    k_end = min(sim._limit(last), sim.k_done + olen)
    outs = [np.zeros(0, np.float32)]
    while sim.k_done < k_end:
        slew_end = sim.k_s + sim.n_slew
        slewing = sim.n_slew and sim.k_done < slew_end
        stop = min(k_end, slew_end) if slewing else k_end
        v = sim.o.vr_run(sim.vp, sim.x, "port_" + sim.eng, stop - sim.k_done, sim.pos(sim.k_done), sim.step(sim.k_done), sim.delta if slewing else 0)
        outs.append(sim.o.quantize(v, sim.dtype, channel=0, k0=sim.k_done)[0])
        sim.k_done = stop
    return np.concatenate(outs)


def test_variable_rate_stream_returns_what_is_due(soxr, oracle):
    """The model is tests/vr_sim.py.  A set_io_ratio with a slew of 50 outputs is issued in the middle of a 441-frame call's
    worth of output (olen cuts that call short); the next call crosses the end of the slew and still returns everything due."""
    from soxr_amd import _native as n
    rng = np.random.default_rng(36)
    s = HostStream(n, np.float32, flags=n.VR, total_out=8 * 441 + BIG)
    try:
        sim = VrSim(oracle, IN_RATE, OUT_RATE, QUALITY, np.float32)
        empty = np.zeros((0, 1), np.float32)
        script = [(441, BIG, None), (441, BIG, None), (441, 147, (1.2, 50)), (0, BIG, None), (441, BIG, None), (441, BIG, (1.5, 1)),
                  (441, BIG, None), (441, BIG, None)]
        for i, (ilen, olen, change) in enumerate(script):
            x = _sig(rng, (ilen, 1), np.float32) if ilen else empty
            before = s.pos
            got = s.process(x, olen)
            want = _vr_sim_call(sim, x[:, 0], olen, False)
            assert got == len(want), f"call {i}"
            assert np.array_equal(s.out[before:s.pos, 0], want), f"call {i}"
            if i == 2:
                assert got == 147  # (cut short by olen: the change of ratio falls inside this call's worth of output)
            if i == 3:
                assert sim.n_slew and sim.k_done > sim.k_s + sim.n_slew and got > 50  # across the end of the slew, in one call
            if change:
                n.check(n.lib.hipsoxr_stream_set_io_ratio(s.h, change[0], change[1]))
                sim.set_io_ratio(*change)
        for i in range(100):
            before = s.pos
            got = s.process(None, 64)
            want = _vr_sim_call(sim, np.zeros(0), 64, True)
            assert got == len(want) and np.array_equal(s.out[before:s.pos, 0], want), f"flush call {i}"
            if got == 0:
                break
        assert s.pos > 2000
    finally:
        s.close()
