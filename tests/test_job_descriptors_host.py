"""The `hipsoxr_job_t` every Python entry builds, field by field (no GPU): the five C entries that take a job are replaced
by recorders, the stream query is faked as in tests/test_vr_ragged_host.py, and each of the eight places that hand a job to
the library — `Plan.run`, `run_adjoint`, `run_adjoint_ragged`, `run_vr_ragged`, `run_vr_ragged_adjoint`, `PreparedJob`,
`RaggedJob` and `_HostPipe._issue` — is driven at small fixed inputs.  Every field of the recorded job, the table rows behind
`clip_table` as they stand when the call is made, and the ratios array are compared with values stated from the inputs."""
import contextlib
import ctypes as C
import types

import numpy as np
import pytest

STREAM = 0x5EED           # what the faked torch.cuda.current_stream answers
ENTRIES = {"hipsoxr_run_device": False, "hipsoxr_run_device_adjoint": False, "hipsoxr_run_device_adjoint_ragged": False,
           "hipsoxr_run_device_vr_ragged": True, "hipsoxr_run_device_vr_ragged_adjoint": True}   # name -> takes io_ratios


class _FakeStream:
    cuda_stream = STREAM


class _Recorder:
    """Stands in for one C entry: copies out the job, its table rows and its ratios at call time; answers "no error"."""

    def __init__(self, with_ratios):
        self.with_ratios, self.calls = with_ratios, []

    def __call__(self, handle, ref, *rest):
        from soxr_amd import _native
        j = getattr(ref, "_obj", ref)     # (byref(job), or the job itself: ctypes passes either as the same pointer)
        rec = {name: getattr(j, name) for name, _ in _native.Job._fields_}
        rows = max(j.n_clips, 1)    # (an empty table stands in one placeholder row)
        rec["rows"] = None if not j.clip_table else \
            np.ctypeslib.as_array((C.c_int64 * (4 * rows)).from_address(j.clip_table)).reshape(rows, 4).copy()
        if self.with_ratios:
            rec["ratios"] = None if not rest[0] else np.ctypeslib.as_array((C.c_double * rows).from_address(rest[0])).copy()
        rec["handle"], rec["stream"] = getattr(handle, "value", handle), rest[-1]
        self.calls.append(rec)
        return None


@pytest.fixture
def entries(monkeypatch):
    import torch
    from soxr_amd import _native
    recs = {name: _Recorder(r) for name, r in ENTRIES.items()}
    for name, rec in recs.items():
        monkeypatch.setattr(_native.lib, name, rec)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _FakeStream())
    return recs


def _want(in_, out, elem, kernel, n_clips, n_channels, in_strides, out_strides, in_frames, out_frames, in_abs0=0, out_k0=0,
          clip_counter=None, dither=0, dither_seed=0, clip_table=None, clip_table_dev=None):
    """every field of hipsoxr_job_t, strides as (clip, frame, channel)"""
    return dict(in_=in_, out=out, elem=elem, kernel=kernel, n_clips=n_clips, n_channels=n_channels,
                in_clip_stride=in_strides[0], in_frame_stride=in_strides[1], in_chan_stride=in_strides[2],
                out_clip_stride=out_strides[0], out_frame_stride=out_strides[1], out_chan_stride=out_strides[2],
                in_abs0=in_abs0, in_frames=in_frames, out_k0=out_k0, out_frames=out_frames, clip_counter=clip_counter,
                dither=dither, dither_seed=dither_seed, clip_table=clip_table, clip_table_dev=clip_table_dev)


def _check(rec, want, plan, stream, rows=None, ratios=None):
    from soxr_amd import _native
    assert set(want) == {name for name, _ in _native.Job._fields_}
    for name in want:
        assert rec[name] == want[name], (name, rec[name], want[name])
    assert rec["handle"] == plan.handle.value and rec["stream"] == stream
    if rows is None:
        assert rec["rows"] is None
    else:
        assert rec["rows"].dtype == np.int64 and np.array_equal(rec["rows"], np.array(rows, np.int64).reshape(-1, 4))
    if "ratios" in rec or ratios is not None:
        assert rec["ratios"].dtype == np.float64 and list(rec["ratios"]) == list(ratios)


def _only(recs, name):
    """the one call made, and to this entry alone"""
    assert [n for n, r in recs.items() if r.calls] == [name] and len(recs[name].calls) == 1
    return recs[name].calls.pop()


def test_plan_run(entries):
    import torch
    from soxr_amd import _native as n, device as dev
    plan = dev.Plan(48000, 44100, "HQ")
    x, y, cc = torch.zeros(600, dtype=torch.int16), torch.zeros(600, dtype=torch.int16), torch.zeros(1, dtype=torch.int64)
    plan.run(x.data_ptr(), y.data_ptr(), n.I16, 3, 2, 100, 92, (200, 2, 1), (184, 2, 1))
    _check(_only(entries, "hipsoxr_run_device"),
           _want(x.data_ptr(), y.data_ptr(), n.I16, n.KERNEL_AUTO, 3, 2, (200, 2, 1), (184, 2, 1), 100, 92), plan, None)
    plan.run(x.data_ptr(), y.data_ptr(), n.I16, 3, 2, 100, 92, (200, 2, 1), (184, 1, 92), stream=0x77, kernel=n.KERNEL_EXACT,
             in_abs0=5, out_k0=7, clip_counter=cc.data_ptr(), dither=3, dither_seed=(1 << 32) + 12345)
    _check(_only(entries, "hipsoxr_run_device"),
           _want(x.data_ptr(), y.data_ptr(), n.I16, n.KERNEL_EXACT, 3, 2, (200, 2, 1), (184, 1, 92), 100, 92, in_abs0=5, out_k0=7,
                 clip_counter=cc.data_ptr(), dither=1, dither_seed=12345), plan, 0x77)
    plan.run(x.data_ptr(), y.data_ptr(), n.F32, 1, 1, 100, 92, (0, 1, 1), (0, 1, 1), dither=False, dither_seed=0xFFFFFFFF)
    _check(_only(entries, "hipsoxr_run_device"),
           _want(x.data_ptr(), y.data_ptr(), n.F32, n.KERNEL_AUTO, 1, 1, (0, 1, 1), (0, 1, 1), 100, 92, dither_seed=0xFFFFFFFF), plan, None)


def test_plan_run_adjoint_with_and_without_a_clip_table(entries):
    import torch
    from soxr_amd import _native as n, device as dev
    plan = dev.Plan(48000, 44100, "HQ")
    gy, gx = torch.zeros(400, dtype=torch.float64), torch.zeros(440, dtype=torch.float64)
    plan.run_adjoint(gy.data_ptr(), gx.data_ptr(), n.F64, 2, 2, 90, 100, (200, 2, 1), (220, 2, 1))
    _check(_only(entries, "hipsoxr_run_device_adjoint"),
           _want(gy.data_ptr(), gx.data_ptr(), n.F64, n.KERNEL_AUTO, 2, 2, (200, 2, 1), (220, 2, 1), 90, 100), plan, None)
    table = np.array([[0, 90, 0, 100], [180, 45, 200, 50]], np.int64)
    plan.run_adjoint(gy.data_ptr(), gx.data_ptr(), n.F64, 2, 2, 90, 100, (0, 2, 1), (0, 2, 1), stream=0x99, kernel=n.KERNEL_ADJOINT,
                     clip_table=table.ctypes.data)
    _check(_only(entries, "hipsoxr_run_device_adjoint"),
           _want(gy.data_ptr(), gx.data_ptr(), n.F64, n.KERNEL_ADJOINT, 2, 2, (0, 2, 1), (0, 2, 1), 90, 100, clip_table=table.ctypes.data),
           plan, 0x99, rows=table)


ROWS = [[40, 90, 0, 100], [0, 7, 200, 8], [300, 120, 216, 60]]     # extents: column 1's maximum 120, column 3's 100


def test_the_three_table_entries_with_a_three_row_table(entries):
    import torch
    from soxr_amd import _native as n, device as dev
    plan = dev.Plan(17600, 16000, "HQ", vr=True)
    a, b = torch.zeros(1000), torch.zeros(1000)
    tdev, cc = torch.zeros(12, dtype=torch.int64), torch.zeros(1, dtype=torch.int64)
    ratios = [1.1, 1.0, 0.5]

    plan.run_adjoint_ragged(a.data_ptr(), b.data_ptr(), n.F32, 2, ROWS, (2, 1), (3, 1))        # a list of rows, no device table
    rec = _only(entries, "hipsoxr_run_device_adjoint_ragged")
    _check(rec, _want(a.data_ptr(), b.data_ptr(), n.F32, n.KERNEL_AUTO, 3, 2, (0, 2, 1), (0, 3, 1), 120, 100, clip_table=rec["clip_table"]),
           plan, None, rows=ROWS)
    flat32 = np.array(ROWS, np.int32).reshape(-1)                                                   # any integer array of 4 n entries
    plan.run_adjoint_ragged(a.data_ptr(), b.data_ptr(), n.F32, 2, flat32, (2, 1), (3, 1), 0x31, n.KERNEL_ADJOINT_FFT, tdev.data_ptr())
    rec = _only(entries, "hipsoxr_run_device_adjoint_ragged")
    _check(rec, _want(a.data_ptr(), b.data_ptr(), n.F32, n.KERNEL_ADJOINT_FFT, 3, 2, (0, 2, 1), (0, 3, 1), 120, 100,
                      clip_table=rec["clip_table"], clip_table_dev=tdev.data_ptr()), plan, 0x31, rows=ROWS)
    own = np.array(ROWS, np.int64)                                                                  # an int64 [n, 4] array is passed as it is
    plan.run_adjoint_ragged(a.data_ptr(), b.data_ptr(), n.F32, 2, own, (2, 1), (3, 1))
    assert _only(entries, "hipsoxr_run_device_adjoint_ragged")["clip_table"] == own.ctypes.data

    plan.run_vr_ragged(a.data_ptr(), b.data_ptr(), n.I16, 2, ROWS, ratios, (2, 1), (1, 500))
    rec = _only(entries, "hipsoxr_run_device_vr_ragged")
    _check(rec, _want(a.data_ptr(), b.data_ptr(), n.I16, n.KERNEL_AUTO, 3, 2, (0, 2, 1), (0, 1, 500), 120, 100, clip_table=rec["clip_table"]),
           plan, None, rows=ROWS, ratios=ratios)
    plan.run_vr_ragged(a.data_ptr(), b.data_ptr(), n.I16, 2, ROWS, np.array(ratios, np.float32), (2, 1), (2, 1), 0x32, n.KERNEL_GATHER,
                       tdev.data_ptr(), cc.data_ptr(), True, (5 << 32) + 9)
    rec = _only(entries, "hipsoxr_run_device_vr_ragged")
    _check(rec, _want(a.data_ptr(), b.data_ptr(), n.I16, n.KERNEL_GATHER, 3, 2, (0, 2, 1), (0, 2, 1), 120, 100, clip_counter=cc.data_ptr(),
                      dither=1, dither_seed=9, clip_table=rec["clip_table"], clip_table_dev=tdev.data_ptr()),
           plan, 0x32, rows=ROWS, ratios=[float(np.float32(r)) for r in ratios])

    plan.run_vr_ragged_adjoint(a.data_ptr(), b.data_ptr(), n.F64, 1, ROWS, ratios, (1, 1), (1, 1), 0x33, n.KERNEL_ADJOINT, tdev.data_ptr())
    rec = _only(entries, "hipsoxr_run_device_vr_ragged_adjoint")
    _check(rec, _want(a.data_ptr(), b.data_ptr(), n.F64, n.KERNEL_ADJOINT, 3, 1, (0, 1, 1), (0, 1, 1), 120, 100,
                      clip_table=rec["clip_table"], clip_table_dev=tdev.data_ptr()), plan, 0x33, rows=ROWS, ratios=ratios)

    for run in (plan.run_vr_ragged, plan.run_vr_ragged_adjoint):
        with pytest.raises(ValueError, match="one io ratio per clip"):
            run(a.data_ptr(), b.data_ptr(), n.F32, 1, ROWS, ratios[:2], (1, 1), (1, 1))
    assert not any(r.calls for r in entries.values())


def test_the_three_table_entries_with_an_empty_table(entries):
    from soxr_amd import _native as n, device as dev
    plan = dev.Plan(17600, 16000, "HQ", vr=True)
    none = np.zeros((0, 4), np.int64)
    plan.run_adjoint_ragged(None, None, n.F32, 0, none, (0, 0), (0, 0), kernel=n.KERNEL_ADJOINT)
    rec = _only(entries, "hipsoxr_run_device_adjoint_ragged")
    assert rec["clip_table"], "a placeholder row stands in: the entry refuses a NULL table"
    _check(rec, _want(None, None, n.F32, n.KERNEL_ADJOINT, 0, 0, (0, 0, 0), (0, 0, 0), 0, 0, clip_table=rec["clip_table"]),
           plan, None, rows=[[0, 0, 0, 0]])
    for name, run in (("hipsoxr_run_device_vr_ragged", plan.run_vr_ragged), ("hipsoxr_run_device_vr_ragged_adjoint", plan.run_vr_ragged_adjoint)):
        run(None, None, n.I16, 1, [], [], (1, 1), (1, 1), 0x41)
        rec = _only(entries, name)
        assert rec["clip_table"]
        _check(rec, _want(None, None, n.I16, n.KERNEL_AUTO, 0, 1, (0, 1, 1), (0, 1, 1), 0, 0, clip_table=rec["clip_table"]),
               plan, 0x41, rows=[[0, 0, 0, 0]], ratios=[1.0])


def test_prepared_job_for_one_two_and_strided_three_dimensions(entries):
    import torch
    from soxr_amd import _native as n, device as dev
    plan = dev.Plan(48000, 44100, "HQ")
    o100 = plan.out_len(100)

    x, out = torch.zeros(100), torch.zeros(o100)
    pj = dev.PreparedJob(plan, x, out)
    assert not any(r.calls for r in entries.values()), "building the job launches nothing"
    pj.launch()
    _check(_only(entries, "hipsoxr_run_device"),
           _want(x.data_ptr(), out.data_ptr(), n.F32, n.KERNEL_AUTO, 1, 1, (100, 1, 1), (o100, 1, 1), 100, o100), plan, STREAM)

    x, out, cc = torch.zeros(100, 2, dtype=torch.int16), torch.zeros(o100, 2, dtype=torch.int16), torch.zeros(1, dtype=torch.int64)
    pj = dev.PreparedJob(plan, x, out, n.KERNEL_EXACT, True, cc, (3 << 32) + 77)
    pj.launch()
    pj.launch()
    again = entries["hipsoxr_run_device"].calls.pop()
    first = _only(entries, "hipsoxr_run_device")
    want = _want(x.data_ptr(), out.data_ptr(), n.I16, n.KERNEL_EXACT, 1, 2, (200, 2, 1), (2 * o100, 2, 1), 100, o100,
                 clip_counter=cc.data_ptr(), dither=1, dither_seed=77)
    _check(first, want, plan, STREAM)
    _check(again, want, plan, STREAM)

    xb, ob = torch.zeros(4, 300, 3, dtype=torch.float64), torch.zeros(2, 2 * o100, 4, dtype=torch.float64)
    x, out = xb[::2, 10:110, :2], ob[:, ::2, 1:3]
    assert tuple(x.shape) == (2, 100, 2) and tuple(out.shape) == (2, o100, 2)
    pj = dev.PreparedJob(plan, x, out, kernel=n.KERNEL_GATHER, dither=0)
    pj.launch()
    _check(_only(entries, "hipsoxr_run_device"),
           _want(xb[0, 10].data_ptr(), ob[0, 0, 1:].data_ptr(), n.F64, n.KERNEL_GATHER, 2, 2, (1800, 3, 1), (8 * o100, 8, 1), 100, o100),
           plan, STREAM)

    with pytest.raises(ValueError, match="out has the wrong shape for this plan"):
        dev.PreparedJob(plan, torch.zeros(100), torch.zeros(o100 + 1))
    for bad in (torch.zeros(()), torch.zeros(1, 1, 100, 1)):
        with pytest.raises(ValueError):
            dev.PreparedJob(plan, bad, torch.zeros(o100))


def _ragged_clips(dtype, mono):
    """out of address order, one empty, one strided (the one that is copied)"""
    import torch
    buf = torch.zeros(5000, dtype=dtype) if mono else torch.zeros(5000, 2, dtype=dtype)
    return buf, [buf[3500:4999], buf[100:1100], buf[3000:3000], buf[2000:2400:2]], [1499, 1000, 0, 200]


def _check_ragged_job(job, clips, n_in, n_out, ch):
    """the table over the clips where they lie, from the tensors the job keeps -> (base pointer, table)"""
    import torch
    keep, es = job._keep, clips[0].element_size()
    assert [k is c for k, c in zip(keep, clips)] == [True, True, True, False], "only the strided clip is copied"
    assert keep[3].is_contiguous() and torch.equal(keep[3], clips[3])
    base = min(k.data_ptr() for k in keep if k.shape[0] > 0)
    table = np.array([[(k.data_ptr() - base) // es if n else 0, n, ch * sum(n_out[:i]), n_out[i]]
                      for i, (k, n) in enumerate(zip(keep, n_in))], np.int64)
    assert table[1, 0] == 0 or table[3, 0] == 0, "the lowest clip is the base"
    assert table[0, 0] - table[1, 0] == 3400 * ch and table[2, 0] == 0
    assert job.n_in == n_in and job.n_out == n_out and np.array_equal(job._table, table) and job._table.dtype == np.int64
    assert job._job.clip_table == job._table.ctypes.data, "_table IS the array the job points at"
    assert job._job.clip_table_dev == job._table_dev.data_ptr() and np.array_equal(job._table_dev.numpy(), table)
    assert tuple(job.y.shape) == (sum(n_out), ch) and job.y.dtype == clips[0].dtype
    assert [tuple(o.shape) for o in job.outputs()] == [(m,) if clips[0].ndim == 1 else (m, ch) for m in n_out]
    assert all(o.data_ptr() == job.y[sum(n_out[:i]):].data_ptr() for i, o in enumerate(job.outputs()) if n_out[i])
    return base, table


def test_ragged_job_without_io_ratios(entries):
    import torch
    from soxr_amd import _native as n, device as dev, dist
    plan = dev.Plan(48000, 44100, "HQ")
    buf, clips, n_in = _ragged_clips(torch.int16, mono=False)
    n_out = [plan.out_len(m) for m in n_in]
    cc = torch.zeros(1, dtype=torch.int64)
    job = dist.RaggedJob(plan, clips, kernel=n.KERNEL_EXACT, dither_seed=(1 << 32) + 7, clip_counter=cc)
    assert not any(r.calls for r in entries.values()) and job._ratios is None
    base, table = _check_ragged_job(job, clips, n_in, n_out, 2)
    want = _want(base, job.y.data_ptr(), n.I16, n.KERNEL_EXACT, 4, 2, (0, 2, 1), (0, 2, 1), 1499, max(n_out), clip_counter=cc.data_ptr(),
                 dither=1, dither_seed=7, clip_table=job._table.ctypes.data, clip_table_dev=job._table_dev.data_ptr())
    job.launch()
    _check(_only(entries, "hipsoxr_run_device"), want, plan, STREAM, rows=table)
    job._table[1, 3] += 1              # the table is read when the call is made: an edit in place reaches the next launch
    job.launch()
    assert _only(entries, "hipsoxr_run_device")["rows"][1, 3] == n_out[1] + 1

    off = dist.RaggedJob(plan, clips, stream=0x51, dither=False)       # a raw stream handle; dither off by name
    off.launch()
    base, table = _check_ragged_job(off, clips, n_in, n_out, 2)
    _check(_only(entries, "hipsoxr_run_device"),
           _want(base, off.y.data_ptr(), n.I16, n.KERNEL_AUTO, 4, 2, (0, 2, 1), (0, 2, 1), 1499, max(n_out),
                 clip_table=off._table.ctypes.data, clip_table_dev=off._table_dev.data_ptr()), plan, 0x51, rows=table)

    empty = dist.RaggedJob(plan, [buf[5:5], buf[9:9]])                 # nothing to emit: nothing is launched
    empty.launch()
    assert not any(r.calls for r in entries.values())
    assert (empty._job.in_ or 0) == empty.y.data_ptr() and np.array_equal(empty._table, np.zeros((2, 4), np.int64))
    assert (empty._job.n_clips, empty._job.in_frames, empty._job.out_frames) == (2, 0, 0)

    with pytest.raises(ValueError, match="no clips"):
        dist.RaggedJob(plan, [])
    for bad in ([buf[:10], buf[:10, 0]], [buf[:10], buf[:10].float()], [buf[:10], buf[None, :10]]):
        with pytest.raises(ValueError, match="clips of one job share device, dtype and channel count; each is "):
            dist.RaggedJob(plan, bad)


def test_ragged_job_with_io_ratios(entries):
    import torch
    from soxr_amd import _native as n, device as dev, dist
    plan = dev.Plan(17600, 16000, "HQ", vr=True)
    buf, clips, n_in = _ragged_clips(torch.float32, mono=True)
    ratios = [1.1, 1.0, 0.75, 0.5]
    n_out = [plan.vr_out_len(m, r) for m, r in zip(n_in, ratios)]
    assert n_out[1] == 1000 and n_out[2] == 0 and n_out[3] == 400
    job = dist.RaggedJob(plan, clips, kernel=n.KERNEL_GATHER, io_ratios=ratios)
    assert not any(r.calls for r in entries.values())
    base, table = _check_ragged_job(job, clips, n_in, n_out, 1)
    assert job._ratios.dtype == np.float64 and list(job._ratios) == ratios
    job.launch()
    _check(_only(entries, "hipsoxr_run_device_vr_ragged"),
           _want(base, job.y.data_ptr(), n.F32, n.KERNEL_GATHER, 4, 1, (0, 1, 1), (0, 1, 1), 1499, max(n_out),
                 clip_table=job._table.ctypes.data, clip_table_dev=job._table_dev.data_ptr()), plan, STREAM, rows=table, ratios=ratios)

    empty = dist.RaggedJob(plan, [buf[5:5]], io_ratios=[1.0])          # an empty job still goes to this entry
    empty.launch()
    rec = _only(entries, "hipsoxr_run_device_vr_ragged")
    assert (rec["n_clips"], rec["in_frames"], rec["out_frames"]) == (1, 0, 0) and list(rec["ratios"]) == [1.0]


class _FakeEvent:
    def record(self, stream):
        stream.log.append(("record", self))


class _LoggedStream:
    def __init__(self, handle):
        self.cuda_stream, self.log = handle, []

    def wait_event(self, e):
        self.log.append(("wait", e))


def test_host_pipe_block_descriptor(entries):
    """`_HostPipe._issue` for a block of two int16 stereo clips, on host tensors with the stream calls faked: the packed-to-
    packed table and the job of the one launch."""
    import torch
    from soxr_amd import _native as n, device as dev, dist
    plan = dev.Plan(48000, 44100, "HQ")
    n_in = [300, 120]
    n_out = [plan.out_len(m) for m in n_in]
    pipe = object.__new__(dist._HostPipe)
    pipe.torch = types.SimpleNamespace(int16=torch.int16, empty=torch.empty,
                                       cuda=types.SimpleNamespace(stream=lambda s: contextlib.nullcontext(), Event=_FakeEvent))
    pipe.plan, pipe.device, pipe.kernel, pipe.ch, pipe.tdtype, pipe.pinned_results = plan, "cpu", n.KERNEL_EXACT, 2, torch.int16, False
    pipe.sin, pipe.sc, pipe.sout = _LoggedStream(0x61), _LoggedStream(0x62), _LoggedStream(0x63)
    pipe.pin_in = [torch.arange(840, dtype=torch.int16) + s for s in range(3)]
    pipe.dev_in = [torch.zeros(840, dtype=torch.int16) for _ in range(3)]
    pipe.dev_out = [torch.arange(2 * sum(n_out), dtype=torch.int16) + s for s in range(3)]
    pipe.pin_out = [torch.zeros(2 * sum(n_out), dtype=torch.int16) for _ in range(3)]
    st = dist._PipeRun(n_in, n_out, 2, 2, 1 << 20, 3)
    assert st.blocks == [[0, 1]]
    pipe._issue(st, 0)
    rec = _only(entries, "hipsoxr_run_device")
    assert rec["clip_table"]
    _check(rec, _want(pipe.dev_in[0].data_ptr(), pipe.dev_out[0].data_ptr(), n.I16, n.KERNEL_EXACT, 2, 2, (0, 2, 1), (0, 2, 1), 300, max(n_out),
                      dither=1, clip_table=rec["clip_table"]), plan, 0x62,
           rows=[[0, 300, 0, n_out[0]], [600, 120, 2 * n_out[0], n_out[1]]])
    assert torch.equal(pipe.dev_in[0], pipe.pin_in[0]) and torch.equal(pipe.pin_out[0], pipe.dev_out[0])   # h2d before, d2h behind
    assert [what for what, _ in pipe.sc.log] == ["wait", "record"] and pipe.sc.log[0][1] is st.ev_free_in[0]
    assert st.ev_run[0] is pipe.sc.log[1][1] and pipe.sout.log[0] == ("wait", st.ev_run[0]) and st.ev_out[0] is pipe.sout.log[1][1]


def test_packed_adjoints_name_what_they_refuse_before_any_call(entries):
    import torch
    from soxr_amd import device as dev, dist
    plan, vr = dev.Plan(48000, 44100, "HQ"), dev.Plan(17600, 16000, "HQ", vr=True)
    g = [torch.zeros(90), torch.zeros(45)]
    for call, count, host in (
            (lambda gys, nx: dist.resample_ragged_adjoint(plan, gys, nx), "one in_frames entry per cotangent clip",
             r"resample_tensor needs a device tensor \(soxr_amd has no CPU fallback\)"),
            (lambda gys, nx: dist.resample_varispeed_adjoint(vr, gys, nx, [1.0] * len(gys)), "one in_frames entry and one io ratio per cotangent clip",
             r"resample_varispeed_adjoint needs device tensors \(soxr_amd has no CPU fallback\)")):
        with pytest.raises(ValueError, match="^no clips$"):
            call([], [])
        with pytest.raises(ValueError, match="^" + count + "$"):
            call(g, [100])
        with pytest.raises(ValueError, match="clips of one job share device, dtype and channel count; each is "):
            call([g[0], g[1].double()], [100, 50])
        with pytest.raises(RuntimeError, match=host):
            call(g, [100, 50])
    with pytest.raises(ValueError, match="one in_frames entry and one io ratio per cotangent clip"):
        dist.resample_varispeed_adjoint(vr, g, [100, 50], [1.0])
    assert not any(r.calls for r in entries.values())
