"""Host side of ragged variable-rate batches (no GPU): the header declares the two entries and no new version, the binding
has them, Plan.vr / Plan.vr_out_len, every refusal by name is decided before anything touches a device (asked with empty or
NULL-pointer jobs), and RaggedJob(io_ratios=None) builds the job it always built."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from vr_sim import ONE, q64  # noqa: E402


def _header():
    with open(os.path.join(ROOT, "include", "hipsoxr.h")) as f:
        return f.read()


def test_header_declares_the_two_entries_and_still_says_0_7_0():
    text = _header()
    assert '#define HIPSOXR_VERSION_STRING "0.7.0"' in text
    assert "no new field — the entries hipsoxr_plan_vr_out_len and hipsoxr_run_device_vr_ragged" in text
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"HIPSOXR_API\s+uint64_t\s+hipsoxr_plan_vr_out_len\(const hipsoxr_plan_t \*, uint64_t in_len, double io_ratio\);", plain)
    assert re.search(r"HIPSOXR_API\s+hipsoxr_error_t\s+hipsoxr_run_device_vr_ragged\(hipsoxr_plan_t \*, const hipsoxr_job_t \*job,\s*"
                     r"const double \*io_ratios\s*, void \*hip_stream\);", plain)
    job = re.search(r"typedef struct \{([^}]*)\}\s*hipsoxr_job_t;", plain, re.S).group(1)
    assert job.strip().endswith("const int64_t *clip_table_dev;"), "no field behind clip_table_dev"


def test_native_binds_them():
    from soxr_amd import _native
    assert _native.version().startswith("hipsoxr-0.7.0")
    assert _native.SIGNATURES["hipsoxr_plan_vr_out_len"] == (C.c_uint64, [C.c_void_p, C.c_uint64, C.c_double])
    assert _native.SIGNATURES["hipsoxr_run_device_vr_ragged"][1] == [C.c_void_p, C.POINTER(_native.Job), C.c_void_p, C.c_void_p]
    assert _native.lib.hipsoxr_plan_vr_out_len.restype is C.c_uint64
    assert [f[0] for f in _native.Job._fields_][-4:] == ["dither", "dither_seed", "clip_table", "clip_table_dev"], "hipsoxr_job_t has the fields it had"


def test_plan_vr_and_vr_out_len():
    from soxr_amd import device as dev
    vr, const = dev.Plan(17600, 16000, "HQ", vr=True), dev.Plan(17600, 16000, "HQ")
    assert vr.vr is True and const.vr is False and vr.phases > 0
    assert const.vr_out_len(1000, 1.0) == 0, "not a variable-rate plan"
    assert vr.vr_out_len(0, 1.0) == 0
    assert vr.vr_out_len(1000, 1.0) == 1000 and vr.vr_out_len(1000, 0.5) == 2000
    for n in (1, 107, 1000, 2 ** 31 + 7):
        for r in (1.1, 1.0, 0.9070294784580499, 0.5, 1.1 * (1 - 2.0 ** -40)):
            s = q64(r)  # the count of k >= 0 with k S + S/2 <= n 2^64
            assert vr.vr_out_len(n, r) == (n * ONE - s // 2) // s + 1, (n, r)
    assert vr.vr_out_len(1000, 1.2) == 0 and vr.vr_out_len(1000, 2.0 ** -20) == 0 and vr.vr_out_len(1000, float("nan")) == 0


def _ask(plan, elem, table, ratios, kernel=0, in_abs0=0, out_k0=0, null_table=False, null_ratios=False, in_frames=None, out_frames=None):
    """the entry on NULL buffers: whatever it answers, it answered without a device"""
    from soxr_amd import _native
    t = np.ascontiguousarray(table, np.int64).reshape(-1, 4)
    r = np.ascontiguousarray(ratios, np.float64)
    j = _native.Job()
    j.elem, j.kernel, j.n_clips, j.n_channels = elem, kernel, t.shape[0], 1
    j.in_frame_stride = j.in_chan_stride = j.out_frame_stride = j.out_chan_stride = 1
    j.in_abs0, j.out_k0 = in_abs0, out_k0
    j.in_frames = int(t[:, 1].max()) if in_frames is None else in_frames
    j.out_frames = int(t[:, 3].max()) if out_frames is None else out_frames
    j.clip_table = None if null_table else t.ctypes.data
    err = _native.lib.hipsoxr_run_device_vr_ragged(plan.handle, C.byref(j), None if null_ratios else r.ctypes.data, None)
    return err.decode() if err else None


def test_every_refusal_is_named_before_anything_is_launched():
    from soxr_amd import _native, device as dev
    vr, const = dev.Plan(17600, 16000, "HQ", vr=True), dev.Plan(17600, 16000, "HQ")
    ok_row, F32 = [[0, 100, 0, 90]], _native.F32
    big = (1 << 30) + 1
    cases = [
        (dict(plan=const), "not a variable-rate plan"),
        (dict(null_table=True), "needs a clip_table"),
        (dict(null_ratios=True), "needs io_ratios"),
        (dict(ratios=[2.0 ** -20]), r"io ratio is out of range \(2\^-20 < io ratio < 2\^20\)"),
        (dict(ratios=[2.0 ** 20]), "io ratio is out of range"),
        (dict(ratios=[float("nan")]), "io ratio is out of range"),
        (dict(ratios=[1.1 * (1 + 4e-12)]), r"^io ratio exceeds the maximum given at creation \(the filter would alias\)$"),
        (dict(table=[[-1, 100, 0, 90]]), "offset or frame count is negative"),
        (dict(table=[[0, 100, -1, 90]]), "offset or frame count is negative"),
        (dict(table=[[0, -1, 0, 0]], in_frames=0), "offset or frame count is negative"),
        (dict(table=[[0, 100, 0, -1]], out_frames=0), "offset or frame count is negative"),
        (dict(in_frames=99), "exceed the job's in_frames / out_frames"),
        (dict(out_frames=89), "exceed the job's in_frames / out_frames"),
        (dict(table=[[0, 100, 0, 92]], ratios=[1.1]), "exceed hipsoxr_plan_vr_out_len"),   # 91 outputs at 1.1
        (dict(table=[[0, 0, 0, 1]]), "exceed hipsoxr_plan_vr_out_len"),
        (dict(table=[[0, big, 0, big]]), r"more than 2\^30 outputs"),
        (dict(in_abs0=5), r"whole signals only \(in_abs0 == 0, out_k0 == 0\)"),
        (dict(out_k0=5), "whole signals only"),
        (dict(elem=_native.F16), "float16 / bfloat16 clip tables are not served"),
        (dict(elem=_native.BF16), "float16 / bfloat16 clip tables are not served"),
    ]
    for k in (_native.KERNEL_TILE, _native.KERNEL_TILE_VALU, _native.KERNEL_TILE_MFMA, _native.KERNEL_FFT, _native.KERNEL_WAVE_DOT,
              _native.KERNEL_FFT_F64, _native.KERNEL_FFT_PCM, _native.KERNEL_ADJOINT):
        cases.append((dict(kernel=k), "served by the exact engine alone"))
    assert vr.vr_out_len(100, 1.1) == 91 and vr.vr_out_len(100, 1.0) == 100
    for kw, want in cases:
        args = dict(plan=vr, elem=F32, table=ok_row, ratios=[1.0])
        args.update(kw)
        got = _ask(**args)
        assert got is not None and re.search(want, got), (kw, got)
        assert got.startswith("variable-rate ragged batch: ") or got.startswith("io ratio exceeds"), got
    # the second clip's ratio and row are looked at too
    assert re.search("exceeds the maximum", _ask(vr, F32, [[0, 10, 0, 5], [0, 10, 0, 5]], [1.0, 1.3]))
    assert re.search("vr_out_len", _ask(vr, F32, [[0, 10, 0, 5], [0, 10, 0, 11]], [1.0, 1.0]))


def test_admitted_empty_jobs_succeed_without_a_device():
    from soxr_amd import _native, device as dev
    vr = dev.Plan(17600, 16000, "HQ", vr=True)
    for elem in (_native.F32, _native.F64, _native.I32, _native.I16):
        for k in (_native.KERNEL_AUTO, _native.KERNEL_EXACT, _native.KERNEL_GATHER):
            assert _ask(vr, elem, [[0, 100, 0, 0], [0, 0, 0, 0]], [1.0, 1.1 * (1 + 0.5e-12)], kernel=k) is None  # out_frames == 0
    assert _ask(vr, _native.F32, np.zeros((0, 4)), np.zeros(0), in_frames=0, out_frames=0) is None   # no clips
    vr.run_vr_ragged(None, None, _native.I16, 1, np.zeros((0, 4), np.int64), [], (1, 1), (1, 1))
    with pytest.raises(ValueError, match="one io ratio per clip"):
        vr.run_vr_ragged(None, None, _native.F32, 1, [[0, 1, 0, 0]], [1.0, 1.0], (1, 1), (1, 1))
    with pytest.raises(RuntimeError, match="exceeds the maximum"):
        vr.run_vr_ragged(None, None, _native.F32, 1, [[0, 1, 0, 0]], [1.5], (1, 1), (1, 1))


class _FakeStream:
    cuda_stream = 0


def _host_job(monkeypatch, plan, clips, **kw):
    """RaggedJob on host tensors (nothing is launched): the stream query is the one call that needs a device"""
    import torch
    from soxr_amd import dist
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _FakeStream())
    return dist.RaggedJob(plan, clips, **kw)


def test_ragged_job_without_ratios_builds_the_job_it_always_built(monkeypatch):
    import torch
    from soxr_amd import _native, device as dev
    plan = dev.Plan(48000, 44100, "HQ")
    buf = torch.zeros(5000, 2, dtype=torch.int16)
    clips = [buf[100:1100], buf[2000:2003], buf[3000:3000], buf[3500:4999]]
    job = _host_job(monkeypatch, plan, clips, kernel=_native.KERNEL_EXACT, dither_seed=7)
    same = _host_job(monkeypatch, plan, clips, kernel=_native.KERNEL_EXACT, dither_seed=7, io_ratios=None)
    n_in = [1000, 3, 0, 1499]
    n_out = [plan.out_len(n) for n in n_in]
    want_table = np.array([[0, n_in[0], 0, n_out[0]], [3800, 3, 2 * n_out[0], n_out[1]], [0, 0, 2 * sum(n_out[:2]), 0],
                           [6800, 1499, 2 * sum(n_out[:3]), n_out[3]]], np.int64)
    for jb in (job, same):
        j = jb._job
        assert jb._ratios is None and jb.n_in == n_in and jb.n_out == n_out
        assert np.array_equal(jb._table, want_table)
        assert (j.in_, j.out, j.elem, j.kernel) == (buf[100:].data_ptr(), jb.y.data_ptr(), _native.I16, _native.KERNEL_EXACT)
        assert (j.n_clips, j.n_channels) == (4, 2)
        assert (j.in_clip_stride, j.in_frame_stride, j.in_chan_stride, j.out_clip_stride, j.out_frame_stride, j.out_chan_stride) == (0, 2, 1, 0, 2, 1)
        assert (j.in_abs0, j.in_frames, j.out_k0, j.out_frames) == (0, 1499, 0, max(n_out))
        assert (j.dither, j.dither_seed, j.clip_counter) == (1, 7, None)
        assert j.clip_table == jb._table.ctypes.data and j.clip_table_dev == jb._table_dev.data_ptr()
        assert tuple(jb.y.shape) == (sum(n_out), 2) and [tuple(o.shape) for o in jb.outputs()] == [(n, 2) for n in n_out]


def test_ragged_job_with_ratios_needs_a_variable_rate_plan_and_sizes_by_vr_out_len(monkeypatch):
    import torch
    from soxr_amd import device as dev, dist
    clips = [torch.zeros(1000), torch.zeros(0), torch.zeros(333)]
    with pytest.raises(ValueError, match="io_ratios needs a variable-rate plan"):
        dist.RaggedJob(dev.Plan(17600, 16000, "HQ"), clips, io_ratios=[1.0, 1.0, 1.0])
    vr = dev.Plan(17600, 16000, "HQ", vr=True)
    with pytest.raises(ValueError, match="one io ratio per clip"):
        dist.RaggedJob(vr, clips, io_ratios=[1.0, 1.0])
    job = _host_job(monkeypatch, vr, clips, io_ratios=[1.1, 1.0, 0.5])
    assert job.n_out == [vr.vr_out_len(1000, 1.1), 0, 666] and job.n_out[0] == 909
    assert np.array_equal(job._table[:, 3], job.n_out) and job._job.out_frames == 909 and job._job.in_frames == 1000
    assert job._ratios.dtype == np.float64 and list(job._ratios) == [1.1, 1.0, 0.5]
    assert [tuple(o.shape) for o in job.outputs()] == [(909,), (0,), (666,)]


def test_varispeed_refuses_a_gradient_by_name():
    import torch
    from soxr_amd import device as dev, dist
    vr = dev.Plan(17600, 16000, "HQ", vr=True)
    with pytest.raises(RuntimeError, match="no gradient is served"):
        dist.resample_varispeed(vr, [torch.zeros(100, requires_grad=True)], [1.0])
    assert "Plan(max(factors) * rate, rate, quality, vr=True)" in dist.resample_varispeed.__doc__
