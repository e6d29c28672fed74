"""Host side of the ragged variable-rate adjoint (no GPU): the header declares hipsoxr_run_device_vr_ragged_adjoint and no new
version, the library exports it and the binding has it, every refusal by name is decided before anything touches a device
(asked with NULL-pointer jobs), admitted empty jobs succeed, `resample_varispeed` keeps its refusal of a gradient without
`grad_kernel` and names what it refuses with it, and the three older entries refuse what they refused."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAME = "hipsoxr_run_device_vr_ragged_adjoint"


def _header():
    with open(os.path.join(ROOT, "include", "hipsoxr.h")) as f:
        return f.read()


def test_header_declares_the_entry_and_still_says_0_7_0():
    text = _header()
    assert '#define HIPSOXR_VERSION_STRING "0.7.0"' in text
    assert "no new field — the entries hipsoxr_plan_vr_out_len and hipsoxr_run_device_vr_ragged" in text
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"HIPSOXR_API\s+hipsoxr_error_t\s+" + NAME + r"\(hipsoxr_plan_t \*, const hipsoxr_job_t \*job,\s*"
                     r"const double \*io_ratios\s*, void \*hip_stream\);", plain)
    job = re.search(r"typedef struct \{([^}]*)\}\s*hipsoxr_job_t;", plain, re.S).group(1)
    assert job.strip().endswith("const int64_t *clip_table_dev;"), "no field behind clip_table_dev"
    fwd = re.search(r"/\*((?:(?!\*/).)*)\*/\s*HIPSOXR_API hipsoxr_error_t hipsoxr_run_device_vr_ragged\(", text, re.S).group(1)
    not_served = fwd.split("Not served:")[1].split(".")[0]
    assert "gradients" not in not_served and NAME in fwd, "the forward entry points at its gradient"


def test_library_exports_it_and_native_binds_it():
    from soxr_amd import _native
    assert _native.version().startswith("hipsoxr-0.7.0")
    assert _native.SIGNATURES[NAME][1] == [C.c_void_p, C.POINTER(_native.Job), C.c_void_p, C.c_void_p]
    assert getattr(_native.lib, NAME).restype is _native.SIGNATURES[NAME][0]
    lib = os.path.join(ROOT, "python-soxr_amd", "soxr_amd", "libhipsoxr.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\sT " + NAME + r"$", syms, re.M)
    assert [f[0] for f in _native.Job._fields_][-4:] == ["dither", "dither_seed", "clip_table", "clip_table_dev"]


def _ask(plan, elem, table, ratios, kernel=0, in_abs0=0, out_k0=0, null_table=False, null_ratios=False, in_frames=None, out_frames=None,
         entry=NAME):
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
    err = getattr(_native.lib, entry)(plan.handle, C.byref(j), None if null_ratios else r.ctypes.data, None)
    return err.decode() if err else None


def test_every_refusal_is_named_before_anything_is_launched():
    from soxr_amd import _native, device as dev
    vr, const = dev.Plan(17600, 16000, "HQ", vr=True), dev.Plan(17600, 16000, "HQ")
    ok_row, F32 = [[0, 90, 0, 100]], _native.F32   # rows are { gy offset, n_y, gx offset, n_x }
    big = (1 << 30) + 1
    cases = [
        (dict(plan=const), "not a variable-rate plan"),
        (dict(null_table=True), "needs a clip_table"),
        (dict(null_ratios=True), "needs io_ratios"),
        (dict(ratios=[2.0 ** -20]), r"io ratio is out of range \(2\^-20 < io ratio < 2\^20\)"),
        (dict(ratios=[2.0 ** 20]), "io ratio is out of range"),
        (dict(ratios=[float("nan")]), "io ratio is out of range"),
        (dict(ratios=[1.1 * (1 + 4e-12)]), r"^io ratio exceeds the maximum given at creation \(the filter would alias\)$"),
        (dict(table=[[-1, 90, 0, 100]]), "offset or frame count is negative"),
        (dict(table=[[0, 90, -1, 100]]), "offset or frame count is negative"),
        (dict(table=[[0, -1, 0, 100]], in_frames=0), "offset or frame count is negative"),
        (dict(table=[[0, 0, 0, -1]], out_frames=0), "offset or frame count is negative"),
        (dict(in_frames=89), "exceed the job's in_frames / out_frames"),
        (dict(out_frames=99), "exceed the job's in_frames / out_frames"),
        (dict(table=[[0, 92, 0, 100]], ratios=[1.1]), "exceeds hipsoxr_plan_vr_out_len"),   # 91 outputs at 1.1
        (dict(table=[[0, 101, 0, 100]]), "exceeds hipsoxr_plan_vr_out_len"),
        (dict(table=[[0, 1, 0, 0]]), "exceeds hipsoxr_plan_vr_out_len"),
        (dict(table=[[0, big, 0, big]]), r"more than 2\^30 cotangent samples"),
        (dict(in_abs0=5), r"whole signals only \(in_abs0 == 0, out_k0 == 0\)"),
        (dict(out_k0=5), "whole signals only"),
        (dict(elem=_native.I16), "float32 or float64 elements only"),
        (dict(elem=_native.I32), "float32 or float64 elements only"),
        (dict(elem=_native.F16), "float16 / bfloat16 clip tables are not served"),
        (dict(elem=_native.BF16), "float16 / bfloat16 clip tables are not served"),
    ]
    for k in (_native.KERNEL_GATHER, _native.KERNEL_TILE, _native.KERNEL_TILE_VALU, _native.KERNEL_TILE_MFMA, _native.KERNEL_FFT,
              _native.KERNEL_EXACT, _native.KERNEL_WAVE_DOT, _native.KERNEL_FFT_F64, _native.KERNEL_FFT_PCM, _native.KERNEL_ADJOINT_FFT,
              _native.KERNEL_ADJOINT_TWO_STAGE, _native.KERNEL_ADJOINT_AUTO):
        cases.append((dict(kernel=k), r"served by the exact adjoint alone \(HIPSOXR_KERNEL_AUTO or HIPSOXR_KERNEL_ADJOINT\)"))
    assert vr.vr_out_len(100, 1.1) == 91 and vr.vr_out_len(100, 1.0) == 100
    for kw, want in cases:
        args = dict(plan=vr, elem=F32, table=ok_row, ratios=[1.0])
        args.update(kw)
        got = _ask(**args)
        assert got is not None and re.search(want, got), (kw, got)
        # the entry's own name in front; the two texts about a ratio are the forward entry's rule in its own words
        assert got.startswith("variable-rate ragged adjoint: ") or got.startswith("io ratio exceeds") or "io ratio is out of range" in got, got
    # an admitted job on NULL buffers gets as far as the buffers, under both selectors: everything above was asked first
    for k in (_native.KERNEL_AUTO, _native.KERNEL_ADJOINT):
        assert _ask(vr, F32, ok_row, [1.0], kernel=k) == "variable-rate ragged adjoint: null buffer"
    # the second clip's ratio and row are looked at too
    assert re.search("exceeds the maximum", _ask(vr, F32, [[0, 5, 0, 10], [0, 5, 0, 10]], [1.0, 1.3]))
    assert re.search("vr_out_len", _ask(vr, F32, [[0, 5, 0, 10], [0, 11, 0, 10]], [1.0, 1.0]))


def test_admitted_empty_jobs_succeed_without_a_device():
    from soxr_amd import _native, device as dev
    vr = dev.Plan(17600, 16000, "HQ", vr=True)
    for elem in (_native.F32, _native.F64):
        for k in (_native.KERNEL_AUTO, _native.KERNEL_ADJOINT):
            assert _ask(vr, elem, [[0, 0, 0, 0], [0, 0, 0, 0]], [1.0, 1.1 * (1 + 0.5e-12)], kernel=k) is None  # out_frames == 0
    assert _ask(vr, _native.F32, np.zeros((0, 4)), np.zeros(0), in_frames=0, out_frames=0) is None   # no clips
    vr.run_vr_ragged_adjoint(None, None, _native.F64, 1, np.zeros((0, 4), np.int64), [], (1, 1), (1, 1))
    vr.run_vr_ragged_adjoint(None, None, _native.F32, 0, [[0, 5, 0, 10]], [1.0], (1, 1), (1, 1))       # no channels
    with pytest.raises(ValueError, match="one io ratio per clip"):
        vr.run_vr_ragged_adjoint(None, None, _native.F32, 1, [[0, 0, 0, 1]], [1.0, 1.0], (1, 1), (1, 1))
    with pytest.raises(RuntimeError, match="exceeds the maximum"):
        vr.run_vr_ragged_adjoint(None, None, _native.F32, 1, [[0, 0, 0, 1]], [1.5], (1, 1), (1, 1))


def test_varispeed_keeps_its_refusal_without_grad_kernel_and_takes_the_keyword():
    import torch
    from soxr_amd import _native, device as dev, dist
    vr = dev.Plan(17600, 16000, "HQ", vr=True)
    with pytest.raises(RuntimeError, match=r"resample_varispeed: no gradient is served for per-clip rates \(the adjoint kernels take "
                                           r"constant-rate plans\); detach the clips or call it under torch.no_grad\(\)"):
        dist.resample_varispeed(vr, [torch.zeros(100, requires_grad=True)], [1.0])
    with pytest.raises(RuntimeError, match="no gradient is served"):
        dist.resample_varispeed(vr, [torch.zeros(100, requires_grad=True)], [1.0], grad_kernel=None)
    params = list(inspect.signature(dist.resample_varispeed).parameters.values())
    assert params[-1].name == "grad_kernel" and params[-1].default is None, "the new last keyword, off by default"
    assert [p.name for p in params[:-1]] == ["plan", "clips", "io_ratios", "kernel", "dither", "dither_seed", "clip_counter"]
    doc = dist.resample_varispeed.__doc__
    assert "Plan(max(factors) * rate, rate, quality, vr=True)" in doc and "No gradient is served" not in doc
    assert "grad_kernel=KERNEL_ADJOINT" in doc
    sig = inspect.signature(dist.resample_varispeed_adjoint)
    assert list(sig.parameters) == ["plan", "gys", "in_frames", "io_ratios", "kernel"] and sig.parameters["kernel"].default == _native.KERNEL_AUTO
    assert "run_vr_ragged_adjoint" in dir(dev.Plan)


def test_what_grad_kernel_refuses_is_named_when_the_forward_is_called():
    import torch
    from soxr_amd import _native, device as dev, dist
    vr, const = dev.Plan(17600, 16000, "HQ", vr=True), dev.Plan(17600, 16000, "HQ")
    ADJ = _native.KERNEL_ADJOINT
    for dtype in (torch.int16, torch.int32):
        with pytest.raises(TypeError, match=r"grad_kernel needs float32 or float64 clips \(integer types have no gradient\)"):
            dist.resample_varispeed(vr, [torch.zeros(100, dtype=dtype)], [1.0], grad_kernel=ADJ)
    x = torch.zeros(100, requires_grad=True)
    for kw in (dict(dither=False), dict(dither_seed=3), dict(clip_counter=torch.zeros(1, dtype=torch.int64))):
        with pytest.raises(ValueError, match="dither, dither_seed and clip_counter belong to integer clips"):
            dist.resample_varispeed(vr, [x], [1.0], grad_kernel=ADJ, **kw)
    for k in (_native.KERNEL_ADJOINT_AUTO, _native.KERNEL_ADJOINT_FFT, _native.KERNEL_ADJOINT_TWO_STAGE, _native.KERNEL_EXACT):
        with pytest.raises(RuntimeError, match="variable-rate ragged adjoint: served by the exact adjoint alone"):
            dist.resample_varispeed(vr, [x], [1.0], grad_kernel=k)
    with pytest.raises(RuntimeError, match="variable-rate ragged adjoint: the plan is not a variable-rate plan"):
        dist.resample_varispeed(const, [x], [1.0], grad_kernel=ADJ)
    with pytest.raises(RuntimeError, match="needs device tensors"):   # admitted: it gets as far as the launch, which host tensors have none of
        dist.resample_varispeed_adjoint(vr, [torch.zeros(90)], [100], [1.0])


def test_the_older_entries_refuse_what_they_refused():
    from soxr_amd import _native, device as dev
    vr = dev.Plan(17600, 16000, "HQ", vr=True)
    got = _ask(vr, _native.F32, [[0, 100, 0, 90]], [1.0], kernel=_native.KERNEL_ADJOINT, entry="hipsoxr_run_device_vr_ragged")
    assert got and "variable-rate ragged batch: served by the exact engine alone" in got
    with pytest.raises(RuntimeError, match=r"variable-rate plans are not served \(HIPSOXR_KERNEL_ADJOINT takes constant-rate plans\)"):
        vr.run_adjoint(None, None, _native.F32, 1, 1, 90, 100, (0, 1, 1), (0, 1, 1), kernel=_native.KERNEL_ADJOINT)
    for k in (_native.KERNEL_AUTO, _native.KERNEL_ADJOINT):
        with pytest.raises(RuntimeError, match=r"variable-rate plans are not served \(ragged batches take constant-rate plans\)"):
            vr.run_adjoint_ragged(None, None, _native.F32, 1, [[0, 90, 0, 100]], (1, 1), (1, 1), kernel=k)
