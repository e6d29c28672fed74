"""Host side of HIPSOXR_KERNEL_ADJOINT_AUTO (no GPU): the selector is 13 in the header and in Python, the Python surface takes it
and documents it, the forward entry refuses it by name, and on both adjoint entries a job without a device is refused exactly
where HIPSOXR_KERNEL_ADJOINT refuses it — under the selector's own name — and passes (the empty job) or reaches "null buffer"
exactly where that selector does."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = (0, 0, 0)
NAME = r"^adjoint job: HIPSOXR_KERNEL_ADJOINT_AUTO"


def test_header_defines_the_selector_and_keeps_the_others():
    with open(os.path.join(ROOT, "include", "hipsoxr.h")) as f:
        text = f.read()
    assert re.search(r"\bHIPSOXR_KERNEL_ADJOINT_AUTO\s*=\s*13\b", text)
    assert re.search(r"\bHIPSOXR_KERNEL_ADJOINT_TWO_STAGE\s*=\s*12\b", text) and re.search(r"\bHIPSOXR_KERNEL_ADJOINT_FFT\s*=\s*11\b", text)
    assert re.search(r"\bHIPSOXR_KERNEL_ADJOINT\s*=\s*10\b", text)
    assert '#define HIPSOXR_VERSION_STRING "0.7.0"' in text  # no field was added to hipsoxr_job_t, no entry exported


def test_python_binds_and_documents_the_selector():
    from soxr_amd import _native, device as dev, dist
    assert _native.KERNEL_ADJOINT_AUTO == 13 and dev.KERNEL_ADJOINT_AUTO == 13
    assert (_native.KERNEL_AUTO, _native.KERNEL_EXACT, _native.KERNEL_ADJOINT, _native.KERNEL_ADJOINT_FFT, _native.KERNEL_ADJOINT_TWO_STAGE) == (0, 6, 10, 11, 12)
    # the defaults change nothing
    assert inspect.signature(dev.resample_tensor_adjoint).parameters["kernel"].default == _native.KERNEL_AUTO
    assert inspect.signature(dev.resample_tensor).parameters["grad_kernel"].default == _native.KERNEL_AUTO
    assert inspect.signature(dist.resample_ragged_adjoint).parameters["kernel"].default == _native.KERNEL_AUTO
    assert inspect.signature(dist.resample_ragged).parameters["grad_kernel"].default == _native.KERNEL_AUTO
    # the adjoint's own backward is the forward it transposes: AUTO
    assert dev._adjoint_forward_kernel(_native.KERNEL_ADJOINT_AUTO) == _native.KERNEL_AUTO
    assert dev._adjoint_forward_kernel(_native.KERNEL_ADJOINT_TWO_STAGE) == _native.KERNEL_AUTO
    assert dev._adjoint_forward_kernel(_native.KERNEL_ADJOINT_FFT) == _native.KERNEL_FFT
    assert dev._adjoint_forward_kernel(_native.KERNEL_ADJOINT) == _native.KERNEL_EXACT
    for fn in (dev.resample_tensor_adjoint, dev.resample_tensor, dist.resample_ragged_adjoint, dist.resample_ragged):
        doc = " ".join(fn.__doc__.split())
        assert "KERNEL_ADJOINT_AUTO" in doc, fn.__name__
        said = doc[doc.index("KERNEL_ADJOINT_AUTO"):]
        # ... and what it resolves to
        assert "KERNEL_ADJOINT_FFT" in said or "two-stage" in said, fn.__name__
        assert "exact adjoint" in said, fn.__name__


def _equal(plan, kernel, elem=None, n_clips=0, gy_frames=0, gx_frames=0, **kw):
    from soxr_amd import _native
    try:
        plan.run_adjoint(None, None, _native.F32 if elem is None else elem, n_clips, 1, gy_frames, gx_frames, Z, Z, kernel=kernel, **kw)
    except RuntimeError as e:
        return str(e)
    return None


def _ragged(plan, kernel, rows, elem=None):
    from soxr_amd import _native
    try:
        plan.run_adjoint_ragged(None, None, _native.F32 if elem is None else elem, 1, np.asarray(rows, np.int64).reshape(-1, 4), (1, 1), (1, 1), kernel=kernel)
    except RuntimeError as e:
        return str(e)
    return None


def _plans():
    from soxr_amd import device as dev
    return {"exact VHQ": dev.Plan(48000, 44100, "VHQ"), "exact MQ": dev.Plan(48000, 44100, "MQ"), "interp VHQ": dev.Plan(48000, 44101, "VHQ"),
            "interp MQ": dev.Plan(44101, 48000, "MQ"), "vr": dev.Plan(48000, 44100, "HQ", vr=True)}


def test_the_equal_length_entry_refuses_what_kernel_adjoint_refuses():
    from soxr_amd import _native as n
    A, K = n.KERNEL_ADJOINT, n.KERNEL_ADJOINT_AUTO
    table = np.zeros((1, 4), np.int64)
    seen = set()
    for name, plan in _plans().items():
        for elem in (n.F32, n.F64, n.F16, n.BF16, n.I16, n.I32):
            for kw in ({}, {"clip_table": table.ctypes.data}, {"n_clips": 1, "gy_frames": plan.out_len(9000) + 1, "gx_frames": 9000},
                       {"n_clips": 1, "gy_frames": -1, "gx_frames": 9000}, {"n_clips": 1, "gy_frames": plan.out_len(9000), "gx_frames": 9000}):
                by_name, auto = _equal(plan, A, elem, **kw), _equal(plan, K, elem, **kw)
                assert (by_name is None) == (auto is None), (name, elem, kw, by_name, auto)
                if auto is None:
                    seen.add("served")
                elif auto == "null buffer" or "exceeds" in auto or "invalid job extent" in auto:
                    assert auto == by_name, (name, elem, kw)  # the length rule and the last question are the exact adjoint's own
                    seen.add("null buffer" if auto == "null buffer" else "extent")
                else:
                    assert re.search(NAME, auto), (name, elem, kw, auto)
                    seen.add("by name")
    assert seen == {"served", "by name", "null buffer", "extent"}, seen
    p = _plans()
    assert re.search(NAME + r" serves float32 or float64 elements \(integer types have no gradient\)$", _equal(p["interp VHQ"], K, n.I16))
    assert re.search(NAME + r": variable-rate plans are not served$", _equal(p["vr"], K))
    assert re.search(NAME + r": a clip_table is served by hipsoxr_run_device_adjoint_ragged, not by this entry$", _equal(p["exact VHQ"], K, clip_table=table.ctypes.data))
    # every plan kind and recipe is served: the empty job succeeds where the named fast selectors refuse
    for name in ("exact VHQ", "exact MQ", "interp VHQ", "interp MQ"):
        assert _equal(p[name], K) is None and _equal(p[name], K, n.F16) is None, name
    assert _equal(p["interp VHQ"], n.KERNEL_ADJOINT_FFT) is not None and _equal(p["exact VHQ"], n.KERNEL_ADJOINT_TWO_STAGE) is not None


def test_windows_are_refused_by_name():
    import ctypes
    from soxr_amd import _native as n, device as dev
    plan = dev.Plan(48000, 44101, "VHQ")
    for entry in ("hipsoxr_run_device_adjoint", "hipsoxr_run_device_adjoint_ragged"):
        for field in ("in_abs0", "out_k0"):
            j = n.Job()
            j.elem, j.kernel, j.n_clips, j.n_channels = n.F32, n.KERNEL_ADJOINT_AUTO, 1, 1
            j.in_frame_stride = j.out_frame_stride = j.in_chan_stride = j.out_chan_stride = 1
            j.in_frames, j.out_frames = plan.out_len(9000), 9000
            setattr(j, field, 3)
            err = getattr(n.lib, entry)(plan.handle, ctypes.byref(j), None)
            assert err and re.search(NAME + r": whole cotangents only \(in_abs0 == 0, out_k0 == 0\)$", err.decode()), (entry, field, err)


def test_the_ragged_entry_refuses_what_kernel_adjoint_refuses():
    import ctypes
    from soxr_amd import _native as n, dist
    A, K = n.KERNEL_ADJOINT, n.KERNEL_ADJOINT_AUTO
    for name, plan in _plans().items():
        good = [0, plan.out_len(9000), 0, 9000]
        for elem in (n.F32, n.F64, n.F16, n.BF16, n.I16, n.I32):
            for rows in ([], [good], [good, [5, 0, 5, 300], [9, 0, 9, 0]], [[0, plan.out_len(9000) + 1, 0, 9000]], [[0, -1, 0, 9000]], [[-4, 10, 0, 9000]]):
                by_name, auto = _ragged(plan, A, rows, elem), _ragged(plan, K, rows, elem)
                assert (by_name is None) == (auto is None), (name, elem, rows, by_name, auto)
                if auto is not None and not re.search(NAME, auto):
                    assert auto == by_name, (name, elem, rows)  # rows, extent, "null buffer": the exact adjoint's own words
        assert (dist._ragged_adjoint_refusal(plan, n.F32, K) is None) == (dist._ragged_adjoint_refusal(plan, n.F32, A) is None)
    p = _plans()
    assert re.search(NAME + r": ragged: float16 / bfloat16 clip tables are not served", _ragged(p["interp VHQ"], K, [], n.F16))
    assert re.search(NAME + r": variable-rate plans are not served$", _ragged(p["vr"], K, []))
    assert _ragged(p["interp VHQ"], K, []) is None and _ragged(p["exact MQ"], K, []) is None
    assert _ragged(p["interp VHQ"], K, [[0, p["interp VHQ"].out_len(9000), 0, 9000]]) == "null buffer"
    assert "exceeds the plan's output length" in _ragged(p["interp VHQ"], K, [[0, p["interp VHQ"].out_len(9000) + 1, 0, 9000]])
    # no table on the ragged entry
    j = n.Job()
    j.elem, j.kernel, j.n_clips, j.n_channels = n.F32, K, 1, 1
    err = n.lib.hipsoxr_run_device_adjoint_ragged(p["exact VHQ"].handle, ctypes.byref(j), None)
    assert err and re.search(NAME + r": the ragged entry needs a clip_table", err.decode())
    # selector 12 keeps its refusal of the ragged entry
    assert "ragged clip tables are not served yet" in _ragged(p["interp VHQ"], n.KERNEL_ADJOINT_TWO_STAGE, [])


def test_the_forward_entry_refuses_the_selector():
    from soxr_amd import _native as n, device as dev
    for plan in (dev.Plan(48000, 44101, "HQ"), dev.Plan(48000, 44100, "VHQ")):
        with pytest.raises(RuntimeError, match=r"^HIPSOXR_KERNEL_ADJOINT_AUTO selects the transpose of the job HIPSOXR_KERNEL_AUTO launches: it is valid on "
                                               r"hipsoxr_run_device_adjoint and hipsoxr_run_device_adjoint_ragged only"):
            plan.run(None, None, n.F32, 0, 0, 0, 0, Z, Z, kernel=n.KERNEL_ADJOINT_AUTO)
    # selectors 10-12: as they were
    with pytest.raises(RuntimeError, match="HIPSOXR_KERNEL_ADJOINT selects the transposed operator: it is valid on hipsoxr_run_device_adjoint only"):
        plan.run(None, None, n.F32, 0, 0, 0, 0, Z, Z, kernel=n.KERNEL_ADJOINT)
    with pytest.raises(RuntimeError, match="HIPSOXR_KERNEL_ADJOINT_TWO_STAGE selects the transposed two-stage form"):
        plan.run(None, None, n.F32, 0, 0, 0, 0, Z, Z, kernel=n.KERNEL_ADJOINT_TWO_STAGE)


def test_the_defaults_keep_their_words():
    from soxr_amd import _native as n, device as dev
    interp = dev.Plan(48000, 44101, "VHQ")
    for k in (n.KERNEL_AUTO, n.KERNEL_EXACT):
        assert _equal(interp, k) == "adjoint job: needs an exact-bank plan (interpolated-phase plans and the two-stage form are not served)"
    assert re.search(r"the kernel selector must be AUTO or EXACT", _equal(dev.Plan(48000, 44100, "HQ"), n.KERNEL_FFT))
