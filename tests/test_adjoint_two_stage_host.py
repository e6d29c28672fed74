"""Host side of the two-stage form's adjoint (no GPU): the selector HIPSOXR_KERNEL_ADJOINT_TWO_STAGE is declared and bound, the
Python surface takes it, jobs without a device decide every refusal by name before anything touches one, the forward entry
and the ragged entry refuse it, and the other selectors answer an interpolated-phase plan with the words they had."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = (0, 0, 0)
NAME = r"^adjoint job: HIPSOXR_KERNEL_ADJOINT_TWO_STAGE"


def test_header_defines_the_selector_and_keeps_the_others():
    with open(os.path.join(ROOT, "include", "hipsoxr.h")) as f:
        text = f.read()
    assert re.search(r"\bHIPSOXR_KERNEL_ADJOINT_TWO_STAGE\s*=\s*12\b", text)
    assert re.search(r"\bHIPSOXR_KERNEL_ADJOINT_FFT\s*=\s*11\b", text) and re.search(r"\bHIPSOXR_KERNEL_ADJOINT\s*=\s*10\b", text)
    assert '#define HIPSOXR_VERSION_STRING "0.7.0"' in text  # no field was added to hipsoxr_job_t, no entry exported


def test_python_binds_the_selector():
    from soxr_amd import _native, device as dev, dist
    assert _native.KERNEL_ADJOINT_TWO_STAGE == 12 and dev.KERNEL_ADJOINT_TWO_STAGE == 12
    assert (_native.KERNEL_AUTO, _native.KERNEL_EXACT, _native.KERNEL_ADJOINT, _native.KERNEL_ADJOINT_FFT) == (0, 6, 10, 11)
    # the defaults change nothing
    assert inspect.signature(dev.resample_tensor_adjoint).parameters["kernel"].default == _native.KERNEL_AUTO
    assert inspect.signature(dev.resample_tensor).parameters["grad_kernel"].default == _native.KERNEL_AUTO
    assert inspect.signature(dist.resample_ragged_adjoint).parameters["kernel"].default == _native.KERNEL_AUTO
    assert inspect.signature(dist.resample_ragged).parameters["grad_kernel"].default == _native.KERNEL_AUTO
    # the adjoint's own backward is the two-stage forward: AUTO
    assert dev._adjoint_forward_kernel(_native.KERNEL_ADJOINT_TWO_STAGE) == _native.KERNEL_AUTO
    assert dev._adjoint_forward_kernel(_native.KERNEL_ADJOINT_FFT) == _native.KERNEL_FFT
    for k in (_native.KERNEL_AUTO, _native.KERNEL_EXACT, _native.KERNEL_ADJOINT):
        assert dev._adjoint_forward_kernel(k) == _native.KERNEL_EXACT
    for fn in (dev.resample_tensor_adjoint, dev.resample_tensor, dist.resample_ragged_adjoint, dist.resample_ragged):
        assert "KERNEL_ADJOINT_TWO_STAGE" in fn.__doc__, fn.__name__


def _refusal(plan, elem=None, kernel=None, n_clips=0, gy_frames=0, gx_frames=0, **kw):
    from soxr_amd import _native
    try:
        plan.run_adjoint(None, None, _native.F32 if elem is None else elem, n_clips, 1, gy_frames, gx_frames, Z, Z,
                         kernel=_native.KERNEL_ADJOINT_TWO_STAGE if kernel is None else kernel, **kw)
    except RuntimeError as e:
        return str(e)
    return None


def test_jobs_without_a_device_decide_the_refusals():
    from soxr_amd import _native as n, device as dev
    hq, vhq = dev.Plan(48000, 44101, "HQ"), dev.Plan(44101, 48000, "VHQ")
    assert hq.phases and vhq.phases
    for plan in (hq, vhq):  # empty job: success, nothing launched — float32 / float64, and the half types (widened)
        for elem in (n.F32, n.F64, n.F16, n.BF16):
            assert _refusal(plan, elem) is None
    for elem in (n.I16, n.I32):
        assert re.search(NAME + r" serves float32 or float64 elements \(integer types have no gradient\)$", _refusal(hq, elem))
    vr = dev.Plan(48000, 44100, "HQ", vr=True)
    assert re.search(NAME + r": variable-rate plans are not served$", _refusal(vr))
    exact = dev.Plan(48000, 44100, "VHQ")
    assert not exact.phases
    assert re.search(NAME + r" needs an interpolated-phase plan \(exact-bank plans are served by HIPSOXR_KERNEL_ADJOINT_FFT,", _refusal(exact))
    table = np.zeros((1, 4), np.int64)
    assert re.search(NAME + r": a clip_table is not served on this entry", _refusal(hq, clip_table=table.ctypes.data))
    # the order: the element type before the plan kind, variable rate before the bank
    assert "float32 or float64" in _refusal(vr, n.I16) and "float32 or float64" in _refusal(exact, n.I32)
    # the length rule is the exact adjoint's own (adj_extent_refusal), on the FORWARD plan
    assert _refusal(hq, n_clips=1, gy_frames=hq.out_len(9000) + 1, gx_frames=9000) == \
        _refusal(hq, kernel=n.KERNEL_ADJOINT, n_clips=1, gy_frames=hq.out_len(9000) + 1, gx_frames=9000)
    assert re.search(r"^adjoint job: .*exceeds", _refusal(hq, n_clips=1, gy_frames=hq.out_len(9000) + 1, gx_frames=9000))
    assert _refusal(hq, n_clips=1, gy_frames=-1, gx_frames=9000) == _refusal(hq, kernel=n.KERNEL_ADJOINT, n_clips=1, gy_frames=-1, gx_frames=9000) != None  # noqa: E711
    # what is left needs buffers and a device: asked last
    assert _refusal(hq, n_clips=1, gy_frames=hq.out_len(9000), gx_frames=9000) == "null buffer"
    for elem in (n.F16, n.BF16):
        assert _refusal(hq, elem, n_clips=1, gy_frames=hq.out_len(9000), gx_frames=9000) == "null buffer"
        assert re.search(NAME + r" needs an interpolated-phase plan", _refusal(exact, elem))


def test_windows_are_refused_by_name():
    import ctypes
    from soxr_amd import _native as n, device as dev
    plan = dev.Plan(48000, 44101, "VHQ")
    for field in ("in_abs0", "out_k0"):
        j = n.Job()
        j.elem, j.kernel, j.n_clips, j.n_channels = n.F32, n.KERNEL_ADJOINT_TWO_STAGE, 1, 1
        j.in_frame_stride = j.out_frame_stride = j.in_chan_stride = j.out_chan_stride = 1
        j.in_frames, j.out_frames = plan.out_len(9000), 9000
        setattr(j, field, 3)
        err = n.lib.hipsoxr_run_device_adjoint(plan.handle, ctypes.byref(j), None)
        assert err and re.search(NAME + r": whole cotangents only \(in_abs0 == 0, out_k0 == 0\)$", err.decode()), (field, err)


def test_the_ragged_entry_refuses_the_selector():
    from soxr_amd import _native as n, device as dev, dist
    K = n.KERNEL_ADJOINT_TWO_STAGE
    for plan in (dev.Plan(48000, 44101, "VHQ"), dev.Plan(48000, 44100, "HQ")):
        for rows in ([], [[0, plan.out_len(9000), 0, 9000]]):
            t = np.asarray(rows, np.int64).reshape(-1, 4)
            with pytest.raises(RuntimeError, match=NAME + r": ragged clip tables are not served yet"):
                plan.run_adjoint_ragged(None, None, n.F32, 1, t, (1, 1), (1, 1), kernel=K)
        # ... which is what dist's functions surface when the forward is called
        assert re.search(NAME + r": ragged clip tables are not served yet", dist._ragged_adjoint_refusal(plan, n.F32, K))


def test_the_forward_entry_refuses_the_selector():
    from soxr_amd import _native as n, device as dev
    plan = dev.Plan(48000, 44101, "HQ")
    with pytest.raises(RuntimeError, match=r"^HIPSOXR_KERNEL_ADJOINT_TWO_STAGE selects the transposed two-stage form: it is valid on hipsoxr_run_device_adjoint only"):
        plan.run(None, None, n.F32, 0, 0, 0, 0, Z, Z, kernel=n.KERNEL_ADJOINT_TWO_STAGE)
    # selectors 10 and 11: as they were
    with pytest.raises(RuntimeError, match="HIPSOXR_KERNEL_ADJOINT selects the transposed operator: it is valid on hipsoxr_run_device_adjoint only"):
        plan.run(None, None, n.F32, 0, 0, 0, 0, Z, Z, kernel=n.KERNEL_ADJOINT)
    with pytest.raises(RuntimeError, match="HIPSOXR_KERNEL_ADJOINT_FFT.*hipsoxr_run_device_adjoint and hipsoxr_run_device_adjoint_ragged only"):
        plan.run(None, None, n.F32, 0, 0, 0, 0, Z, Z, kernel=n.KERNEL_ADJOINT_FFT)


def test_the_other_selectors_keep_their_words_on_an_interpolated_phase_plan():
    from soxr_amd import _native as n, device as dev
    interp = dev.Plan(48000, 44101, "VHQ")
    for k in (n.KERNEL_AUTO, n.KERNEL_EXACT):
        assert _refusal(interp, kernel=k) == "adjoint job: needs an exact-bank plan (interpolated-phase plans and the two-stage form are not served)"
    assert _refusal(interp, kernel=n.KERNEL_ADJOINT) is None
    assert _refusal(interp, kernel=n.KERNEL_ADJOINT_FFT) == \
        "adjoint job: HIPSOXR_KERNEL_ADJOINT_FFT needs an exact-bank plan (interpolated-phase plans are served by HIPSOXR_KERNEL_ADJOINT, on the exact engine)"
    assert re.search(r"the kernel selector must be AUTO or EXACT", _refusal(dev.Plan(48000, 44100, "HQ"), kernel=n.KERNEL_FFT))
