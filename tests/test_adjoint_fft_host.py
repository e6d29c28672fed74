"""Host side of the adjoint on the frequency-domain engine (no GPU): the selector HIPSOXR_KERNEL_ADJOINT_FFT is declared and
bound, the Python surface takes it, empty jobs decide its refusals before anything touches a device, and the forward entries
refuse it by name."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = (0, 0, 0)


def test_header_defines_the_selector_and_keeps_the_version():
    with open(os.path.join(ROOT, "include", "hipsoxr.h")) as f:
        text = f.read()
    assert re.search(r"\bHIPSOXR_KERNEL_ADJOINT_FFT\s*=\s*11\b", text)
    assert re.search(r"\bHIPSOXR_KERNEL_ADJOINT\s*=\s*10\b", text)
    assert '#define HIPSOXR_VERSION_STRING "0.7.0"' in text  # no field was added to hipsoxr_job_t, no entry exported
    assert "no new field — the selector HIPSOXR_KERNEL_ADJOINT_FFT" in text


def test_python_binds_the_selector():
    from soxr_amd import _native, device as dev, dist
    assert _native.KERNEL_ADJOINT_FFT == 11 and dev.KERNEL_ADJOINT_FFT == 11
    assert _native.version().startswith("hipsoxr-0.7.0")
    # the defaults change nothing
    assert inspect.signature(dev.resample_tensor_adjoint).parameters["kernel"].default == _native.KERNEL_AUTO
    assert inspect.signature(dev.resample_tensor).parameters["grad_kernel"].default == _native.KERNEL_AUTO
    assert inspect.signature(dist.resample_ragged_adjoint).parameters["kernel"].default == _native.KERNEL_AUTO
    assert inspect.signature(dist.resample_ragged).parameters["grad_kernel"].default == _native.KERNEL_AUTO
    # the adjoint's own backward: the forward on the engine the adjoint ran on
    assert dev._adjoint_forward_kernel(_native.KERNEL_ADJOINT_FFT) == _native.KERNEL_FFT
    for k in (_native.KERNEL_AUTO, _native.KERNEL_EXACT, _native.KERNEL_ADJOINT):
        assert dev._adjoint_forward_kernel(k) == _native.KERNEL_EXACT


def _refusal(plan, elem=None, kernel=None, n_clips=0, gy_frames=0, gx_frames=0, **kw):
    from soxr_amd import _native
    try:
        plan.run_adjoint(None, None, _native.F32 if elem is None else elem, n_clips, 1, gy_frames, gx_frames, Z, Z,
                         kernel=_native.KERNEL_ADJOINT_FFT if kernel is None else kernel, **kw)
    except RuntimeError as e:
        return str(e)
    return None


def test_empty_jobs_decide_the_refusals():
    from soxr_amd import _native as n, device as dev
    hq, vhq = dev.Plan(48000, 44100, "HQ"), dev.Plan(44100, 16000, "VHQ")
    for plan in (hq, vhq):  # empty job: success, nothing launched — float32 / float64, and the half types (widened)
        for elem in (n.F32, n.F64, n.F16, n.BF16):
            assert _refusal(plan, elem) is None
    for elem in (n.I16, n.I32):
        assert re.search(r"ADJOINT_FFT serves float32 or float64", _refusal(hq, elem))
    vr, interp = dev.Plan(48000, 44100, "HQ", vr=True), dev.Plan(48000, 44101, "HQ")
    assert re.search(r"ADJOINT_FFT: variable-rate plans are not served", _refusal(vr))
    assert re.search(r"ADJOINT_FFT needs an exact-bank plan .*HIPSOXR_KERNEL_ADJOINT,", _refusal(interp))
    for q in ("MQ", "LQ", "QQ"):
        assert re.search(r"ADJOINT_FFT: .*HQ and VHQ only .*120 dB", _refusal(dev.Plan(48000, 44100, q))), q
    table = np.zeros((1, 4), np.int64)
    assert re.search(r"ADJOINT_FFT: a clip_table is served by hipsoxr_run_device_adjoint_ragged", _refusal(hq, clip_table=table.ctypes.data))
    # the order: the element type before the plan, the plan before the recipe
    assert "float32 or float64" in _refusal(vr, n.I16) and "variable-rate" in _refusal(dev.Plan(48000, 44100, "MQ", vr=True))
    # the length rule is the FORWARD plan's, as for every adjoint job
    assert re.search(r"adjoint job: .*exceeds", _refusal(hq, n_clips=1, gy_frames=hq.out_len(100) + 1, gx_frames=100))
    assert _refusal(hq, n_clips=1, gy_frames=hq.out_len(100), gx_frames=100) == "null buffer"
    # AUTO, EXACT and ADJOINT keep their words
    assert re.search(r"adjoint job: .*exact-bank plan \(interpolated-phase plans and the two-stage form are not served\)", _refusal(interp, kernel=n.KERNEL_AUTO))
    assert re.search(r"the kernel selector must be AUTO or EXACT", _refusal(hq, kernel=n.KERNEL_FFT))
    assert _refusal(interp, kernel=n.KERNEL_ADJOINT) is None


def test_the_ragged_entry():
    from soxr_amd import _native as n, device as dev
    K = n.KERNEL_ADJOINT_FFT
    hq = dev.Plan(48000, 44100, "HQ")

    def call(plan, rows, elem=n.F32, table=True, **kw):
        t = np.asarray(rows, np.int64).reshape(-1, 4)
        try:
            if table:
                plan.run_adjoint_ragged(None, None, elem, 1, t, (1, 1), (1, 1), kernel=K, **kw)
            else:  # the ragged entry without a table: a raw job
                import ctypes
                j = n.Job()
                j.elem, j.kernel, j.n_clips, j.n_channels = elem, K, 0, 1
                n.check(n.lib.hipsoxr_run_device_adjoint_ragged(plan.handle, ctypes.byref(j), None))
        except RuntimeError as e:
            return str(e)
        return None

    assert call(hq, []) is None and call(hq, [[0, 0, 0, 0]]) is None  # no clips; a clip without frames
    assert call(hq, [[0, hq.out_len(500), 0, 500]]) == "null buffer"
    assert re.search(r"ADJOINT_FFT: the ragged entry needs a clip_table", call(hq, [], table=False))
    for elem in (n.F16, n.BF16):
        assert re.search(r"ADJOINT_FFT: ragged: float16 / bfloat16 clip tables are not served", call(hq, [], elem))
    assert re.search(r"ADJOINT_FFT serves float32 or float64", call(hq, [], n.I32))
    assert re.search(r"ADJOINT_FFT: .*HQ and VHQ only", call(dev.Plan(48000, 44100, "MQ"), []))
    assert re.search(r"ADJOINT_FFT needs an exact-bank plan", call(dev.Plan(48000, 44101, "VHQ"), []))
    assert re.search(r"ragged: a clip's n_y .*exceeds the plan's output length", call(hq, [[0, hq.out_len(500) + 1, 0, 500]]))
    assert re.search(r"ragged: a clip's offset or frame count is negative", call(hq, [[0, 1, -1, 5]]))


def test_the_forward_entries_refuse_the_selector():
    from soxr_amd import _native as n, device as dev
    K = n.KERNEL_ADJOINT_FFT
    plan = dev.Plan(48000, 44100, "HQ")
    with pytest.raises(RuntimeError, match="HIPSOXR_KERNEL_ADJOINT_FFT.*hipsoxr_run_device_adjoint and hipsoxr_run_device_adjoint_ragged only"):
        plan.run(None, None, n.F32, 0, 0, 0, 0, Z, Z, kernel=K)
    with pytest.raises(RuntimeError, match="HIPSOXR_KERNEL_ADJOINT.*hipsoxr_run_device_adjoint only"):  # selector 10: as it was
        plan.run(None, None, n.F32, 0, 0, 0, 0, Z, Z, kernel=n.KERNEL_ADJOINT)
    vr = dev.Plan(48000, 44100, "HQ", vr=True)
    table = np.array([[0, 100, 0, 50]], np.int64)
    with pytest.raises(RuntimeError, match="variable-rate ragged batch: served by the exact engine alone"):
        vr.run_vr_ragged(None, None, n.F32, 1, table, [1.0], (1, 1), (1, 1), kernel=K)
