"""Host side of the adjoint of interpolated-phase plans (no GPU): the selector HIPSOXR_KERNEL_ADJOINT is declared and bound,
the Python surface takes it, and empty jobs decide its refusals before anything touches a device."""
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_defines_the_selector_and_keeps_the_version():
    with open(os.path.join(ROOT, "include", "hipsoxr.h")) as f:
        text = f.read()
    assert re.search(r"\bHIPSOXR_KERNEL_ADJOINT\s*=\s*10\b", text)
    assert '#define HIPSOXR_VERSION_STRING "0.7.0"' in text  # no field was added to hipsoxr_job_t
    assert "no new field — the selector HIPSOXR_KERNEL_ADJOINT" in text


def test_python_binds_the_selector():
    from soxr_amd import _native, device as dev
    assert _native.KERNEL_ADJOINT == 10 and dev.KERNEL_ADJOINT == 10
    assert _native.version().startswith("hipsoxr-0.7.0")
    assert inspect.signature(dev.resample_tensor_adjoint).parameters["kernel"].default == _native.KERNEL_AUTO
    assert inspect.signature(dev.resample_tensor).parameters["grad_kernel"].default == _native.KERNEL_AUTO
    assert inspect.signature(dev.resample_tensor).parameters["kernel"].default == _native.KERNEL_AUTO


def test_tile_constant_is_the_kernel_s():
    """_native.ADJOINT_INTERP_TILE is what tests place tile edges by: it is csrc/adjoint.hip's kAdjIW."""
    from soxr_amd import _native
    with open(os.path.join(ROOT, "python-soxr_amd", "csrc", "adjoint.hip")) as f:
        m = re.search(r"constexpr\s+int\s+kAdjIW\s*=\s*(\d+)\s*;", f.read())
    assert m and int(m.group(1)) == _native.ADJOINT_INTERP_TILE


def test_empty_jobs_decide_the_refusals():
    from soxr_amd import _native, device as dev
    K = _native.KERNEL_ADJOINT
    exact, interp, vr = dev.Plan(48000, 44100, "HQ"), dev.Plan(48000, 44101, "HQ"), dev.Plan(48000, 44100, "HQ", vr=True)
    assert interp.phases and vr.phases and not exact.phases
    z = (0, 0, 0)
    for plan in (interp, exact):  # empty job: success, nothing launched
        for elem in (_native.F32, _native.F64):
            plan.run_adjoint(None, None, elem, 0, 0, 0, 0, z, z, kernel=K)
    for plan in (interp, exact):
        for elem in (_native.I16, _native.I32):
            with pytest.raises(RuntimeError, match="adjoint job: .*float32 or float64"):
                plan.run_adjoint(None, None, elem, 0, 0, 0, 0, z, z, kernel=K)
        with pytest.raises(RuntimeError, match="adjoint job: .*exceeds"):
            plan.run_adjoint(None, None, _native.F32, 1, 1, plan.out_len(100) + 1, 100, z, z, kernel=K)
    with pytest.raises(RuntimeError, match="adjoint job: .*variable-rate"):
        vr.run_adjoint(None, None, _native.F32, 0, 0, 0, 0, z, z, kernel=K)
    # the defaults keep their refusal of an interpolated-phase plan, word for word
    for kernel in (_native.KERNEL_AUTO, _native.KERNEL_EXACT):
        with pytest.raises(RuntimeError, match="adjoint job: .*exact-bank"):
            interp.run_adjoint(None, None, _native.F32, 0, 0, 0, 0, z, z, kernel=kernel)
    # and the forward entry does not know the selector
    with pytest.raises(RuntimeError, match="HIPSOXR_KERNEL_ADJOINT.*hipsoxr_run_device_adjoint only"):
        interp.run(None, None, _native.F32, 0, 0, 0, 0, z, z, kernel=K)
