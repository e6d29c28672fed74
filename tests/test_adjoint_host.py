"""Host side of the differentiable resample_tensor (no GPU): the C entry is declared, the Python surface exists, and a
CPU tensor is refused the way resample_tensor refuses it."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_adjoint_entry():
    with open(os.path.join(ROOT, "include", "hipsoxr.h")) as f:
        text = f.read()
    assert re.search(r"HIPSOXR_API\s+hipsoxr_error_t\s+hipsoxr_run_device_adjoint\s*\(\s*hipsoxr_plan_t\s*\*\s*,"
                     r"\s*const\s+hipsoxr_job_t\s*\*\s*job\s*,\s*void\s*\*\s*hip_stream\s*\)\s*;", text)
    assert '#define HIPSOXR_VERSION_STRING "0.7.0"' in text  # no field was added to hipsoxr_job_t


def test_library_exports_the_adjoint_entry():
    from soxr_amd import _native
    assert "hipsoxr_run_device_adjoint" in _native.SIGNATURES
    assert hasattr(_native.lib, "hipsoxr_run_device_adjoint")


def test_python_surface_exists():
    from soxr_amd import device as dev
    assert callable(dev.resample_tensor_adjoint)
    assert callable(dev.Plan.run_adjoint)


def test_cpu_tensor_is_refused_like_resample_tensor():
    import torch
    from soxr_amd import device as dev
    plan = dev.Plan(2, 1, "LQ")
    with pytest.raises(RuntimeError) as fwd:
        dev.resample_tensor(plan, torch.zeros(64))
    assert "needs a device tensor" in str(fwd.value)
    with pytest.raises(RuntimeError) as adj:
        dev.resample_tensor_adjoint(plan, torch.zeros(32), 64)
    assert str(adj.value) == str(fwd.value)
    with pytest.raises(RuntimeError) as req:  # requires_grad changes nothing about it
        dev.resample_tensor(plan, torch.zeros(64, requires_grad=True))
    assert str(req.value) == str(fwd.value)


def test_refusals_need_no_device():
    """The refusals by name are decided before anything touches a device: an empty job asks for them."""
    from soxr_amd import _native, device as dev
    exact, interp = dev.Plan(48000, 44100, "HQ"), dev.Plan(44100, 48001, "HQ")
    assert interp.phases and not exact.phases
    z = (0, 0, 0)
    exact.run_adjoint(None, None, _native.F32, 0, 0, 0, 0, z, z)  # empty job: success, nothing launched
    exact.run_adjoint(None, None, _native.F64, 0, 0, 0, 0, z, z, kernel=_native.KERNEL_EXACT)
    for plan, elem, kw, word in ((interp, _native.F32, {}, "exact-bank"), (exact, _native.I16, {}, "float32 or float64"),
                                 (exact, _native.I32, {}, "float32 or float64"),
                                 (exact, _native.F32, {"kernel": _native.KERNEL_FFT}, "AUTO or EXACT"),
                                 (exact, _native.F64, {"kernel": _native.KERNEL_TILE}, "AUTO or EXACT")):
        with pytest.raises(RuntimeError, match="adjoint job: .*" + word):
            plan.run_adjoint(None, None, elem, 0, 0, 0, 0, z, z, **kw)
    with pytest.raises(RuntimeError, match="adjoint job: .*exceeds"):
        exact.run_adjoint(None, None, _native.F32, 1, 1, exact.out_len(100) + 1, 100, z, z)
