"""Host side of the ragged adjoint (no GPU): hipsoxr_run_device_adjoint_ragged is declared, exported and bound, the ABI
version has not moved, and every refusal the entry makes by name is returned before a device is asked for — an empty job
or a job of null buffers asks for it.  The equal-length entry still refuses a clip_table."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "hipsoxr_run_device_adjoint_ragged"


def _header():
    with open(os.path.join(ROOT, "include", "hipsoxr.h")) as f:
        return f.read()


def test_header_declares_the_entry():
    text = _header()
    assert re.search(r"HIPSOXR_API\s+hipsoxr_error_t\s+" + ENTRY + r"\s*\(\s*hipsoxr_plan_t\s*\*\s*,"
                     r"\s*const\s+hipsoxr_job_t\s*\*\s*job\s*,\s*void\s*\*\s*hip_stream\s*\)\s*;", text)
    assert "no new field — the entry " + ENTRY in text


def test_version_is_still_0_7_0():
    from soxr_amd import _native
    assert '#define HIPSOXR_VERSION_STRING "0.7.0"' in _header()  # no field was added to hipsoxr_job_t
    assert _native.version().startswith("hipsoxr-0.7.0")


def test_library_exports_the_entry_and_python_binds_it():
    import subprocess
    from soxr_amd import _native, device as dev, dist
    assert ENTRY in _native.SIGNATURES and hasattr(_native.lib, ENTRY)
    assert _native.SIGNATURES[ENTRY] == _native.SIGNATURES["hipsoxr_run_device_adjoint"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True)
    assert re.search(r" T " + ENTRY + r"$", out, re.M)
    assert callable(dev.Plan.run_adjoint_ragged)
    assert callable(dist.resample_ragged_adjoint) and callable(dist.resample_ragged)


def _call(plan, table, elem=None, kernel=0, n_channels=1, in_frames=None, out_frames=None, in_abs0=0, out_k0=0, n_clips=None):
    """The C entry on a job of null buffers: `table` is a list of rows or None (a NULL clip_table).  -> error string / None"""
    from soxr_amd import _native
    j = _native.Job()
    j.elem, j.kernel = _native.F32 if elem is None else elem, kernel
    t = None
    if table is not None:
        t = np.ascontiguousarray(np.array(table, np.int64).reshape(-1, 4))
        keep = t if len(t) else np.zeros((1, 4), np.int64)
        j.clip_table = keep.ctypes.data
    n = len(t) if t is not None else 1
    j.n_clips, j.n_channels = n if n_clips is None else n_clips, n_channels
    j.in_frame_stride = j.out_frame_stride = n_channels
    j.in_chan_stride = j.out_chan_stride = 1
    j.in_abs0, j.out_k0 = in_abs0, out_k0
    j.in_frames = in_frames if in_frames is not None else (int(t[:, 1].max()) if t is not None and len(t) else 0)
    j.out_frames = out_frames if out_frames is not None else (int(t[:, 3].max()) if t is not None and len(t) else 0)
    err = getattr(_native.lib, ENTRY)(plan.handle, C.byref(j), None)
    return err.decode() if err else None


@pytest.fixture(scope="module")
def plans():
    from soxr_amd import device as dev
    exact, interp, vr = dev.Plan(48000, 44100, "HQ"), dev.Plan(48000, 44101, "HQ"), dev.Plan(48000, 44100, "HQ", vr=True)
    assert not exact.phases and interp.phases
    return exact, interp, vr


def test_refusals_by_name_need_no_device(plans):
    from soxr_amd import _native as n
    exact, interp, vr = plans
    ok = [[0, exact.out_len(100), 0, 100], [500, 10, 700, 50]]
    refused = [
        ("clip_table", _call(exact, None)),                                                   # a NULL clip_table
        ("negative", _call(exact, [ok[0], [-1, 10, 700, 50]])),                               # negative gy offset
        ("negative", _call(exact, [ok[0], [500, 10, -7, 50]])),                               # negative gx offset
        ("negative", _call(exact, [ok[0], [500, -1, 700, 50]])),                              # negative n_y
        ("negative", _call(exact, [ok[0], [500, 10, 700, -50]])),                             # negative n_x
        ("above the job's", _call(exact, ok, out_frames=99)),                                 # a row above the job's maxima
        ("above the job's", _call(exact, ok, in_frames=exact.out_len(100) - 1)),
        ("exceeds the plan's output length", _call(exact, [ok[0], [500, exact.out_len(50) + 1, 700, 50]])),
        ("float32 or float64", _call(exact, ok, elem=n.I16)),                                 # integer types
        ("float32 or float64", _call(exact, ok, elem=n.I32)),
        ("whole signals", _call(exact, ok, in_abs0=1)),                                       # windows
        ("whole signals", _call(exact, ok, out_k0=1)),
        ("variable-rate", _call(vr, ok)),                                                     # variable-rate plans
        ("variable-rate", _call(vr, ok, kernel=n.KERNEL_ADJOINT)),
        ("AUTO or EXACT", _call(exact, ok, kernel=n.KERNEL_FFT)),                             # any other selector
        ("AUTO or EXACT", _call(exact, ok, kernel=n.KERNEL_TILE)),
        ("AUTO or EXACT", _call(exact, ok, kernel=n.KERNEL_FFT_PCM)),
        ("exact-bank", _call(interp, ok)),                                                    # interpolated plans: by name only
        ("exact-bank", _call(interp, ok, kernel=n.KERNEL_EXACT)),
    ]
    for word, err in refused:
        assert err is not None and err.startswith("adjoint job: ") and word in err, (word, err)
    # a served job gets as far as the buffers (null here), i.e. past every refusal by name
    assert _call(exact, ok) == "null buffer"
    assert _call(exact, ok, kernel=n.KERNEL_EXACT) == "null buffer"
    assert _call(interp, ok, kernel=n.KERNEL_ADJOINT) == "null buffer"
    assert _call(exact, ok, kernel=n.KERNEL_ADJOINT, elem=n.F64, n_channels=3) == "null buffer"


def test_empty_jobs_succeed_with_nothing_launched(plans):
    from soxr_amd import _native as n
    exact, interp, _ = plans
    assert _call(exact, []) is None                                            # no clips
    assert _call(exact, [[0, 0, 0, 100]], n_channels=0) is None                # no channels
    assert _call(exact, [[0, 0, 0, 0], [0, 0, 0, 0]]) is None                  # the largest n_x is 0
    assert _call(interp, [], kernel=n.KERNEL_ADJOINT, elem=n.F64) is None
    z = np.zeros((0, 4), np.int64)
    exact.run_adjoint_ragged(None, None, n.F32, 0, z, (0, 0), (0, 0))          # the Python launcher, the same
    with pytest.raises(RuntimeError, match="adjoint job: .*exact-bank"):
        interp.run_adjoint_ragged(None, None, n.F32, 1, z, (1, 1), (1, 1))
    with pytest.raises(RuntimeError, match="adjoint job: .*float32 or float64"):
        exact.run_adjoint_ragged(None, None, n.I16, 1, z, (1, 1), (1, 1))


def test_the_equal_length_entry_still_refuses_a_clip_table(plans):
    from soxr_amd import _native as n
    exact = plans[0]
    table = np.array([0, exact.out_len(100), 0, 100], np.int64)
    z = (0, 1, 1)
    with pytest.raises(RuntimeError, match="adjoint job: .*ragged") as e:
        exact.run_adjoint(None, None, n.F32, 1, 1, exact.out_len(100), 100, z, z, clip_table=table.ctypes.data)
    assert ENTRY in str(e.value)  # ... and names the entry that serves it


def test_cpu_tensors_are_refused(plans):
    import torch
    from soxr_amd import dist
    exact = plans[0]
    with pytest.raises(RuntimeError, match="needs a device tensor"):
        dist.resample_ragged_adjoint(exact, [torch.zeros(10), torch.zeros(5)], [11, 6])
    with pytest.raises(ValueError):
        dist.resample_ragged_adjoint(exact, [torch.zeros(10)], [11, 6])
