"""HIPSOXR_KERNEL_FFT_PCM, host side: the selector exists under one number in the C header and both Python modules,
and the device entry points take a dither seed.  (What the selector computes: tests/test_gpu_fft_pcm.py.)"""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "hipsoxr.h")) as f:
        return f.read()


def test_header_defines_the_selector():
    enum = re.search(r"typedef enum \{([^}]*)\} hipsoxr_kernel_t;", _header(), re.S).group(1)
    values = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"(HIPSOXR_KERNEL_\w+)\s*=\s*(\d+)", enum))
    assert values["HIPSOXR_KERNEL_FFT_PCM"] == 9
    # nothing that existed changes its number
    assert [values[k] for k in ("HIPSOXR_KERNEL_AUTO", "HIPSOXR_KERNEL_FFT", "HIPSOXR_KERNEL_EXACT", "HIPSOXR_KERNEL_FFT_F64")] == [0, 5, 6, 8]
    assert len(set(values.values())) == len(values) == 10


def test_python_modules_export_the_selector():
    from soxr_amd import _native, device
    assert _native.KERNEL_FFT_PCM == 9
    assert device.KERNEL_FFT_PCM == 9
    assert (_native.KERNEL_AUTO, _native.KERNEL_FFT, _native.KERNEL_EXACT, _native.KERNEL_FFT_F64) == (0, 5, 6, 8)


def test_device_entry_points_take_a_dither_seed():
    from soxr_amd import device, dist
    for fn in (device.resample_tensor, device.PreparedJob.__init__, dist.RaggedJob.__init__):
        p = inspect.signature(fn).parameters
        assert "dither_seed" in p and p["dither_seed"].default == 0, fn
    assert "clip_counter" in inspect.signature(dist.RaggedJob.__init__).parameters


def test_library_reports_the_version_that_has_the_selector():
    from soxr_amd import _native
    major, minor = (int(v) for v in re.search(r"hipsoxr-(\d+)\.(\d+)", _native.version()).groups())
    assert (major, minor) >= (0, 6)
