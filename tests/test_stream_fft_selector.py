"""HIPSOXR_STREAM_FFT, host side: the flag exists under one value in the C header and the Python binding, collides with
no other stream flag, TensorStream takes `engine`, and the version is the one that has it.  (What the flag computes:
tests/test_gpu_stream_fft.py.)"""
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ("VR", "NO_DITHER", "DEFER", "RESIDENT", "AUTO_RESIDENT", "STREAM_FFT")


def _header():
    with open(os.path.join(ROOT, "include", "hipsoxr.h")) as f:
        return f.read()


def test_header_defines_the_flag_and_it_collides_with_no_other():
    values = {}
    for name in FLAGS:
        m = re.search(r"#define\s+HIPSOXR_%s\s+(\d+)UL" % name, _header())
        assert m, name
        values[name] = int(m.group(1))
    assert values["STREAM_FFT"] == 512
    # nothing that existed changes its value; every flag is one bit of its own
    assert [values[k] for k in FLAGS[:-1]] == [32, 8, 64, 128, 256]
    assert all(v & (v - 1) == 0 for v in values.values()) and len(set(values.values())) == len(values)
    # (recipes share the word with the flags: 0, 1, 2, 4, 6 — below the lowest flag bit)
    assert min(values.values()) > 6


def test_python_binding_exports_the_same_value():
    from soxr_amd import _native
    assert _native.STREAM_FFT == 512
    assert (_native.VR, _native.NO_DITHER, _native.DEFER, _native.RESIDENT, _native.AUTO_RESIDENT) == (32, 8, 64, 128, 256)


def test_tensor_stream_takes_engine():
    from soxr_amd import device
    p = inspect.signature(device.TensorStream.__init__).parameters
    assert "engine" in p and p["engine"].default == "exact"
    # the host-array stream and the grouped launch are unchanged
    import soxr_amd
    assert "engine" not in inspect.signature(soxr_amd.ResampleStream.__init__).parameters
    assert "engine" not in inspect.signature(device.TensorStreamGroup.__init__).parameters
    with pytest.raises(ValueError):
        device.TensorStream(48000, 44100, 1, engine="fast")  # (refused before anything touches a device)


def test_version_is_the_one_that_has_the_flag():
    import soxr_amd
    from soxr_amd import _native
    hdr = re.search(r'#define\s+HIPSOXR_VERSION_STRING\s+"([^"]+)"', _header()).group(1)
    assert hdr == "0.7.0"
    assert _native.version().startswith("hipsoxr-0.7.0")
    assert soxr_amd.__version__ == "0.7.0"
