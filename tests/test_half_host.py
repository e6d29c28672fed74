"""Host side of float16 / bfloat16 device jobs (no GPU): the header has the two element types and no new version, the
binding exposes them, the refusals by name are decided before anything touches a device, and the host surface stays
refused."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "hipsoxr.h")) as f:
        return f.read()


def test_header_has_the_two_enumerators():
    text = _header()
    enum = re.search(r"typedef enum \{([^}]*)\}\s*hipsoxr_elem_t;", text, re.S)
    assert enum, "hipsoxr_elem_t not found"
    body = re.sub(r"/\*.*?\*/", "", enum.group(1), flags=re.S)
    values = dict((k, int(v)) for k, v in re.findall(r"(HIPSOXR_\w+)\s*=\s*(\d+)", body))
    assert values == {"HIPSOXR_F32": 0, "HIPSOXR_F64": 1, "HIPSOXR_I32": 2, "HIPSOXR_I16": 3, "HIPSOXR_F16": 4, "HIPSOXR_BF16": 5}


def test_version_is_still_0_7_0():
    assert '#define HIPSOXR_VERSION_STRING "0.7.0"' in _header()  # no field was added to hipsoxr_job_t
    assert "no new field — the element types HIPSOXR_F16 / HIPSOXR_BF16" in _header()
    from soxr_amd import _native
    assert _native.version().startswith("hipsoxr-0.7.0")


def test_native_exposes_the_element_types():
    from soxr_amd import _native
    assert (_native.F32, _native.F64, _native.I32, _native.I16, _native.F16, _native.BF16) == (0, 1, 2, 3, 4, 5)


def test_job_and_stream_forms_of_the_dtype_map():
    import torch
    from soxr_amd import _native, device as dev
    assert dev._torch_elem(torch.float16) == _native.F16 and dev._torch_elem(torch.bfloat16) == _native.BF16
    for dt in (torch.float32, torch.float64, torch.int32, torch.int16):
        assert dev._torch_stream_elem(dt) == dev._torch_elem(dt)
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match=r"float32, float64, int16, int32, float16, bfloat16.*streams take four"):
            dev._torch_stream_elem(dt)
    with pytest.raises(TypeError, match="float16, bfloat16"):
        dev._torch_elem(torch.int8)


def test_empty_half_adjoint_job_succeeds_and_the_ragged_entry_names_its_refusal():
    """Asked with empty jobs, as resample_tensor asks before it builds a graph: no device is needed."""
    from soxr_amd import _native, device as dev
    exact, interp = dev.Plan(48000, 44100, "HQ"), dev.Plan(44100, 48001, "HQ")
    z = (0, 0, 0)
    for elem in (_native.F16, _native.BF16):
        exact.run_adjoint(None, None, elem, 0, 0, 0, 0, z, z)
        exact.run_adjoint(None, None, elem, 0, 0, 0, 0, z, z, kernel=_native.KERNEL_EXACT)
        interp.run_adjoint(None, None, elem, 0, 0, 0, 0, z, z, kernel=_native.KERNEL_ADJOINT)
        assert dev._adjoint_refusal(exact, elem) is None
        # ... and what a float32 job is refused, a half job is refused in the same words
        with pytest.raises(RuntimeError, match="adjoint job: .*exact-bank"):
            interp.run_adjoint(None, None, elem, 0, 0, 0, 0, z, z)
        with pytest.raises(RuntimeError, match="adjoint job: .*AUTO or EXACT"):
            exact.run_adjoint(None, None, elem, 0, 0, 0, 0, z, z, kernel=_native.KERNEL_FFT)
        with pytest.raises(RuntimeError, match="adjoint job: .*exceeds"):
            exact.run_adjoint(None, None, elem, 1, 1, exact.out_len(100) + 1, 100, z, z)
        with pytest.raises(RuntimeError, match="adjoint job: ragged: float16 / bfloat16 clip tables are not served"):
            exact.run_adjoint_ragged(None, None, elem, 0, np.zeros((0, 4), np.int64), (0, 0), (0, 0))


def test_element_types_above_bf16_stay_invalid():
    from soxr_amd import _native, device as dev
    plan = dev.Plan(48000, 44100, "HQ")
    for elem in (6, 7, -1):
        with pytest.raises(RuntimeError, match="invalid element type"):
            plan.run(None, None, elem, 1, 1, 0, 0, (0, 1, 1), (0, 1, 1))


def test_every_table_row_has_its_half_kernels():
    """A half job takes the row the float32 job takes, so every row of fft_pairs needs float16 / bfloat16 instances: the
    half table (fft_half_kernels) is written from the instantiation lists, keyed by (N_in, N_out, threads) — every row of the
    schedule table is in exactly one of them, and each list is compiled in a unit of its own.  (Names only: the kernels
    themselves are run, instance by instance, by tests/test_gpu_fft_table_half.py; its case plan is held by tests/test_fft_table.py.)"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _table_probe as tp
    with open(tp.FFT_SRC) as f:
        text = f.read()
    rows, _ = tp.parse_table(text)
    lists = {}
    for name in ("HIPSOXR_PART1_SPECS", "HIPSOXR_PART2_SPECS", "HIPSOXR_PART8_SPECS", "HIPSOXR_PART5_SPECS"):
        line = re.search(r"#define " + name + r"\(X\)([^\n]*)\n", text).group(1)
        lists[name] = [(int(a), int(b), c.strip()) for a, b, c in re.findall(r"X\((\d+), (\d+), ([^)]*)\)", line)]
        assert lists[name], name
    nt_one_round = int(re.search(r"#define FFT_ONE_ROUND_NT (\d+)", text).group(1))
    half_table = re.search(r"static const HalfKernels halves\[\] = \{(.*?)\};", text, re.S).group(1)
    for name in lists:   # the half table is made of all four lists; the one-round sizes have unit-stride forms alone
        assert name + ("(HIPSOXR_HALF_ROW_F32)" if name == "HIPSOXR_PART5_SPECS" else "(HIPSOXR_HALF_ROW)") in half_table, name
    keyed = {}
    for name, specs in lists.items():
        for na, nb, nt in specs:
            key = (na, nb, nt_one_round if nt == "FFT_ONE_ROUND_NT" else int(nt))
            assert key not in keyed, (key, name, keyed.get(key))
            keyed[key] = name
    for r in rows:
        key = (r["NA"], r["NB"], nt_one_round if r["nt"] is None else r["nt"])
        assert key in keyed, "no float16 / bfloat16 kernels for table row " + tp.row_name(r)
        assert (keyed[key] == "HIPSOXR_PART5_SPECS") == (r["small"] == 3), (tp.row_name(r), keyed[key])
    assert len(keyed) == len({(r["NA"], r["NB"]) for r in rows})   # ... and the lists hold nothing the table does not use
    for unit, name in ((6, "HIPSOXR_PART1_SPECS(HIPSOXR_INST_HALF)"), (7, "HIPSOXR_PART2_SPECS(HIPSOXR_INST_HALF)"),
                       (8, "HIPSOXR_PART8_SPECS(HIPSOXR_INST_HALF)")):
        assert re.search(r"FFT_PART == %d\n#define HIPSOXR_EXTERN\n%s" % (unit, re.escape(name)), text), unit
    with open(os.path.join(ROOT, "python-soxr_amd", "build.sh")) as f:
        build = f.read()
    for unit in (6, 7, 8):
        assert "-DFFT_PART=%d " % unit in build and "fft%d.o" % unit in build.split("OBJS=")[1]
    assert "half.o" in build.split("OBJS=")[1]


def test_host_surface_stays_refused():
    import soxr_amd
    with pytest.raises(TypeError):
        soxr_amd.resample(np.zeros(100, np.float16), 48000, 44100)
