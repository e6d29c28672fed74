"""float16 / bfloat16 device jobs (HIPSOXR_F16 / HIPSOXR_BF16).

The contract is an identity, not a tolerance: a half job equals the float32 job of the same selector and layout on the
exactly widened values followed by ONE round-to-nearest-even conversion — bit for bit, whether the conversion is fused into
the frequency-domain engine's paired kernels (unit-stride columns, interleaved channel pairs, ragged unit-stride columns) or
runs as the widening / narrowing passes around the float32 job (everything else).  The host reference of every identity is
`resample_tensor(plan, x.float(), kernel=K).cpu().to(dtype)`: torch's conversions are exact on the way up and round to
nearest even on the way down, subnormals, infinities and overflow included.

One case is a tolerance by construction: a fused half job on ANOTHER block size than the float32 job's (forced in a child
process on the debug-switch build) is held to |y_half - y_f32| <= 4e-5 x RMS + half an ulp of the half type at y_f32 — the
engine's own bar of tests/test_gpu_fft.py plus the one rounding.  The same child's launch log names the kernel form each
shape took, so that a fused form that quietly fell back to the passes would fail here."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
AUTO, GATHER, FFT, EXACT, WAVE_DOT, FFT_F64, FFT_PCM, ADJOINT = 0, 1, 5, 6, 7, 8, 9, 10
HERE = os.path.dirname(os.path.abspath(__file__))
DBG_LIB = os.path.join(os.path.dirname(HERE), "python-soxr_amd", "_variants", "dbg", "libhipsoxr.so")
RATIOS = [(48000, 44100), (44100, 48000), (44100, 16000), (96000, 48000), (16000, 48000)]  # tests/test_gpu_fft_pcm.RATIOS


def _dtypes():
    import torch
    return {"float16": torch.float16, "bfloat16": torch.bfloat16}


DTYPES = ["float16", "bfloat16"]


def _gauss(rng, shape, dtype, rms=0.1):
    """Gaussian at `rms`, rounded to the half type: a device tensor of that type."""
    import torch
    return torch.from_numpy((rng.standard_normal(shape) * rms).astype(np.float32)).cuda().to(dtype)


def _bits(t):
    import torch
    return t.detach().cpu().contiguous().view(torch.int16)


def _assert_same_bits(got, want, what):
    import torch
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    g, w = _bits(got), _bits(want)
    ndiff = int((g != w).sum())
    print(f"{what}: {ndiff} of {g.numel()} differ")
    assert torch.equal(g, w), (what, ndiff, g.numel())


def _check(plan, x, kernel, what=""):
    """half job == float32 job on the widened values, rounded once (the host reference of every identity here)"""
    from soxr_amd import device as dev
    xf = x.float()
    y = dev.resample_tensor(plan, x, kernel=kernel)
    want = dev.resample_tensor(plan, xf, kernel=kernel).cpu().to(x.dtype)
    assert y.dtype == x.dtype and y.ndim == x.ndim
    _assert_same_bits(y, want, f"{what} {x.dtype} {tuple(x.shape)} kernel={kernel}")
    return y


# ---- fused identity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("quality", ["VHQ", "HQ"])
@pytest.mark.parametrize("in_rate,out_rate", RATIOS)
def test_identity_mono_and_batch(in_rate, out_rate, quality, dtype):
    """Unit-stride columns: k_fft_pair2's half forms, by name and under AUTO (>= 2^13 outputs in all: the float rule).
    44.1k -> 48k at 9001 frames is far below the 8192 block pairs from which float32 leaves k_fft_pair2."""
    from soxr_amd import device as dev
    dt = _dtypes()[dtype]
    rng = np.random.default_rng(in_rate + out_rate + (1 if quality == "HQ" else 0))
    plan = dev.Plan(in_rate, out_rate, quality)
    for shape in ((30011,), (3, 20001, 1), (9001,)):
        x = _gauss(rng, shape, dt)
        for kernel in (FFT, AUTO):
            _check(plan, x, kernel, f"{in_rate}->{out_rate} {quality}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("length", [1, 7, 4703, 4704, 4705, 100001])
def test_identity_lengths_and_edges(length, dtype):
    """48k -> 44.1k VHQ.  Each length as it is, as the odd-offset view x[1:] of a base tensor (2-byte alignment), and into an
    output view that starts at odd element offsets (the first granule's leading elements are somebody else's: sh != 0) —
    with sentinels around it, which must survive."""
    import torch
    from soxr_amd import device as dev
    dt = _dtypes()[dtype]
    rng = np.random.default_rng(length)
    plan = dev.Plan(48000, 44100, "VHQ")
    base = _gauss(rng, (length + 1,), dt)
    for kernel in (FFT, AUTO):
        _check(plan, base[:length], kernel, "aligned")
        _check(plan, base[1:], kernel, "odd offset")
    x = base[1:]
    n_out = plan.out_len(length)
    want = dev.resample_tensor(plan, x.float(), kernel=FFT).cpu().to(dt)
    for off in (1, 3, 6):
        buf = torch.full((n_out + 16,), 7.0, dtype=dt, device="cuda")
        y = dev.resample_tensor(plan, x, out=buf[off:off + n_out], kernel=FFT)
        _assert_same_bits(y, want, f"out offset {off}")
        guard = torch.cat([buf[:off], buf[off + n_out:]]).cpu()
        assert bool((guard == 7.0).all()), f"elements outside the output were written (offset {off})"


@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_odd_last_element(dtype):
    """Outputs whose last element stands alone in its dword (odd and even run ends, odd and even starts)."""
    import torch
    from soxr_amd import device as dev
    dt = _dtypes()[dtype]
    plan = dev.Plan(48000, 44100, "VHQ")
    rng = np.random.default_rng(5)
    seen = set()
    for length in (9001, 9002, 9003, 9004):
        x = _gauss(rng, (length,), dt)
        n_out = plan.out_len(length)
        seen.add(n_out & 1)
        want = dev.resample_tensor(plan, x.float(), kernel=FFT).cpu().to(dt)
        for off in (0, 1):
            buf = torch.full((n_out + 8,), -3.0, dtype=dt, device="cuda")
            y = dev.resample_tensor(plan, x, out=buf[off:off + n_out], kernel=FFT)
            _assert_same_bits(y, want, f"length {length} out offset {off}")
            assert bool((torch.cat([buf[:off], buf[off + n_out:]]).cpu() == -3.0).all())
    assert seen == {0, 1}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("in_rate,out_rate", [(48000, 44100), (44100, 16000)])
def test_identity_channel_pairs(in_rate, out_rate, dtype):
    """[frames, 2] and [frames, 4]: one aligned 4-byte (l, r) word per frame in and out; once with the base offset by two
    elements (still 4-byte aligned: fused) and once by one (2-byte aligned: the passes) — the same bits either way."""
    from soxr_amd import device as dev
    dt = _dtypes()[dtype]
    rng = np.random.default_rng(in_rate * 3 + out_rate)
    plan = dev.Plan(in_rate, out_rate, "VHQ")
    for shape in ((30011, 2), (20001, 4)):
        x = _gauss(rng, shape, dt)
        for kernel in (FFT, AUTO):
            _check(plan, x, kernel, "pairs")
    flat = _gauss(rng, (2 * 30011 + 2,), dt)
    _check(plan, flat[2:].view(30011, 2), AUTO, "pairs, base + 2 elements")
    _check(plan, flat[1:-1].view(30011, 2), AUTO, "pairs, base + 1 element")


# ---- values -------------------------------------------------------------------------------------------------------------
def test_float16_subnormals_are_exact_in_and_correctly_rounded_out():
    """RMS 1e-4: most samples are below float16's smallest normal (6.1e-5) — the level of audio near a zero crossing."""
    import torch
    from soxr_amd import device as dev
    plan = dev.Plan(48000, 44100, "VHQ")
    tiny = 2.0 ** -14
    for shape, kernel in (((30011,), FFT), ((30011, 2), AUTO), ((3001,), AUTO)):
        x = _gauss(np.random.default_rng(len(shape)), shape, torch.float16, rms=1e-4)
        y = _check(plan, x, kernel, "subnormals")
        for t in (x, y):
            a = t.float().abs()
            assert int(((a > 0) & (a < tiny)).sum()) > t.numel() // 10, "the case is vacuous: no subnormals"


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_samples(dtype):
    """One NaN and one +inf sample: the non-finite outputs stand where the reference has them, the finite ones have its bits."""
    import torch
    from soxr_amd import device as dev
    dt = _dtypes()[dtype]
    plan = dev.Plan(48000, 44100, "VHQ")
    for shape, kernel in (((30011,), FFT), ((30011, 2), AUTO), ((20001, 3), AUTO), ((30011,), EXACT)):
        x = _gauss(np.random.default_rng(11), shape, dt)
        x.view(-1)[1234] = float("nan")
        x.view(-1)[25000] = float("inf")
        y = dev.resample_tensor(plan, x, kernel=kernel).cpu()
        want = dev.resample_tensor(plan, x.float(), kernel=kernel).cpu().to(dt)
        bad, bad_want = ~torch.isfinite(y.float()), ~torch.isfinite(want.float())
        assert int(bad_want.sum()) > 0 and torch.equal(bad, bad_want), (shape, kernel, int(bad.sum()), int(bad_want.sum()))
        assert torch.equal(torch.isnan(y.float()), torch.isnan(want.float()))
        assert torch.equal(_bits(y)[~bad], _bits(want)[~bad])


def test_float16_overflow_becomes_inf_without_saturation():
    """+-60000 in runs of random length: the filter's overshoot passes 65504 and becomes +-inf exactly where the reference's
    conversion makes it so — as torch.Tensor.to does, no saturation."""
    import torch
    from soxr_amd import device as dev
    plan = dev.Plan(48000, 44100, "VHQ")
    rng = np.random.default_rng(3)
    for shape, kernel in (((50001,), FFT), ((30011, 2), AUTO), ((4001,), AUTO)):
        n = int(np.prod(shape))
        runs = rng.integers(1, 40, size=n)
        v = np.repeat(np.where(rng.random(n) < 0.5, -60000.0, 60000.0), runs)[:n].reshape(shape).astype(np.float16)
        x = torch.from_numpy(v).cuda()
        y = _check(plan, x, kernel, "overflow")
        assert int(torch.isinf(y).sum()) > 0 and not bool(torch.isnan(y).any())


# ---- ragged -------------------------------------------------------------------------------------------------------------
def _raw_ragged(plan, elem_t, in_base, out_buf, table, ch, kernel):
    import ctypes as C
    import torch
    from soxr_amd import _native as n, device as dev
    j = n.Job()
    j.in_, j.out, j.elem, j.kernel = in_base.data_ptr(), out_buf.data_ptr(), dev._torch_elem(elem_t), kernel
    j.n_clips, j.n_channels = table.shape[0], ch
    j.in_frame_stride, j.in_chan_stride, j.out_frame_stride, j.out_chan_stride = ch, 1, ch, 1
    j.in_frames, j.out_frames = int(table[:, 1].max()), int(table[:, 3].max())
    j.clip_table = table.ctypes.data
    n.check(n.lib.hipsoxr_run_device(plan.handle, C.byref(j), torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel", [AUTO, FFT, EXACT])
def test_ragged_packed_at_odd_offsets_with_guards(dtype, kernel):
    """Clips of 1, 4705, 20001 and 0 frames packed at odd element offsets, outputs packed at odd offsets with guard elements
    between them: one fused launch (AUTO, FFT) or clip by clip (EXACT) — the float32 job over the same table, rounded once,
    and no guard touched."""
    import torch
    from soxr_amd import device as dev
    dt = _dtypes()[dtype]
    plan = dev.Plan(48000, 44100, "VHQ")
    frames = [1, 4705, 20001, 0]
    n_out = [plan.out_len(n) for n in frames]
    in_off, out_off, pos_i, pos_o = [], [], 1, 3
    for n, m in zip(frames, n_out):
        in_off.append(pos_i); out_off.append(pos_o)
        pos_i += n + (1 if (pos_i + n) % 2 == 0 else 2)   # the next clip starts at an odd element again
        pos_o += m + (5 if (pos_o + m + 5) % 2 else 4)
    assert all(o % 2 for o in in_off + out_off)
    table = np.ascontiguousarray(np.stack([in_off, frames, out_off, n_out], axis=1), dtype=np.int64)
    x = _gauss(np.random.default_rng(17), (pos_i + 8,), dt)
    out = torch.full((pos_o + 8,), 9.0, dtype=dt, device="cuda")
    _raw_ragged(plan, dt, x, out, table, 1, kernel)
    ref = torch.full((pos_o + 8,), 9.0, dtype=torch.float32, device="cuda")
    _raw_ragged(plan, torch.float32, x.float(), ref, table, 1, kernel)
    _assert_same_bits(out, ref.cpu().to(dt), f"ragged kernel={kernel}")   # (9.0 is exact in both types: the guards compare too)
    mask = torch.ones(out.shape[0], dtype=torch.bool)
    for o, m in zip(out_off, n_out):
        mask[o:o + m] = False
    assert bool((out.cpu()[mask] == 9.0).all()), "guard elements between packed clips were written"


@pytest.mark.parametrize("dtype", DTYPES)
def test_ragged_job_surface(dtype):
    """dist.RaggedJob on half clips (views of one base at odd offsets) == the same job on their float32 widenings, rounded;
    and interleaved stereo clips — no fused ragged form — clip by clip under KERNEL_EXACT."""
    import torch
    from soxr_amd import device as dev, dist
    dt = _dtypes()[dtype]
    plan = dev.Plan(48000, 44100, "VHQ")
    base = _gauss(np.random.default_rng(23), (40000,), dt)
    basef = base.float()
    cuts = [(1, 1), (5, 4705), (4713, 20001), (30001, 0)]
    clips, clipsf = [base[a:a + n] for a, n in cuts], [basef[a:a + n] for a, n in cuts]
    for kernel in (AUTO, EXACT):
        got = dist.resample_ragged(plan, clips, kernel=kernel)
        want = dist.resample_ragged(plan, clipsf, kernel=kernel)
        for g, w in zip(got, want):
            _assert_same_bits(g, w.cpu().to(dt), f"RaggedJob kernel={kernel}")
    st = _gauss(np.random.default_rng(29), (30002,), dt)
    clips2 = [st[2:2 + 2 * 4705].view(4705, 2), st[2 + 2 * 4705:2 + 2 * 4705 + 2 * 7].view(7, 2)]
    got = dist.resample_ragged(plan, clips2, kernel=EXACT)
    for g, c in zip(got, clips2):
        _assert_same_bits(g, dev.resample_tensor(plan, c.float(), kernel=EXACT).cpu().to(dt), "stereo clips")


# ---- fallback identity: the float32 job under the same selector ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_fallback_identity(dtype):
    import torch
    from soxr_amd import _native as n, device as dev
    dt = _dtypes()[dtype]
    rng = np.random.default_rng(31)
    vhq = dev.Plan(48000, 44100, "VHQ")
    _check(dev.Plan(48000, 44100, "MQ"), _gauss(rng, (30011,), dt), AUTO, "MQ")
    interp = dev.Plan(48000, 44101, "VHQ")
    assert interp.phases
    _check(interp, _gauss(rng, (20001,), dt), AUTO, "two-stage form")
    _check(interp, _gauss(rng, (20001,), dt), EXACT, "interpolated-phase plan, exact engine")
    _check(vhq, _gauss(rng, (20001, 3), dt), AUTO, "odd interleaved channel count")
    _check(vhq, _gauss(rng, (20001, 3), dt), FFT, "odd interleaved channel count by name")
    _check(vhq, _gauss(rng, (500,), dt), AUTO, "small job")
    _check(vhq, _gauss(rng, (3, 2000, 2), dt), GATHER, "gather selector")
    _check(vhq, _gauss(rng, (20001, 4), dt)[:, ::2], EXACT, "non-dense view")   # (EXACT only: those bits are layout-independent)
    _check(dev.Plan(44100, 48000, "HQ"), _gauss(rng, (2, 9001, 2), dt).transpose(1, 2).contiguous().transpose(1, 2), AUTO, "planar channels")
    # one raw window: outputs [1000, 6000) of a column whose samples are all present
    x = _gauss(rng, (20001,), dt)
    xf = x.float()
    y = torch.full((5000 + 2,), 5.0, dtype=dt, device="cuda")
    yf = torch.empty(5000, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    vhq.run(x.data_ptr(), y[1:].data_ptr(), dev._torch_elem(dt), 1, 1, 20001, 5000, (0, 1, 1), (0, 1, 1), stream=st, out_k0=1000)
    vhq.run(xf.data_ptr(), yf.data_ptr(), n.F32, 1, 1, 20001, 5000, (0, 1, 1), (0, 1, 1), stream=st, out_k0=1000)
    _assert_same_bits(y[1:5001], yf.cpu().to(dt), "window out_k0 = 1000")
    assert float(y[0]) == 5.0 and float(y[5001]) == 5.0
    whole = dev.resample_tensor(vhq, xf, kernel=EXACT)
    assert torch.equal(yf, whole[1000:6000])   # (the window is the whole signal's outputs: the case is what it says)


# ---- gradient -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rates,grad_kernel", [((48000, 44100), AUTO), ((48000, 44101), ADJOINT)])
def test_gradient_is_the_float32_adjoint_rounded_once(rates, grad_kernel, dtype):
    import torch
    from soxr_amd import device as dev
    dt = _dtypes()[dtype]
    rng = np.random.default_rng(41)
    plan = dev.Plan(rates[0], rates[1], "VHQ")
    for shape in ((5001,), (2, 3001, 2)):
        x = _gauss(rng, shape, dt).requires_grad_(True)
        y = dev.resample_tensor(plan, x, grad_kernel=grad_kernel)
        assert y.dtype == dt and y.requires_grad
        gy = _gauss(rng, tuple(y.shape), dt, rms=1.0)
        y.backward(gy)
        n_in = shape[0] if len(shape) == 1 else shape[1]
        want = dev.resample_tensor_adjoint(plan, gy.float(), n_in, kernel=grad_kernel).cpu().to(dt)
        _assert_same_bits(x.grad, want, f"x.grad {rates} {shape}")
    # double backward: the adjoint's own gradient is the forward on the exact engine
    x = _gauss(rng, (4001,), dt).requires_grad_(True)
    y = dev.resample_tensor(plan, x, grad_kernel=grad_kernel)
    gy = _gauss(rng, tuple(y.shape), dt, rms=1.0).requires_grad_(True)
    (gx,) = torch.autograd.grad(y, x, gy, create_graph=True)
    assert gx.dtype == dt and gx.shape == x.shape and gx.requires_grad
    (ggy,) = torch.autograd.grad(gx, gy, torch.ones_like(gx))
    assert ggy.dtype == dt and ggy.shape == gy.shape and bool(torch.isfinite(ggy.float()).all())


# ---- refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_by_name(dtype):
    import torch
    from soxr_amd import device as dev, dist
    dt = _dtypes()[dtype]
    plan = dev.Plan(48000, 44100, "VHQ")
    x = _gauss(np.random.default_rng(1), (30011,), dt)
    with pytest.raises(RuntimeError, match="HIPSOXR_KERNEL_FFT_PCM serves int16 / int32 jobs"):
        dev.resample_tensor(plan, x, kernel=FFT_PCM)
    with pytest.raises(RuntimeError, match="HIPSOXR_KERNEL_FFT_F64 serves float32 / float64 jobs .*float16 / bfloat16"):
        dev.resample_tensor(plan, x, kernel=FFT_F64)
    with pytest.raises(RuntimeError, match="HIPSOXR_KERNEL_WAVE_DOT serves float32, float64, int32 and int16 jobs"):
        dev.resample_tensor(plan, x, kernel=WAVE_DOT)
    with pytest.raises(RuntimeError, match="FFT engine needs a whole-signal"):   # what a float32 job is told on an MQ plan
        dev.resample_tensor(dev.Plan(48000, 44100, "MQ"), x, kernel=FFT)
    with pytest.raises(TypeError, match="float32, float64, int16, int32, float16, bfloat16.*streams take four"):
        dev.TensorStream(48000, 44100, dtype=dt)
    with pytest.raises(TypeError, match="streams take four"):
        dev.TensorStreamGroup(2, 48000, 44100, dtype=dt)
    clips = [x[:3001].clone().requires_grad_(True), x[4000:9000].clone().requires_grad_(True)]
    with pytest.raises(RuntimeError, match="adjoint job: ragged: float16 / bfloat16 clip tables are not served"):
        dist.resample_ragged(plan, clips)
    with pytest.raises(RuntimeError, match="adjoint job: ragged: float16 / bfloat16 clip tables are not served"):
        dist.resample_ragged_adjoint(plan, [c.detach() for c in clips], [3300, 5500])
    got = dist.resample_ragged(plan, [c.detach() for c in clips])   # (without grad: served)
    assert [tuple(g.shape) for g in got] == [(plan.out_len(3001),), (plan.out_len(5000),)]


# ---- the other element types are untouched -----------------------------------------------------------------------------------
def test_float32_and_int16_golden_cases_after_a_half_job(soxr):
    """A float32 and an int16 case of tests/golden/oracle_vectors.json, run through the same process behind half jobs of
    the same plans: the bits those fixtures pin."""
    import torch
    from soxr_amd import device as dev
    with open(os.path.join(HERE, "golden", "oracle_vectors.json")) as f:
        cases = {c["name"]: c for c in json.load(f)["cases"]}
    for name in ("c1_vhq_48k_44k1_f32", "c4_vhq_44k1_16k_i16_2ch"):
        case = cases[name]
        rng = np.random.default_rng(case["seed"])
        x = rng.standard_normal((case["frames"], case["channels"]))
        x = (x * 5000).astype(case["dtype"]) if case["dtype"].startswith("int") else (x * 0.25).astype(case["dtype"])
        plan = dev.Plan(case["in_rate"], case["out_rate"], case["quality"])
        for dt in (torch.float16, torch.bfloat16):
            for kernel in (AUTO, EXACT):
                dev.resample_tensor(plan, torch.from_numpy(x.astype(np.float32) / (5000 if case["dtype"].startswith("int") else 1)).cuda().to(dt), kernel=kernel)
        torch.cuda.synchronize()
        y = soxr.resample(x, case["in_rate"], case["out_rate"], quality=case["quality"])
        assert y.shape[0] == case["out_frames"]
        assert hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest() == case["sha256"], name
        if case["dtype"] == "float32":   # ... and as a device job on the canonical-order engine
            yd = dev.resample_tensor(plan, torch.from_numpy(x).cuda(), kernel=EXACT).cpu().numpy()
            assert hashlib.sha256(np.ascontiguousarray(yd).tobytes()).hexdigest() == case["sha256"], name + " (device job)"


# ---- forms: the launch log of a debug-switch build, and the one tolerance case ---------------------------------------------------
def _half_ulp(y, dtype):
    """Half the spacing of the half type at |y| (float64 numpy): 11 / 8 significand bits, subnormal spacing below the smallest normal."""
    bits, emin = (10, -14) if dtype == "float16" else (7, -126)
    e = np.floor(np.log2(np.maximum(np.abs(y), 2.0 ** emin)))
    return 0.5 * 2.0 ** (e - bits)


def test_fused_forms_in_the_launch_log_and_another_block_size_within_the_bar(tmp_path):
    """Child process on the debug-switch build, HIPSOXR_DEBUG_FFT_K=20: the launch log names the fused forms (pair2 on
    float16 / a ragged table, strided2_cp on bfloat16 pairs), `none` then the float32 job's own line where there is no fused
    form, and nothing of the engine for small and EXACT jobs.  Its mono result ran blocks of 20 periods; the float32 job here
    takes the size rules' block (the forms differ by construction): within 4e-5 x RMS + half an ulp of float16."""
    import torch
    from soxr_amd import device as dev
    assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
    out, log = str(tmp_path / "y.npy"), str(tmp_path / "launch.log")
    env = dict(os.environ, HIPSOXR_LIBRARY=DBG_LIB, HIPSOXR_DEBUG_FFT_K="20", HIPSOXR_DEBUG_LAUNCH_LOG=log)
    r = subprocess.run([sys.executable, os.path.join(HERE, "_half_probe.py"), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    marks = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("HALF_PROBE ")][-1][len("HALF_PROBE "):])
    print(json.dumps(marks, indent=1))

    def fft_lines(key):
        return [ln for ln in marks[key] if ln.startswith("form=")]
    m = fft_lines("mono_f16_fft")
    assert len(m) == 1 and m[0].startswith("form=pair2 ") and " k=20 " in m[0] and " kind=f16 " in m[0], m
    s = fft_lines("stereo_bf16_auto")
    assert len(s) == 1 and s[0].startswith("form=strided2_cp ") and " kind=bf16 " in s[0], s
    s3 = fft_lines("stereo3_f16_auto")
    assert [ln.split()[0] for ln in s3] == ["form=none", "form=strided2_st"] and " kind=f16 " in s3[0] and " kind=f32 " in s3[1], s3
    g = fft_lines("ragged_f16_auto")
    assert len(g) == 1 and g[0].startswith("form=pair2 ") and " kind=f16 " in g[0] and g[0].endswith("ragged=3"), g
    assert not fft_lines("small_f16_auto") and not fft_lines("exact_f16")
    assert marks["small_f16_auto"] and marks["exact_f16"]   # (the float32 job's exact-engine launch is logged)

    plan = dev.Plan(48000, 44100, "VHQ")
    x = torch.from_numpy((np.random.default_rng(2024).standard_normal(9001) * 0.1).astype(np.float32)).cuda()
    yf = dev.resample_tensor(plan, x.half().float(), kernel=FFT).cpu().numpy().astype(np.float64)
    yh = torch.from_numpy(np.load(out)).view(torch.float16).numpy().astype(np.float64)
    assert yh.shape == yf.shape
    rms = float(np.sqrt(np.mean(yf ** 2)))
    excess = np.abs(yh - yf) - (4e-5 * rms + _half_ulp(yf, "float16"))
    print(f"forced k=20 against the size rules' block: max |diff| {np.abs(yh - yf).max():.3e}, RMS {rms:.3e}, worst excess {excess.max():.3e}")
    assert np.all(excess <= 0), float(excess.max())
