"""GPU: the two-stage form's adjoint (HIPSOXR_KERNEL_ADJOINT_TWO_STAGE; csrc/twostage.hip k_poly_adj, launch_adjoint_two_stage):
gx = A^T gy, A the forward job the two-stage form runs under KERNEL_AUTO on an interpolated-phase plan — the FFT stage's
transposed plan on the frequency-domain engine and the gather-form transpose of the polyphase stage.

REFERENCE: the float64 exact adjoint, resample_tensor_adjoint(plan, gy.double(), n_x, kernel=KERNEL_ADJOINT), which
tests/test_gpu_adjoint_interp.py pins to the oracle's coefficients.  BARS: relative RMS 1e-6 (float32), 2e-9 (float64 VHQ) —
tests/test_gpu_two_stage.py's — and 1e-6 (float64 HQ: its -128 dB stop band aliases; tests/test_gpu_adjoint_fft.py's);
pointwise 4e-5 x RMS(ref) over the whole result, the first and last 64 frames looked at separately.  Every figure is printed
before it is asserted.

RATE PAIRS: _adjoint_two_stage_probe.PAIRS.  Two of them take 40 and 56 polyphase taps: the 56-tap design has no two-stage
form in either width (poly_design refuses its table), and float64 tables of 40 taps or more leave LDS — the forward form does
not take those jobs (AUTO == EXACT), so they are REPLACED (_adjoint_two_stage_probe.REPLACED), not skipped.  For every
(pair, width) the precondition is asserted: the forward under KERNEL_AUTO differs in bits from KERNEL_EXACT — the two-stage
form is what is being transposed.  SIZES: the smallest n_x with both sides at 8192 frames or more, one more, and about 20000
(for the steep pairs, whose smallest size is above that: 1100 output frames' worth more than the smallest).

INSTANCES: k_poly_adj has ten tap counts; eight are reachable by HQ / VHQ plans (_adjoint_two_stage_probe.COVER, UNREACHABLE:
8 and 56 taps) and each is launched once per width it fits (float64: up to 32 taps) in a child process on the debug-switch build,
the instance read from the launch log's poly_adj line.  After a failed child or a HIP error nothing further is started from
this file."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _adjoint_two_stage_probe as tp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DBG_LIB = os.path.join(os.path.dirname(HERE), "python-soxr_amd", "_variants", "dbg", "libhipsoxr.so")
REL32, POINT = 1e-6, 4e-5
REL64 = {"VHQ": 2e-9, "HQ": 1e-6}
GUARD, POISON = 8, 12345.0
KINDS = ("f32", "f64")

_stopped = []  # a failed child or a HIP error: nothing further is started on the GPU from this file


@pytest.fixture(autouse=True)
def _nothing_after_a_failure():
    if _stopped:
        pytest.fail("an earlier GPU step of this file failed (%s): no further GPU work from it" % _stopped[0])


def _dtype(kind):
    import torch
    return torch.float32 if kind == "f32" else torch.float64


def _bar(case, kind):
    return REL32 if kind == "f32" else REL64[case[2]]


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2))) if np.size(a) else 0.0


@functools.lru_cache(maxsize=None)
def _plan(case):
    from soxr_amd import device as dev
    plan = dev.Plan(*case)
    assert plan.phases, "an interpolated-phase plan is what this file is about"
    return plan


def _sizes(case):
    plan = _plan(case)
    n0 = tp.smallest(plan)
    assert min(n0, plan.out_len(n0)) >= tp.MIN_FRAMES and (n0 == tp.MIN_FRAMES or plan.out_len(n0 - 1) < tp.MIN_FRAMES)
    # (the third also serves the truncated job: 1000 outputs fewer must leave 8192)
    third = 20011 if 20011 > n0 + 1 and plan.out_len(20011) - 1000 >= tp.MIN_FRAMES else n0 + int(1100 * plan.in_rate / plan.out_rate) + 1
    return (n0, n0 + 1, third)


def _two(plan, gy, n_x, **kw):
    from soxr_amd import device as dev
    try:
        return dev.resample_tensor_adjoint(plan, gy, n_x, kernel=dev.KERNEL_ADJOINT_TWO_STAGE, **kw)
    except RuntimeError as e:  # (a HIP error surfaces as RuntimeError, from torch or from the library; a refusal by name is none)
        if "adjoint job:" not in str(e):
            _stopped.append(str(e)[:200])
        raise


@functools.lru_cache(maxsize=None)
def _job(case, kind, n_x, cut=0):
    """(gy, reference gx float64 numpy): white noise, the float64 exact adjoint of the same values — computed once, shared"""
    import torch
    from soxr_amd import device as dev
    plan = _plan(case)
    gen = torch.Generator(device="cuda").manual_seed(1000 + n_x + cut)
    gy = torch.randn(plan.out_len(n_x) - cut, dtype=_dtype(kind), device="cuda", generator=gen)
    ref = dev.resample_tensor_adjoint(plan, gy.double(), n_x, kernel=dev.KERNEL_ADJOINT).cpu().numpy()
    ref.setflags(write=False)
    return gy, ref


def _check_values(case, kind, got, ref, tag):
    err = got.astype(np.float64) - ref
    scale = _rms(ref)
    rel, worst = _rms(err) / scale, float(np.abs(err).max()) / scale
    head, tail = float(np.abs(err[:64]).max()) / scale, float(np.abs(err[-64:]).max()) / scale
    print("adjoint_two_stage %s: rel rms %.3g (bar %.3g) worst/rms %.3g head %.3g tail %.3g (bar %.3g)" % (tag, rel, _bar(case, kind), worst, head, tail, POINT))
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert 0 < rel <= _bar(case, kind), (tag, rel)
    assert worst <= POINT and head <= POINT and tail <= POINT, (tag, worst, head, tail)


def _assert_two_stage_forward(case, kind, n_x):
    """the precondition, never skipped: AUTO's forward is not the exact engine's on this plan, width and size"""
    import torch
    from soxr_amd import device as dev
    plan = _plan(case)
    x = torch.randn(n_x, dtype=_dtype(kind), device="cuda", generator=torch.Generator(device="cuda").manual_seed(n_x))
    y = dev.resample_tensor(plan, x)
    assert not torch.equal(y, dev.resample_tensor(plan, x, kernel=dev.KERNEL_EXACT)), (case, kind, n_x, "AUTO ran the exact engine")
    return x, y


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", tp.PAIRS, ids=lambda c: "%g-%g-%s" % c)
def test_values_transpose_and_truncation(case, kind):
    import torch
    case = tp.case_for(case, kind)
    plan = _plan(case)
    assert tp.poly_taps(plan) <= (tp.F64_MAX_TAPS if kind == "f64" else max(tp.TAPS))
    for n_x in _sizes(case):
        tag = "%g-%g-%s %s n_x=%d" % (case + (kind, n_x))
        x, y = _assert_two_stage_forward(case, kind, n_x)
        gy, ref = _job(case, kind, n_x)
        gx = _two(plan, gy, n_x)  # (no listed job may raise "unavailable")
        _check_values(case, kind, gx.cpu().numpy(), ref, tag)
        # 5. two runs give the same bits
        assert torch.equal(gx, _two(plan, gy, n_x)), tag
        # 2. the transpose of the GPU forward: <A x, gy> = <x, A^T gy>
        lhs, rhs = float((y.double() * gy.double()).sum()), float((x.double() * gx.double()).sum())
        bound = 2 * _bar(case, kind) * float(x.double().norm() * gy.double().norm()) * max(1.0, (plan.out_rate / plan.in_rate) ** 0.5)
        print("adjoint_two_stage %s: |<y, gy> - <x, A^T gy>| %.3g, bound %.3g" % (tag, abs(lhs - rhs), bound))
        assert abs(lhs - rhs) <= bound, tag
    # 3. a truncated cotangent: the forward job truncated by 1000 outputs, transposed
    n_x = _sizes(case)[2]
    gy, ref = _job(case, kind, n_x, 1000)
    assert gy.shape[0] == plan.out_len(n_x) - 1000 >= tp.MIN_FRAMES
    _check_values(case, kind, _two(plan, gy, n_x).cpu().numpy(), ref, "%g-%g-%s %s truncated n_x=%d" % (case + (kind, n_x)))


@pytest.fixture(scope="module")
def instances(tmp_path_factory):
    assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
    tmp = tmp_path_factory.mktemp("adjoint_two_stage")
    env = {key: v for key, v in os.environ.items() if not key.startswith("HIPSOXR_")}
    env.update({"HIPSOXR_LIBRARY": DBG_LIB, "HIPSOXR_DEBUG_LAUNCH_LOG": str(tmp / "launch.log")})
    r = subprocess.run([sys.executable, os.path.join(HERE, "_adjoint_two_stage_probe.py"), str(tmp / "results.npz")], env=env,
                       capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        _stopped.append("probe exit status %d" % r.returncode)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(tmp / "results.npz")


def test_every_reachable_instance_is_launched(instances):
    assert sorted(list(tp.COVER) + list(tp.UNREACHABLE)) == sorted(tp.TAPS) and tp.UNREACHABLE == (8, 56)
    seen = set()
    for taps, case in sorted(tp.COVER.items()):
        plan = _plan(case)
        assert tp.poly_taps(plan) == taps
        for kind in KINDS:
            if kind == "f64" and taps > tp.F64_MAX_TAPS:
                continue
            lines = str(instances["log_%d_%s" % (taps, kind)]).splitlines()
            poly = [tp.fields(ln) for ln in lines if ln.startswith("kernel=poly_adj ")]
            assert len(poly) == 1 and len(lines) == 2, lines  # one k_poly_adj launch and the FFT stage's line
            f = poly[0]
            up = plan.out_rate > plan.in_rate
            assert (int(f["T"]), int(f["width"])) == (taps, 4 if kind == "f32" else 8), f
            assert int(f["R"]) in (1, 2, 4) and int(f["lds"]) <= 160 * 1024 and f["block"] == "256"
            # the FFT stage first down (its transposed plan is 1:2), last up (2:1)
            fft = tp.fields(lines[0 if not up else 1])
            assert (int(fft["L"]), int(fft["M"])) == ((2, 1) if not up else (1, 2)) and fft["form"] != "none", fft
            seen.add((taps, kind))
            _check_values(case, kind, instances["got_%d_%s" % (taps, kind)], instances["ref_%d_%s" % (taps, kind)], "instance T=%d %s" % (taps, kind))
    assert len(seen) == 8 + 6


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", ["interleaved3", "planar2"])
def test_layouts_and_guards(layout, kind):
    """Three clips x 3 interleaved channels / 2 planar channels, gy and out= strided views: the guard frames stay, every element
    is written, and each column has the bits of the column run alone."""
    import torch
    case = (48000, 44101, "VHQ") if layout == "interleaved3" else (44101, 48000, "HQ")
    plan, dt = _plan(case), _dtype(kind)
    n_x = tp.smallest(plan) + 5
    n_y, clips = plan.out_len(n_x), 3
    gen = torch.Generator(device="cuda").manual_seed(5)
    if layout == "interleaved3":
        ch = 3
        gy = torch.randn(clips, n_y, 4, dtype=dt, device="cuda", generator=gen)[:, :, :ch]
        buf = torch.full((clips, n_x + 2 * GUARD, 5), POISON, dtype=dt, device="cuda")
        out, guards = buf[:, GUARD:-GUARD, 1:1 + ch], (buf[:, :GUARD], buf[:, -GUARD:], buf[:, :, :1], buf[:, :, 1 + ch:])
    else:
        ch = 2
        gy = torch.randn(clips, ch, n_y + 5, dtype=dt, device="cuda", generator=gen)[:, :, :n_y].permute(0, 2, 1)
        buf = torch.full((clips, ch, n_x + 2 * GUARD), POISON, dtype=dt, device="cuda")
        out, guards = buf[:, :, GUARD:-GUARD].permute(0, 2, 1), (buf[:, :, :GUARD], buf[:, :, -GUARD:])
    assert not gy.is_contiguous() and not out.is_contiguous()
    got = _two(plan, gy, n_x, out=out)
    assert got.data_ptr() == out.data_ptr()
    for g in guards:
        assert (g == POISON).all(), "a guard element was written"
    assert torch.isfinite(out).all() and not (out == POISON).any(), "an element of gx was not written"
    for c in range(clips):
        for k in range(ch):
            alone = _two(plan, gy[c, :, k].contiguous(), n_x)
            same = torch.equal(out[c, :, k], alone)
            diff = float((out[c, :, k].double() - alone.double()).abs().max())
            print("adjoint_two_stage %s %s clip %d channel %d: equal bits %s (max difference %.3g)" % (layout, kind, c, k, same, diff))
            assert same, (layout, kind, c, k, diff)
    first = out.clone()
    assert torch.equal(_two(plan, gy, n_x, out=out), first)  # ... and a second run into the same view


def test_half_is_the_float32_job_rounded_once():
    import torch
    case = (48000, 44101, "VHQ")
    plan = _plan(case)
    n_x = tp.smallest(plan)
    for dt in (torch.float16, torch.bfloat16):
        for shape in ((plan.out_len(n_x),), (plan.out_len(n_x), 2)):
            gy = torch.randn(shape, device="cuda").to(dt)
            got = _two(plan, gy, n_x)
            want = _two(plan, gy.float(), n_x).to(dt)
            assert got.dtype == dt and torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_autograd():
    import torch
    from soxr_amd import device as dev
    K = dev.KERNEL_ADJOINT_TWO_STAGE
    case = (44101, 48000, "VHQ")
    plan = _plan(case)
    n = tp.smallest(plan) + 100
    for dt in (torch.float32, torch.float64):
        x = torch.randn(n, 2, dtype=dt, device="cuda")
        xr = x.clone().requires_grad_()
        y = dev.resample_tensor(plan, xr, grad_kernel=K)
        assert y.grad_fn is not None and torch.equal(y.detach(), dev.resample_tensor(plan, x))
        gy = torch.randn_like(y)
        y.backward(gy)
        assert torch.equal(xr.grad, dev.resample_tensor_adjoint(plan, gy, n, kernel=K))
        # the double backward: the adjoint's own backward is the forward under AUTO — the two-stage form
        gyr = gy.clone().requires_grad_()
        ggx = torch.randn(n, 2, dtype=dt, device="cuda")
        dev.resample_tensor_adjoint(plan, gyr, n, kernel=K).backward(ggx)
        assert torch.equal(gyr.grad, dev.resample_tensor(plan, ggx))
        gy2 = gy.clone().requires_grad_()
        (g2,) = torch.autograd.grad(dev.resample_tensor(plan, xr, grad_kernel=K), xr, gy2, create_graph=True)
        g2.backward(ggx)
        assert torch.equal(gy2.grad, gyr.grad)
        # without requires_grad nothing changes, and the other gradient keeps its bits
        assert dev.resample_tensor(plan, x, grad_kernel=K).grad_fn is None
        xe = x.clone().requires_grad_()
        dev.resample_tensor(plan, xe, grad_kernel=dev.KERNEL_ADJOINT).backward(gy)
        assert torch.equal(xe.grad, dev.resample_tensor_adjoint(plan, gy, n, kernel=dev.KERNEL_ADJOINT)) and not torch.equal(xe.grad, xr.grad)


@pytest.mark.parametrize("case", [(48000, 44101, "HQ"), (8000, 44100.25, "VHQ")], ids=lambda c: "%g-%g-%s" % c)
def test_a_fresh_plan_adjoint_before_any_forward(case):
    import torch
    from soxr_amd import device as dev
    plan = dev.Plan(*case)  # (a plan of its own: nothing has run on it)
    n_x = tp.smallest(plan)
    gy, ref = _job(case, "f32", n_x)
    gx = _two(plan, gy, n_x)
    _check_values(case, "f32", gx.cpu().numpy(), ref, "fresh plan %g-%g-%s" % case)
    assert torch.equal(gx, _two(_plan(case), gy, n_x))
    torch.cuda.synchronize()
    del plan


def test_refusals_with_a_device_present():
    import torch
    from soxr_amd import _native, device as dev, dist
    K = _native.KERNEL_ADJOINT_TWO_STAGE
    plan = _plan((48000, 44101, "VHQ"))
    unavailable = r"^adjoint job: HIPSOXR_KERNEL_ADJOINT_TWO_STAGE: the two-stage form is unavailable .*HIPSOXR_KERNEL_ADJOINT runs the exact adjoint$"
    # a job the form does not admit: fewer than 8192 frames — never the exact adjoint in its place
    for dt in (torch.float32, torch.float64, torch.float16):
        n_x = 4000
        gy = torch.randn(plan.out_len(n_x), dtype=dt, device="cuda")
        out = torch.full((n_x,), POISON, dtype=dt, device="cuda")
        with pytest.raises(RuntimeError, match=unavailable):
            _two(plan, gy, n_x, out=out)
        torch.cuda.synchronize()
        assert (out == POISON).all()
    n_x = tp.smallest(plan)
    gy = torch.randn(plan.out_len(n_x), device="cuda")
    out = torch.full((n_x,), POISON, device="cuda")
    # a plan without the form: below HQ; an exact-bank plan; integers; the forward entry; the ragged entry
    with pytest.raises(RuntimeError, match=unavailable):
        _two(dev.Plan(48000, 44101, "MQ"), gy, n_x, out=out)
    with pytest.raises(RuntimeError, match="ADJOINT_TWO_STAGE needs an interpolated-phase plan .*HIPSOXR_KERNEL_ADJOINT_FFT"):
        exact = dev.Plan(48000, 44100, "VHQ")
        _two(exact, torch.randn(exact.out_len(n_x), device="cuda"), n_x, out=out)
    with pytest.raises(RuntimeError, match="ADJOINT_TWO_STAGE serves float32 or float64"):
        _two(plan, torch.zeros(100, dtype=torch.int16, device="cuda"), 200)
    y = torch.full((plan.out_len(n_x),), POISON, device="cuda")
    with pytest.raises(RuntimeError, match="HIPSOXR_KERNEL_ADJOINT_TWO_STAGE selects the transposed two-stage form"):
        dev.resample_tensor(plan, torch.randn(n_x, device="cuda"), out=y, kernel=K)
    with pytest.raises(RuntimeError, match="ADJOINT_TWO_STAGE: ragged clip tables are not served yet"):
        dist.resample_ragged_adjoint(plan, [gy], [n_x], kernel=K)
    with pytest.raises(RuntimeError, match="ADJOINT_TWO_STAGE: ragged clip tables are not served yet"):  # ... at forward time
        dist.resample_ragged(plan, [torch.randn(n_x, device="cuda").requires_grad_()], grad_kernel=K)
    torch.cuda.synchronize()
    assert (out == POISON).all() and (y == POISON).all()  # a refusal never falls through to another path
    assert torch.equal(_two(plan, gy, n_x, out=out), _two(plan, gy, n_x)) and not (out == POISON).any()
