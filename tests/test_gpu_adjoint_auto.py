"""GPU: HIPSOXR_KERNEL_ADJOINT_AUTO (csrc/adjoint_auto.hip; csrc/twostage.hip launch_adjoint_two_stage_ragged, k_poly_adj's RAGGED
instances) — the transpose of the job the forward launches under KERNEL_AUTO for the same plan and shape, on both adjoint
entries.  Every test here fails on a library without the selector (13 is refused).

EQUAL LENGTHS: the selector resolves to a named selector's launch, so the bits are that selector's (torch.equal).
RAGGED, EXACT BANK: the bits of the ragged KERNEL_ADJOINT_FFT launch from 8192 cotangent frames in all, of KERNEL_ADJOINT below.
RAGGED, INTERPOLATED PHASES: through the C-level plan.run_adjoint_ragged on the mixed table of _adjoint_auto_probe.mixed_rows,
GUARD poisoned frames between clips on the gx side.  Two-stage clips against the float64 exact adjoint of the clip alone with
the BARS OF tests/test_gpu_adjoint_two_stage.py, copied: relative RMS 1e-6 (float32), 2e-9 (float64 VHQ), 1e-6 (float64 HQ);
pointwise 4e-5 x RMS(ref) over the whole clip, the first and last 64 frames looked at separately; every figure is printed
before it is asserted.  Short clips: the bits of KERNEL_ADJOINT on the clip alone.  The identity <A x, gy> = <x, A^T gy> over
the table: that file's bound, 2 x bar x |x| |gy| max(1, sqrt(out / in)).
LAUNCH SHAPE: child processes on the debug-switch build (_adjoint_auto_probe.py) — the number of launches does not depend on
the number of clips, a table cut into 3 ranges has the bits of the uncut one, and every reachable tap count of k_poly_adj is
launched in ragged form once per width.  After a failed child or a HIP error nothing further is started from this file."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _adjoint_auto_probe as ap
import _adjoint_two_stage_probe as tp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DBG_LIB = os.path.join(os.path.dirname(HERE), "python-soxr_amd", "_variants", "dbg", "libhipsoxr.so")
REL32, POINT = 1e-6, 4e-5                # tests/test_gpu_adjoint_two_stage.py REL32, POINT
REL64 = {"VHQ": 2e-9, "HQ": 1e-6}        # ... REL64
GUARD, POISON = ap.GUARD, ap.POISON
KINDS = ("f32", "f64")

_stopped = []  # a failed child or a HIP error: nothing further is started on the GPU from this file


@pytest.fixture(autouse=True)
def _nothing_after_a_failure():
    if _stopped:
        pytest.fail("an earlier GPU step of this file failed (%s): no further GPU work from it" % _stopped[0])


def _guarded(fn, *a, **kw):
    """fn(*a, **kw); a RuntimeError that is no refusal by name — a HIP error, from torch or from the library — stops the file"""
    try:
        return fn(*a, **kw)
    except RuntimeError as e:
        if "adjoint job:" not in str(e) and "HIPSOXR_KERNEL" not in str(e):
            _stopped.append(str(e)[:200])
        raise


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
    return dev.Plan(*case)


def _check_values(case, kind, got, ref, tag):
    err = got.astype(np.float64) - ref
    scale = _rms(ref)
    rel, worst = _rms(err) / scale, float(np.abs(err).max()) / scale
    head, tail = float(np.abs(err[:64]).max()) / scale, float(np.abs(err[-64:]).max()) / scale
    print("adjoint_auto %s: rel rms %.3g (bar %.3g) worst/rms %.3g head %.3g tail %.3g (bar %.3g)" % (tag, rel, _bar(case, kind), worst, head, tail, POINT))
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert 0 < rel <= _bar(case, kind), (tag, rel)
    assert worst <= POINT and head <= POINT and tail <= POINT, (tag, worst, head, tail)


def _adj(plan, gy, n_x, kernel):
    from soxr_amd import device as dev
    return _guarded(dev.resample_tensor_adjoint, plan, gy, n_x, kernel=kernel)


# ---- equal lengths: the named selector's bits ------------------------------------------------------------------------------
def _n_x_for(plan, n_y):
    n = int(n_y * plan.in_rate / plan.out_rate)
    while plan.out_len(n) < n_y:
        n += 1
    return n


@pytest.mark.parametrize("kind", KINDS)
def test_equal_lengths_resolve_to_the_named_selectors(kind):
    import torch
    from soxr_amd import device as dev
    K, dt = dev.KERNEL_ADJOINT_AUTO, _dtype(kind)
    gen = torch.Generator(device="cuda").manual_seed(11)
    interp = (48000, 44101, "VHQ")
    forty = [c for c in tp.REPLACED["f64"] if tp.poly_taps(_plan(c)) == 40][0]
    # (case, cotangent frames or None = the whole output of n_x, n_x or None = the least that holds the cotangent, selector it resolves to)
    jobs = [((48000, 44100, "VHQ"), 8192, None, dev.KERNEL_ADJOINT_FFT),
            ((48000, 44100, "VHQ"), 4000, None, dev.KERNEL_ADJOINT),
            ((48000, 44100, "MQ"), 20000, None, dev.KERNEL_ADJOINT),
            (interp, None, tp.smallest(_plan(interp)), dev.KERNEL_ADJOINT_TWO_STAGE),
            (interp, None, 4000, dev.KERNEL_ADJOINT),
            ((48000, 44101, "MQ"), None, 20000, dev.KERNEL_ADJOINT)]
    if kind == "f64":  # 40 taps: the float64 table leaves LDS, the forward form does not take the job
        jobs.append((forty, None, tp.smallest(_plan(forty)), dev.KERNEL_ADJOINT))
    for case, n_y, n_x, named in jobs:
        plan = _plan(case)
        n_x = _n_x_for(plan, n_y) if n_x is None else n_x
        n_y = plan.out_len(n_x) if n_y is None else n_y
        gy = torch.randn(n_y, dtype=dt, device="cuda", generator=gen)
        got, want = _adj(plan, gy, n_x, K), _adj(plan, gy, n_x, named)
        same = torch.equal(got, want)
        print("adjoint_auto equal %s %s n_y=%d n_x=%d: the bits of selector %d: %s" % ("%g-%g-%s" % case, kind, n_y, n_x, named, same))
        assert same and got.shape == (n_x,), (case, kind, named)
        if named != dev.KERNEL_ADJOINT:  # ... and it is the fast form that ran, not the exact adjoint
            assert not torch.equal(got, _adj(plan, gy, n_x, dev.KERNEL_ADJOINT)), (case, kind)
    # two clips x two channels: the total counts, not the frames (2048 x 2 x 2 = 8192)
    plan = _plan((48000, 44100, "VHQ"))
    for n_y, named in ((2048, dev.KERNEL_ADJOINT_FFT), (2047, dev.KERNEL_ADJOINT)):
        gy = torch.randn(2, n_y, 2, dtype=dt, device="cuda", generator=gen)
        n_x = _n_x_for(plan, n_y)
        assert torch.equal(_adj(plan, gy, n_x, K), _adj(plan, gy, n_x, named)), (n_y, named)


def test_half_is_the_float32_job_rounded_once():
    import torch
    from soxr_amd import device as dev
    K = dev.KERNEL_ADJOINT_AUTO
    for case in ((48000, 44101, "VHQ"), (48000, 44100, "VHQ")):
        plan = _plan(case)
        n_x = max(tp.smallest(plan) if plan.phases else 0, _n_x_for(plan, 8192))
        gy = torch.randn(plan.out_len(n_x), 2, device="cuda").to(torch.float16)
        got, want = _adj(plan, gy, n_x, K), _adj(plan, gy.float(), n_x, K).to(torch.float16)
        assert got.dtype == torch.float16 and torch.equal(got.view(torch.int16), want.view(torch.int16)), case


# ---- ragged, exact-bank plan --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_ragged_exact_bank_resolves_to_the_named_selectors(kind):
    import torch
    from soxr_amd import device as dev, dist
    plan, dt = _plan((48000, 44100, "VHQ")), _dtype(kind)
    gen = torch.Generator(device="cuda").manual_seed(12)
    for n_ys, named in (((300, 9000, 4111, 2048, 777), dev.KERNEL_ADJOINT_FFT), ((300, 4000, 2048, 1066, 777), dev.KERNEL_ADJOINT)):
        assert (sum(n_ys) >= 8192) == (named == dev.KERNEL_ADJOINT_FFT)
        n_xs = [_n_x_for(plan, n) for n in n_ys]
        gys = [torch.randn(n, dtype=dt, device="cuda", generator=gen) for n in n_ys]
        got = _guarded(dist.resample_ragged_adjoint, plan, gys, n_xs, kernel=dev.KERNEL_ADJOINT_AUTO)
        want = _guarded(dist.resample_ragged_adjoint, plan, gys, n_xs, kernel=named)
        other = _guarded(dist.resample_ragged_adjoint, plan, gys, n_xs, kernel=dev.KERNEL_ADJOINT if named == dev.KERNEL_ADJOINT_FFT else dev.KERNEL_ADJOINT_FFT)
        for c, (g, w, o) in enumerate(zip(got, want, other)):
            assert torch.equal(g, w) and g.shape == (n_xs[c],), (kind, named, c)
        assert not all(torch.equal(g, o) for g, o in zip(got, other)), (kind, named)  # (the two engines differ in bits: the test can tell them apart)


# ---- ragged, interpolated-phase plan ---------------------------------------------------------------------------------------
def _assert_two_stage_forward(plan, kind, rows, channels):
    """the precondition, never skipped: the ragged forward under AUTO is not the exact engine's on the two-stage clips"""
    import torch
    from soxr_amd import device as dev, dist
    gen = torch.Generator(device="cuda").manual_seed(13)
    shape = (lambda n: (n,)) if channels == 1 else (lambda n: (n, channels))
    xs = [torch.randn(shape(n_x), dtype=_dtype(kind), device="cuda", generator=gen) for n_x, _, _ in rows]
    fed = [c for c, (n_x, _, _) in enumerate(rows) if n_x]  # (the row without input has no forward)
    auto, exact = (_guarded(dist.resample_ragged, plan, [xs[c] for c in fed], kernel=k) for k in (dev.KERNEL_AUTO, dev.KERNEL_EXACT))
    ys = [None] * len(rows)
    for c, a, e in zip(fed, auto, exact):
        n_x, _, cls = rows[c]
        forward_two = min(n_x, plan.out_len(n_x)) >= tp.MIN_FRAMES  # (the forward's class is the whole clip's: the clip without cotangent is a two-stage clip there)
        assert forward_two or cls != "two"
        assert torch.equal(a, e) != forward_two, (n_x, "AUTO ran the exact engine" if forward_two else "a short clip left the exact engine")
        ys[c] = a
    return xs, ys


def _ragged_case(case, kind, channels):
    import torch
    from soxr_amd import device as dev
    plan = _plan(case)
    assert plan.phases
    rows = ap.mixed_rows(plan)
    tag = "%g-%g-%s %s ch=%d" % (case + (kind, channels))
    xs, ys = _assert_two_stage_forward(plan, kind, rows, channels)
    job = ap.Job(plan, rows, _dtype(kind), channels)
    gx = _guarded(job.run, dev.KERNEL_ADJOINT_AUTO)
    torch.cuda.synchronize()
    first = gx.clone()
    assert (job.guards() == POISON).all(), "a guard element, or the surroundings of the row without input, was written"
    lhs = rhs = nx2 = ny2 = 0.0
    for c, (n_x, n_y, cls) in enumerate(rows):
        gy_c, gx_c = job.clip_gy(c), job.clip_gx(c)
        if channels == 1:
            gy_c, gx_c = gy_c[:, 0], gx_c[:, 0]
        assert gx_c.shape[0] == n_x and gy_c.shape[0] == n_y
        if cls == "empty":
            continue
        assert not (gx_c == POISON).any(), (tag, c, "an element of gx was not written")
        if cls == "two":
            ref = _adj(plan, gy_c.double().contiguous(), n_x, dev.KERNEL_ADJOINT).cpu().numpy()
            _check_values(case, kind, gx_c.cpu().numpy(), ref, "%s clip %d n_x=%d n_y=%d" % (tag, c, n_x, n_y))
        elif cls == "short":
            alone = _adj(plan, gy_c.contiguous(), n_x, dev.KERNEL_ADJOINT)
            same = torch.equal(gx_c, alone)
            print("adjoint_auto %s clip %d n_x=%d (short): the bits of KERNEL_ADJOINT on the clip alone: %s" % (tag, c, n_x, same))
            assert same, (tag, c)
        else:  # no cotangent: zeros
            assert cls == "zero" and (gx_c == 0).all(), (tag, c)
        # the identity's sums, over the table: A the ragged forward under AUTO (a truncated cotangent meets the first n_y outputs)
        y_c = ys[c][:n_y]
        lhs += float((y_c.double() * gy_c.double()).sum())
        rhs += float((xs[c].double() * gx_c.double()).sum())
        nx2 += float(xs[c].double().pow(2).sum())
        ny2 += float(gy_c.double().pow(2).sum())
    bound = 2 * _bar(case, kind) * (nx2 * ny2) ** 0.5 * max(1.0, (plan.out_rate / plan.in_rate) ** 0.5)
    print("adjoint_auto %s: |<A x, gy> - <x, A^T gy>| %.3g over the table, bound %.3g" % (tag, abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound, tag
    # a second run: the same bits
    assert torch.equal(_guarded(job.run, dev.KERNEL_ADJOINT_AUTO), first), tag


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", [(48000, 44101, "VHQ"), (44101, 48000, "VHQ"), (48000, 44101, "HQ")], ids=lambda c: "%g-%g-%s" % c)
def test_ragged_mixed_table_mono(case, kind):
    _ragged_case(case, kind, 1)


@pytest.mark.parametrize("case", [(48000, 44101, "VHQ"), (44101, 48000, "VHQ")], ids=lambda c: "%g-%g-%s" % c)
def test_ragged_mixed_table_interleaved_stereo(case):
    _ragged_case(case, "f32", 2)


def test_ragged_switch_free_fallbacks_are_the_exact_adjoint():
    """A table no clip of which the form admits, and a plan without the form (MQ): ONE launch of the exact adjoint — the bits of
    the ragged KERNEL_ADJOINT launch."""
    import torch
    from soxr_amd import device as dev, dist
    gen = torch.Generator(device="cuda").manual_seed(14)
    for case, n_xs in (((48000, 44101, "VHQ"), (4000, 300, 8000)), ((48000, 44101, "MQ"), (20000, 9000))):
        plan = _plan(case)
        gys = [torch.randn(plan.out_len(n), device="cuda", generator=gen) for n in n_xs]
        got = _guarded(dist.resample_ragged_adjoint, plan, gys, n_xs, kernel=dev.KERNEL_ADJOINT_AUTO)
        want = _guarded(dist.resample_ragged_adjoint, plan, gys, n_xs, kernel=dev.KERNEL_ADJOINT)
        assert all(torch.equal(g, w) for g, w in zip(got, want)), case


# ---- autograd ------------------------------------------------------------------------------------------------------------------
def test_autograd_through_resample_ragged():
    import torch
    from soxr_amd import device as dev, dist
    K = dev.KERNEL_ADJOINT_AUTO
    plan = _plan((44101, 48000, "VHQ"))
    n_xs = [tp.smallest(plan) + 100, 4000, 300]
    for dt in (torch.float32, torch.float64):
        gen = torch.Generator(device="cuda").manual_seed(15)
        xs = [torch.randn(n, dtype=dt, device="cuda", generator=gen) for n in n_xs]
        xr = [x.clone().requires_grad_() for x in xs]
        ys = _guarded(dist.resample_ragged, plan, xr, grad_kernel=K)
        plain = dist.resample_ragged(plan, xs)
        assert all(y.grad_fn is not None and torch.equal(y.detach(), p) for y, p in zip(ys, plain))
        gys = [torch.randn(y.shape, dtype=dt, device="cuda", generator=gen) for y in ys]
        grads = _guarded(torch.autograd.grad, ys, xr, gys)
        direct = _guarded(dist.resample_ragged_adjoint, plan, gys, n_xs, kernel=K)
        for c, (g, d) in enumerate(zip(grads, direct)):
            assert torch.equal(g, d), (dt, c)
        # the first clip ran on the transposed two-stage form, the others on the exact adjoint
        exact = dist.resample_ragged_adjoint(plan, gys, n_xs, kernel=dev.KERNEL_ADJOINT)
        assert not torch.equal(direct[0], exact[0]) and torch.equal(direct[1], exact[1]) and torch.equal(direct[2], exact[2])
        # one double backward: the adjoint's own backward is the ragged forward under AUTO
        gyr = [g.clone().requires_grad_() for g in gys]
        ggx = [torch.randn(n, dtype=dt, device="cuda", generator=gen) for n in n_xs]
        gxs = _guarded(dist.resample_ragged_adjoint, plan, gyr, n_xs, kernel=K)
        _guarded(torch.autograd.backward, gxs, ggx)
        fwd = dist.resample_ragged(plan, ggx)
        for c, (g, f) in enumerate(zip(gyr, fwd)):
            assert torch.equal(g.grad, f), (dt, c)
    # ... and the equal-length surface takes the selector for grad_kernel: a short job and a long one through one value
    for n in (4000, tp.smallest(plan) + 7):
        x = torch.randn(n, device="cuda").requires_grad_()
        y = _guarded(dev.resample_tensor, plan, x, grad_kernel=K)
        gy = torch.randn_like(y)
        (g,) = _guarded(torch.autograd.grad, y, x, gy)
        assert torch.equal(g, _adj(plan, gy, n, K))


# ---- launch shape (debug-switch build, child processes) ---------------------------------------------------------------------
def _probe(tmp, mode, extra_env):
    assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
    env = {key: v for key, v in os.environ.items() if not key.startswith("HIPSOXR_")}
    env.update({"HIPSOXR_LIBRARY": DBG_LIB, "HIPSOXR_DEBUG_LAUNCH_LOG": str(tmp / ("launch_%s.log" % mode))})
    env.update(extra_env)
    r = subprocess.run([sys.executable, os.path.join(HERE, "_adjoint_auto_probe.py"), mode, str(tmp / ("results_%s.npz" % mode))], env=env,
                       capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        _stopped.append("probe %s exit status %d" % (mode, r.returncode))
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(tmp / ("results_%s.npz" % mode))


# a budget that holds the two smallest columns of the mixed table (8192 outputs or inputs: 2 x 8192 elements and the pads) and
# not a small one beside a large one (about 20000 frames: 37000 elements and more), nor two large ones: ranges {n0, n0 + 1},
# {about 20011}, {the truncated clip}
BUDGET_BYTES = 4 * 2 * 16900


@pytest.fixture(scope="module")
def shape(tmp_path_factory):
    return _probe(tmp_path_factory.mktemp("adjoint_auto"), "shape", {})


@pytest.fixture(scope="module")
def budget(tmp_path_factory):
    return _probe(tmp_path_factory.mktemp("adjoint_auto_budget"), "budget", {"HIPSOXR_DEBUG_POLY_MID_BUDGET": str(BUDGET_BYTES)})


def _kinds_of(log):
    lines = str(log).splitlines()
    poly = [ap.fields(ln) for ln in lines if ln.startswith("kernel=poly_adj ")]
    interp = [ap.fields(ln) for ln in lines if ln.startswith("kernel=adj_interp ")]
    fft = [ap.fields(ln) for ln in lines if ln.startswith("form=") or " form=" in ln]
    return lines, poly, interp, fft


@pytest.mark.parametrize("name", sorted(ap.DIRECTIONS))
def test_the_number_of_launches_does_not_depend_on_the_number_of_clips(shape, name):
    for clips in (8, 40):
        lines, poly, interp, fft = _kinds_of(shape["log_%s_%d" % (name, clips)])
        print("adjoint_auto launch log %s, %d clips:\n  %s" % (name, clips, "\n  ".join(lines)))
        assert len(poly) == 1 and poly[0].get("ragged") == "1", lines           # one range: one k_poly_adj launch, ragged
        assert len(fft) == 1 and fft[0]["form"] != "none" and "ragged" in fft[0], lines  # ... and one FFT-stage launch over the columns
        assert len(interp) == 1 and interp[0]["ragged"] == str(3 * clips // 8), lines   # the short clips: ONE k_adj_interp launch
        assert len(lines) == 3, lines
        assert int(poly[0]["cols"]) == 4 * clips // 8 and int(fft[0]["ragged"]) == 4 * clips // 8
        # the adjoint's order: the FFT stage's transposed plan first down (1:2), last up (2:1); the exact adjoint last
        up = name == "up"
        assert lines.index([ln for ln in lines if "form=" in ln][0]) == (1 if up else 0) and lines[2].startswith("kernel=adj_interp ")
        assert (int(fft[0]["L"]), int(fft[0]["M"])) == ((1, 2) if up else (2, 1)), fft


@pytest.mark.parametrize("name", sorted(ap.DIRECTIONS))
def test_a_table_cut_into_three_ranges_has_the_same_bits(shape, budget, name):
    lines, poly, interp, fft = _kinds_of(budget["log_%s_8" % name])
    print("adjoint_auto launch log %s, budget %d bytes:\n  %s" % (name, BUDGET_BYTES, "\n  ".join(lines)))
    assert len(poly) == 3 and len(fft) == 3 and len(interp) == 1 and len(lines) == 7, lines
    assert all(f.get("ragged") == "1" for f in poly) and [int(f["cols"]) for f in poly] == [2, 1, 1]
    whole, cut = shape["gx_%s" % name], budget["gx_%s" % name]
    same = np.array_equal(whole, cut)
    print("adjoint_auto %s: 3 ranges against 1: equal bits %s" % (name, same))
    assert same and whole.shape == cut.shape


def test_every_reachable_instance_is_launched_in_ragged_form(shape):
    seen = set()
    for taps, case in sorted(tp.COVER.items()):
        plan = _plan(case)
        for kind in KINDS:
            if kind == "f64" and taps > tp.F64_MAX_TAPS:
                continue
            lines, poly, interp, fft = _kinds_of(shape["log_%d_%s" % (taps, kind)])
            assert len(poly) == 1 and len(fft) == 1 and not interp and len(lines) == 2, lines
            f = poly[0]
            assert (int(f["T"]), int(f["width"]), f.get("ragged")) == (taps, 4 if kind == "f32" else 8, "1"), f
            assert int(f["R"]) in (1, 2, 4) and int(f["lds"]) <= 160 * 1024 and f["block"] == "256" and int(f["cols"]) == 1
            assert bool(shape["guards_%d_%s" % (taps, kind)]), "a guard element was written"
            seen.add((taps, kind))
            _check_values(case, kind, shape["got_%d_%s" % (taps, kind)], shape["ref_%d_%s" % (taps, kind)], "ragged instance T=%d %s" % (taps, kind))
    assert len(seen) == 8 + 6
