"""GPU: the adjoint of interpolated-phase plans (csrc/adjoint.hip k_adj_interp, HIPSOXR_KERNEL_ADJOINT) and the autograd
pair around resample_tensor(grad_kernel=KERNEL_ADJOINT).

Expected values come from the oracle's FORWARD on unit impulses: `oracle.resample_channel(pl, e_a, "port_f64",
bank=Plan.bank())` (and "port_f32" on float32 impulses) is bit-identical to the engine, and a unit impulse returns exactly
the coefficient the engine multiplies by — so A64 / A32 hold the engine's own coefficients and the only error left is
summation.  The adjoint formula is not restated here.  Column a of the matrix does not depend on the job's length (the
signal is zero outside it), so ONE matrix per (plan, width) is built at N_DENSE frames and a job of n_x frames uses
A[:out_len(n_x), :n_x] (test_dense_slices_are_the_shorter_jobs pins that).

Bounds, per element: float64 1e-13 |A64|^T|gy| (unit roundoff times at most 273 terms, with the margin of
tests/test_gpu_adjoint.py); float32 (terms + 2) 2^-24 |A32|^T|gy|, terms = ceil(T L / M) + 1 (any float32 summation order
of that many terms, plus the output rounding).

Kernel geometry the sizes are chosen by: a workgroup takes W = _native.ADJOINT_INTERP_TILE consecutive frames of one
column and walks the cotangent samples its frames read in chunks of `chunk` samples from the first one on (tile 0: from
k = 0); both are read back from the launch log of the debug-switch build (one child process for all logged jobs)."""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DBG_LIB = os.path.join(os.path.dirname(HERE), "python-soxr_amd", "_variants", "dbg", "libhipsoxr.so")
GUARD, POISON = 8, 12345.0
F32, F64 = "f32", "f64"
DTYPE = {F32: np.float32, F64: np.float64}

HQ, VHQ = (48000, 44101, "HQ"), (48000, 44101, "VHQ")
UP, DOWN = (8000, 44100.25, "LQ"), (44100.25, 8000, "LQ")  # 5.5x up (L = 176401, M = 32000) and down
# plan -> (taps, phase intervals, ceil(T L / M) + 1) from oracle/design.py
GEOMETRY = {HQ: (216, 32, 200), VHQ: (296, 128, 273), UP: (48, 16, 266), DOWN: (232, 16, 44)}
EXACT = (48000, 44100, "HQ")
N_DENSE = 777
SEAM_N = 100  # frames of the chunk-seam jobs: one tile, out_len = 551 cotangent samples on the 5.5x-up plan

_child_failed = []  # a fault, abort or time limit in the child: nothing further is started on the GPU from this file


@pytest.fixture(autouse=True)
def _nothing_after_a_failed_child():
    if _child_failed:
        pytest.fail("the probe process failed (%s): no further GPU work from this file" % _child_failed[0])


def _w():
    from soxr_amd import _native
    return _native.ADJOINT_INTERP_TILE


@functools.lru_cache(maxsize=None)
def _plan(case):
    from soxr_amd import device as dev
    plan = dev.Plan(*case)
    if case in GEOMETRY:
        assert plan.phases, "an interpolated-phase plan is what this file is about"
        assert (plan.taps, plan.phases, math.ceil(plan.taps * plan.L / plan.M) + 1) == GEOMETRY[case]
    return plan


def _terms(case):
    return GEOMETRY[case][2]


@functools.lru_cache(maxsize=None)
def _dense_n(case, n_x, kind):
    from oracle import oracle
    plan, pl = _plan(case), oracle.plan(*case)
    bank = plan.bank()
    eye = np.eye(n_x, dtype=DTYPE[kind])
    mode = "port_f32" if kind == F32 else "port_f64"
    A = np.stack([oracle.resample_channel(pl, eye[a], mode, bank=bank) for a in range(n_x)], axis=1).astype(np.float64)
    assert A.shape == (plan.out_len(n_x), n_x)
    assert (A != 0).sum(0).max() <= math.ceil(plan.taps * plan.L / plan.M) + 1
    A.setflags(write=False)
    return A


def _dense(case, n_x, kind):
    """A [n_y, n_x] float64: the engine's own coefficients in the width `kind`, from the oracle's forward on unit impulses"""
    assert n_x <= N_DENSE
    return _dense_n(case, N_DENSE, kind)[:_plan(case).out_len(n_x), :n_x]


def _bound(case, kind, A, gy):
    mag = np.abs(A).T @ np.abs(gy.astype(np.float64))
    return 1e-13 * mag + 1e-300 if kind == F64 else (_terms(case) + 2) * 2.0 ** -24 * mag


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _adjoint(plan, gy, n_x, **kw):
    import torch
    from soxr_amd import device as dev
    kw.setdefault("kernel", dev.KERNEL_ADJOINT)
    g = torch.from_numpy(gy).cuda() if isinstance(gy, np.ndarray) else gy
    return dev.resample_tensor_adjoint(plan, g, n_x, **kw).cpu().numpy()


def _lengths(case):
    W = _w()
    return [1, 5, GEOMETRY[case][0] // 2, W - 1, W, W + 1, 2 * W + 7, N_DENSE]


# ---------------------------------------------------------------------------------------------------------------------
# logged jobs: one child process on the debug-switch build
# ---------------------------------------------------------------------------------------------------------------------
def _make_jobs():
    rng = np.random.default_rng(5151)
    out = {}
    for case in GEOMETRY:
        for kind in (F32, F64):
            for n_x in _lengths(case):
                gy = rng.standard_normal((1, _plan(case).out_len(n_x), 1)).astype(DTYPE[kind])
                out["dense_%s_%d_%s" % ("-".join(str(c) for c in case), n_x, kind)] = (case, n_x, kind, gy)
    n_y = _plan(UP).out_len(SEAM_N)
    for kind in (F32, F64):
        gy3 = rng.standard_normal((1, n_y, 3)).astype(DTYPE[kind])
        out["seam3_" + kind] = (UP, SEAM_N, kind, gy3)
        for c in range(3):
            out["seam_col%d_%s" % (c, kind)] = (UP, SEAM_N, kind, np.ascontiguousarray(gy3[:, :, c:c + 1]))
    return out


@pytest.fixture(scope="module")
def jobs():
    """name -> (plan, n_x, type, gy [clips, n_y, channels])"""
    return _make_jobs()


@pytest.fixture(scope="module")
def results(jobs, tmp_path_factory):
    assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
    tmp = tmp_path_factory.mktemp("adjoint_interp")
    meta = [{"name": n, "case": list(case), "n_x": n_x} for n, (case, n_x, _, _) in jobs.items()]
    np.savez(tmp / "jobs.npz", meta=np.array(json.dumps(meta)), **{"gy_" + n: j[3] for n, j in jobs.items()})
    env = {key: v for key, v in os.environ.items() if not key.startswith("HIPSOXR_")}
    env.update({"HIPSOXR_LIBRARY": DBG_LIB, "HIPSOXR_DEBUG_LAUNCH_LOG": str(tmp / "launch.log")})
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "_adjoint_interp_probe.py"), str(tmp / "jobs.npz"),
                            str(tmp / "results.npz")], env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _child_failed.append("time limit")
        raise
    if r.returncode != 0:
        _child_failed.append("exit status %d" % r.returncode)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(tmp / "results.npz")


def _parse(log):
    assert log and log.count("\n") == 0, "one launch per job: %r" % log
    f = dict(tok.split("=", 1) for tok in log.split())
    out = {k: (v if k in ("kernel", "walk") else int(v)) for k, v in f.items() if k != "grid"}
    out["gx"], out["gy"], out["gz"] = (int(v) for v in f["grid"].split("x"))
    return out


def _payload(name, jobs, results):
    """guards checked, payload fully written; -> (gy, gx) as [frames, columns] matrices"""
    _, n_x, _, gy = jobs[name]
    buf = results["gx_" + name]
    assert buf.shape == (gy.shape[0], n_x + 2 * GUARD, gy.shape[2]) and buf.dtype == gy.dtype
    assert np.all(buf[:, :GUARD] == POISON) and np.all(buf[:, -GUARD:] == POISON), "guard elements were written"
    assert np.isfinite(buf[:, GUARD:-GUARD]).all(), "a payload element was not written"
    cols = lambda t: t.transpose(1, 0, 2).reshape(t.shape[1], t.shape[0] * t.shape[2])  # (n_y may be 0)
    return cols(gy), cols(buf[:, GUARD:-GUARD])


def _check_log(log, case, kind):
    plan = _plan(case)
    assert log["kernel"] == "adj_interp" and log["width"] == (4 if kind == F32 else 8)
    assert (log["L"], log["M"], log["T"], log["P"]) == (plan.L, plan.M, plan.taps, plan.phases)
    assert log["tile"] == _w() and log["chunk"] > 0 and log["block"] > 0 and 0 < log["lds"] <= 16 << 10


@pytest.mark.parametrize("kind", [F64, F32])
@pytest.mark.parametrize("case", list(GEOMETRY), ids=lambda c: "%g-%g-%s" % c)
def test_dense_parity(jobs, results, case, kind):
    worst = 0.0
    for n_x in _lengths(case):
        name = "dense_%s_%d_%s" % ("-".join(str(c) for c in case), n_x, kind)
        log = _parse(str(results["log_" + name]))
        _check_log(log, case, kind)
        assert (log["gx"], log["gy"]) == (-(-n_x // _w()), 1)
        gy, gx = _payload(name, jobs, results)
        A = _dense(case, n_x, kind)
        err = np.abs(gx[:, 0].astype(np.float64) - A.T @ gy[:, 0].astype(np.float64))
        bound = _bound(case, kind, A, gy[:, 0])
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        worst = max(worst, ratio)
        print("adjoint interp %s %s n_x=%d: error/bound %.4f" % (case, kind, n_x, ratio))
        assert (err <= bound).all(), (n_x, ratio)
    print("adjoint interp %s %s worst error/bound: %.4f" % (case, kind, worst))


@pytest.mark.parametrize("kind", [F64, F32])
def test_chunk_seams(jobs, results, kind):
    """5.5x up: a frame reads up to 266 cotangent samples.  The job is one tile, so its chunks start at k = 0, chunk,
    2 chunk, ...: frames whose samples lie either side of k = chunk sum across two staged chunks."""
    log3 = _parse(str(results["log_seam3_" + kind]))
    _check_log(log3, UP, kind)
    chunk = log3["chunk"]
    A = _dense(UP, SEAM_N, kind)
    assert A.shape[0] > chunk
    straddle = (A[:chunk] != 0).any(0) & (A[chunk:] != 0).any(0)
    assert straddle.sum() >= 8, "no frame of this job reads across a chunk seam: resize the job"
    gy3, gx3 = _payload("seam3_" + kind, jobs, results)
    assert log3["gy"] == 3
    for c in range(3):
        name = "seam_col%d_%s" % (c, kind)
        _check_log(_parse(str(results["log_" + name])), UP, kind)
        gy, gx = _payload(name, jobs, results)
        assert np.array_equal(gy[:, 0], gy3[:, c])
        err = np.abs(gx[:, 0].astype(np.float64) - A.T @ gy[:, 0].astype(np.float64))
        bound = _bound(UP, kind, A, gy[:, 0])
        print("adjoint interp seams %s column %d: error/bound %.4f (at the seam %.4f)"
              % (kind, c, float((err / bound).max()), float((err / bound)[straddle].max())))
        assert (err <= bound).all()
        assert np.array_equal(_bits(gx[:, 0]), _bits(gx3[:, c])), "an interleaved column differs from the same column run alone"


# ---------------------------------------------------------------------------------------------------------------------
# in this process, product build
# ---------------------------------------------------------------------------------------------------------------------
def test_dense_slices_are_the_shorter_jobs():
    for case in (HQ, UP):
        for kind in (F32, F64):
            assert np.array_equal(_dense_n(case, 5, kind), _dense(case, 5, kind))


@pytest.mark.parametrize("kind", [F64, F32])
def test_bit_identity(kind):
    import torch
    from soxr_amd import device as dev
    plan, n_x = _plan(HQ), 2 * _w() + 88
    n_y = plan.out_len(n_x)
    dt = torch.float64 if kind == F64 else torch.float32
    g = torch.Generator().manual_seed(21)
    col = torch.randn(n_y, dtype=dt, generator=g).cuda()
    K = dev.KERNEL_ADJOINT
    alone = dev.resample_tensor_adjoint(plan, col, n_x, kernel=K)
    assert plan.phases and alone.shape == (n_x,)
    assert torch.equal(dev.resample_tensor_adjoint(plan, col, n_x, kernel=K), alone)       # two runs of the same job
    batch = torch.randn(7, n_y, 1, dtype=dt, generator=g).cuda()
    batch[0, :, 0] = col
    assert torch.equal(dev.resample_tensor_adjoint(plan, batch, n_x, kernel=K)[0, :, 0], alone)
    wide = torch.randn(n_y, 5, dtype=dt, generator=g).cuda()
    wide[:, 3] = col
    assert torch.equal(dev.resample_tensor_adjoint(plan, wide, n_x, kernel=K)[:, 3], alone)
    big = torch.randn(3 * n_y + 1, dtype=dt, generator=g).cuda()
    big[1::3][:n_y] = col
    view = big[1::3][:n_y]
    assert view.stride(0) == 3 and torch.equal(dev.resample_tensor_adjoint(plan, view, n_x, kernel=K), alone)
    A = _dense(HQ, n_x, kind)
    gy = col.cpu().numpy()
    assert (np.abs(alone.cpu().numpy().astype(np.float64) - A.T @ gy.astype(np.float64)) <= _bound(HQ, kind, A, gy)).all()


def test_guards_truncation_and_unread_tail():
    import torch
    from soxr_amd import device as dev
    plan, n_x = _plan(HQ), 600
    n_full, n_short = plan.out_len(n_x), 200
    K = dev.KERNEL_ADJOINT
    A = _dense(HQ, n_x, F64)
    unread = ~(A[:n_short] != 0).any(0)  # frames no output below n_short reads
    assert unread.sum() > 100 and not unread[:200].any()
    gy = torch.randn(2, n_full, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(22)).cuda()

    def guarded(g):
        buf = torch.full((2, n_x + 16, 2), 777.0, dtype=torch.float64, device="cuda")
        buf[:, 8:-8] = float("nan")
        out = dev.resample_tensor_adjoint(plan, g, n_x, out=buf[:, 8:-8], kernel=K)
        assert out.data_ptr() == buf[:, 8:-8].data_ptr()
        assert torch.isfinite(buf[:, 8:-8]).all(), "a payload element was not written"
        assert (buf[:, :8] == 777.0).all() and (buf[:, -8:] == 777.0).all(), "guard elements were written"
        return buf[:, 8:-8].clone()

    full = guarded(gy)
    short = guarded(gy[:, :n_short])                      # a truncated cotangent ...
    ext = gy.clone()
    ext[:, n_short:] = 0
    assert torch.equal(short, guarded(ext))               # ... is the full job on the zero-extended one, bit for bit
    assert not torch.equal(short, full)
    tail = short.cpu().numpy()[:, unread]
    assert np.array_equal(_bits(tail), np.zeros_like(_bits(tail))), "a frame no output reads must come back +0"
    for c in range(2):
        for h in range(2):
            g1 = gy[c, :n_short, h].cpu().numpy()
            err = np.abs(short[c, :, h].cpu().numpy() - A[:n_short].T @ g1)
            assert (err <= _bound(HQ, F64, A[:n_short], g1)).all()
    with pytest.raises(RuntimeError, match="adjoint job: .*exceeds"):
        dev.resample_tensor_adjoint(plan, torch.zeros(n_full + 1, dtype=torch.float64, device="cuda"), n_x, kernel=K)


def test_transpose_of_the_gpu_forward_at_20000_frames():
    """<A x, gy> = <x, A^T gy> with A x from the exact engine's forward.  The scale <|A||x|, |gy|> is taken from the dense
    matrix of the job's first N_DENSE frames: a sum over a subset of the non-negative terms, so a smaller scale (a tighter
    bound) than the whole job's."""
    import torch
    from soxr_amd import device as dev
    plan, n_x = _plan(HQ), 20000
    n_y = plan.out_len(n_x)
    g = torch.Generator().manual_seed(23)
    x = torch.randn(n_x, dtype=torch.float64, generator=g).cuda()
    gy = torch.randn(n_y, dtype=torch.float64, generator=g).cuda()
    ax = dev.resample_tensor(plan, x, kernel=dev.KERNEL_EXACT).cpu().numpy()
    gx = dev.resample_tensor_adjoint(plan, gy, n_x, kernel=dev.KERNEL_ADJOINT).cpu().numpy()
    xh, gyh = x.cpu().numpy(), gy.cpu().numpy()
    A = _dense(HQ, N_DENSE, F64)
    scale = float((np.abs(A) @ np.abs(xh[:N_DENSE])) @ np.abs(gyh[:A.shape[0]]))
    lhs, rhs = math.fsum(ax * gyh), math.fsum(xh * gx)
    print("adjoint interp transpose: lhs %.17g rhs %.17g |lhs - rhs| = %.3e, bound %.3e" % (lhs, rhs, abs(lhs - rhs), 1e-12 * scale))
    assert np.abs(ax).max() > 0 and np.abs(gx).max() > 0
    assert scale > 0 and abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs, scale)


@pytest.mark.parametrize("kind", [F64, F32])
def test_non_finite_reach(kind):
    """One +inf / NaN at k = n_y // 2 reaches the frames a with a - H <= q_k <= a + H - 1 (q_k = k M div L) and nothing
    else: no padding, no 0 * inf."""
    plan, n_x = _plan(HQ), 2 * _w() + 88
    n_y, H = plan.out_len(n_x), plan.taps // 2
    base_gy = np.random.default_rng(24).standard_normal(n_y).astype(DTYPE[kind])
    base = _adjoint(plan, base_gy, n_x)
    assert np.isfinite(base).all()
    k = n_y // 2
    q_k = k * plan.M // plan.L
    a = np.arange(n_x)
    inside = (a - H <= q_k) & (q_k <= a + H - 1)
    support = _dense(HQ, n_x, kind)[k] != 0
    assert inside.sum() == plan.taps and not inside[0] and not inside[-1] and support.sum() > H and not (support & ~inside).any()
    for v in (np.inf, np.nan):
        gy = base_gy.copy()
        gy[k] = v
        gx = _adjoint(plan, gy, n_x)
        hit = ~np.isfinite(gx)
        assert hit[support].all(), "a frame whose support holds the non-finite sample is finite"
        assert not (hit & ~inside).any(), "the non-finite sample spread past its true support"
        assert np.array_equal(_bits(gx[~hit]), _bits(base[~hit])), "a finite frame changed"


def test_more_columns_than_grid_y():
    plan, n_x, cols = _plan(HQ), 5, 65600
    n_y = plan.out_len(n_x)
    gy = np.random.default_rng(25).standard_normal((cols, n_y, 1)).astype(np.float32)
    gx = _adjoint(plan, gy, n_x)
    assert gx.shape == (cols, n_x, 1)
    A = _dense(HQ, n_x, F32)
    g2 = gy[:, :, 0].astype(np.float64)
    err = np.abs(gx[:, :, 0].astype(np.float64) - g2 @ A)
    bound = (_terms(HQ) + 2) * 2.0 ** -24 * (np.abs(g2) @ np.abs(A))
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    assert np.abs(gx[-65:]).max() > 0  # (the columns behind gridDim.y = 65535)


def test_fresh_plan_adjoint_before_any_forward():
    from soxr_amd import device as dev
    for kind in (F64, F32):
        plan = dev.Plan(*HQ)  # (not the cached one: no forward has uploaded its interpolation table)
        A = _dense(HQ, 300, kind)
        gy = np.random.default_rng(26).standard_normal(A.shape[0]).astype(DTYPE[kind])
        gx = _adjoint(plan, gy, 300)
        assert (np.abs(gx.astype(np.float64) - A.T @ gy.astype(np.float64)) <= _bound(HQ, kind, A, gy)).all()


def test_exact_bank_plan_under_the_selector_has_auto_s_bits():
    import torch
    from soxr_amd import device as dev
    plan = _plan(EXACT)
    assert not plan.phases
    for dt in (torch.float32, torch.float64):
        for n_x in (600, 4000):  # the lane-per-element kernel, the period-tiled kernel
            gy = torch.randn(2, plan.out_len(n_x), 2, dtype=dt, device="cuda")
            auto = dev.resample_tensor_adjoint(plan, gy, n_x)
            assert torch.equal(dev.resample_tensor_adjoint(plan, gy, n_x, kernel=dev.KERNEL_ADJOINT), auto)


def test_gradcheck():
    import torch
    from soxr_amd import device as dev
    plan = _plan(HQ)
    x = torch.randn(300, dtype=torch.float64, device="cuda").requires_grad_()
    fwd = lambda t: dev.resample_tensor(plan, t, kernel=dev.KERNEL_EXACT, grad_kernel=dev.KERNEL_ADJOINT)
    assert torch.autograd.gradcheck(fwd, (x,))
    assert torch.autograd.gradgradcheck(fwd, (x,))


def test_backward_is_the_adjoint_and_the_plain_path_stays_plain():
    import torch
    from soxr_amd import device as dev
    plan, n = _plan(HQ), 6000
    x = torch.randn(n, 2, device="cuda")
    y_plain = dev.resample_tensor(plan, x, grad_kernel=dev.KERNEL_ADJOINT)  # without requires_grad: the plain path
    assert y_plain.grad_fn is None and not y_plain.requires_grad and torch.equal(y_plain, dev.resample_tensor(plan, x))
    xr = x.clone().requires_grad_()
    with torch.no_grad():
        assert dev.resample_tensor(plan, xr, grad_kernel=dev.KERNEL_ADJOINT).grad_fn is None
    y = dev.resample_tensor(plan, xr, grad_kernel=dev.KERNEL_ADJOINT)  # AUTO forward (the two-stage form at this size)
    assert y.grad_fn is not None and torch.equal(y.detach(), y_plain)
    gy = torch.randn_like(y)
    y.backward(gy)
    assert torch.equal(xr.grad, dev.resample_tensor_adjoint(plan, gy, n, kernel=dev.KERNEL_ADJOINT))
    with pytest.raises(RuntimeError, match="adjoint job: .*exact-bank"):  # the default still refuses, at forward time
        dev.resample_tensor(plan, xr)


def test_refusals_by_name():
    import torch
    from soxr_amd import _native, device as dev
    plan, K = _plan(HQ), _native.KERNEL_ADJOINT
    n_x = 2000
    gy, gx = torch.randn(plan.out_len(n_x), device="cuda"), torch.full((n_x,), 5.0, device="cuda")
    args = (gy.data_ptr(), gx.data_ptr(), _native.F32, 1, 1, gy.shape[0], n_x, (0, 1, 1), (0, 1, 1))
    with pytest.raises(RuntimeError, match="adjoint job: .*float32 or float64"):
        dev.resample_tensor_adjoint(plan, torch.zeros(100, dtype=torch.int16, device="cuda"), 200, kernel=K)
    with pytest.raises(RuntimeError, match="adjoint job: .*float32 or float64"):
        plan.run_adjoint(*((args[:2]) + (_native.I32,) + args[3:]), kernel=K)
    table = np.array([0, gy.shape[0], 0, n_x], np.int64)
    with pytest.raises(RuntimeError, match="adjoint job: .*ragged"):
        plan.run_adjoint(*args, kernel=K, clip_table=table.ctypes.data)
    vr = dev.Plan(48000, 44101, "HQ", vr=True)
    with pytest.raises(RuntimeError, match="adjoint job: .*variable-rate"):
        vr.run_adjoint(*args, kernel=K)
    with pytest.raises(RuntimeError, match="adjoint job: .*variable-rate"):
        dev.resample_tensor(vr, torch.randn(n_x, device="cuda").requires_grad_(), grad_kernel=K)
    # the forward entries do not know the selector
    y = torch.full((plan.out_len(n_x),), 5.0, device="cuda")
    x = torch.randn(n_x, device="cuda")
    with pytest.raises(RuntimeError, match="HIPSOXR_KERNEL_ADJOINT.*hipsoxr_run_device_adjoint only"):
        plan.run(x.data_ptr(), y.data_ptr(), _native.F32, 1, 1, n_x, y.shape[0], (0, 1, 1), (0, 1, 1), kernel=K)
    with pytest.raises(RuntimeError, match="HIPSOXR_KERNEL_ADJOINT.*hipsoxr_run_device_adjoint only"):
        dev.resample_tensor(plan, x, out=y, kernel=K)
    torch.cuda.synchronize()
    assert (gx == 5.0).all() and (y == 5.0).all()  # a refusal never falls through to another path
    plan.run_adjoint(*args, kernel=K)
    assert torch.equal(gx, dev.resample_tensor_adjoint(plan, gy, n_x, kernel=K))
