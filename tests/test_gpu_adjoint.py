"""GPU: the transposed polyphase operator (csrc/adjoint.hip, hipsoxr_run_device_adjoint) and the autograd pair around
resample_tensor.

Expected values come from the oracle's FORWARD: `oracle.resample_channel(pl, e_a, "ref", bank=Plan.bank())` on unit impulses
e_a gives the dense matrix A [n_y, n_x] in float64, and the expected gradient is A^T gy — the adjoint formula is not restated
here.

Kernel geometry the sizes below are chosen by (csrc/adjoint.hip): the period is replicated c = max(ceil(16 / M),
ceil(64 / L)) times (Mc = c M input frames); jobs of at least 4 Mc frames run on the period-tiled kernel, shorter ones on
the lane-per-element kernel; a workgroup tile of the tiled kernel is 64 Mc frames of one unit-stride column, or
floor(64 / channels) Mc frames of interleaved channels.
"""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (in_rate, out_rate, quality): VHQ and HQ for the first two pairs, LQ and QQ once each
CASES = [(48000, 44100, "VHQ"), (48000, 44100, "HQ"), (44100, 48000, "VHQ"), (44100, 48000, "HQ"), (1, 2, "LQ"),
         (2, 1, "HQ"), (16000, 48000, "QQ"), (44100, 16000, "VHQ"), (16000, 44100, "HQ")]


@functools.lru_cache(maxsize=None)
def _plan(case):
    from soxr_amd import device as dev
    return dev.Plan(*case)


def _mc(plan):
    return max(-(-16 // plan.M), -(-64 // plan.L)) * plan.M


def _lengths(case):
    plan = _plan(case)
    n = [1, 5, plan.taps // 2, plan.M + 3, 3 * plan.M + 7, 4 * _mc(plan) + 9]  # (the last: the period-tiled kernel)
    if case[:2] == (48000, 44100):
        n.append(701)
    return n


@functools.lru_cache(maxsize=None)
def _dense(case, n_x, f32):
    """A [n_y, n_x] float64 from the oracle's forward on unit impulses (f32: on the bank rounded to float32)."""
    from oracle import oracle
    plan, pl = _plan(case), oracle.plan(*case)
    bank = plan.bank()
    if f32:
        bank = bank.astype(np.float32).astype(np.float64)
    eye = np.eye(n_x)
    A = np.stack([oracle.resample_channel(pl, eye[a], "ref", bank=bank) for a in range(n_x)], axis=1)
    assert A.shape == (plan.out_len(n_x), n_x)
    A.setflags(write=False)
    return A


def _adjoint(plan, gy, n_x, **kw):
    import torch
    from soxr_amd import device as dev
    return dev.resample_tensor_adjoint(plan, torch.from_numpy(gy).cuda(), n_x, **kw).cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%g-%g-%s" % c)
def test_dense_parity_f64(case):
    plan, rng = _plan(case), np.random.default_rng(11)
    for n_x in _lengths(case):
        A = _dense(case, n_x, False)
        gy = rng.standard_normal(A.shape[0])
        gx = _adjoint(plan, gy, n_x)
        # unit roundoff 1.1e-16 times at most ~500 terms, whatever the summation order
        bound = 1e-13 * (np.abs(A).T @ np.abs(gy)) + 1e-300
        err = np.abs(gx - A.T @ gy)
        assert gx.shape == (n_x,) and (err <= bound).all(), (n_x, float((err / bound).max()))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%g-%g-%s" % c)
def test_dense_parity_f32(case):
    plan, rng = _plan(case), np.random.default_rng(12)
    tt = math.ceil(plan.taps * plan.L / plan.M) + 1
    worst = 0.0
    for n_x in _lengths(case):
        A = _dense(case, n_x, True)
        gy = rng.standard_normal(A.shape[0]).astype(np.float32)
        gx = _adjoint(plan, gy, n_x)
        assert gx.dtype == np.float32 and gx.shape == (n_x,)
        # any float32 summation order of at most Tt terms, plus the output rounding
        bound = (tt + 2) * 2.0 ** -24 * (np.abs(A).T @ np.abs(gy.astype(np.float64)))
        err = np.abs(gx.astype(np.float64) - A.T @ gy.astype(np.float64))
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        worst = max(worst, ratio)
        print("adjoint f32 error/bound %s n_x=%d: %.4f" % (case, n_x, ratio))
        assert (err <= bound).all(), (n_x, ratio)
    print("adjoint f32 worst error/bound %s: %.4f" % (case, worst))


def test_tile_edges_and_layouts():
    """48k -> 44.1k LQ, float64: Mc = 160, so a workgroup tile is 64 * 160 = 10240 frames of a unit-stride column and
    21 * 160 = 3360 frames of three interleaved channels; 31207 frames = three column tiles (nine interleaved ones) and a
    remainder of 487 frames, no multiple of M = 160."""
    import torch
    from oracle import oracle
    from soxr_amd import device as dev
    case = (48000, 44100, "LQ")
    plan, pl = _plan(case), oracle.plan(*case)
    assert _mc(plan) == 160
    tile, tile3, n_x = 10240, 3360, 3 * 10240 + 487
    n_y = plan.out_len(n_x)
    g = torch.Generator().manual_seed(5)
    gy = torch.randn(3, n_y, 3, dtype=torch.float64, generator=g).cuda()
    cols = torch.stack([torch.stack([dev.resample_tensor_adjoint(plan, gy[c, :, h].contiguous(), n_x) for h in range(3)], 1)
                        for c in range(3)])
    assert cols.shape == (3, n_x, 3)

    def guarded(gy_view):
        buf = torch.full((3, n_x + 16, 3), 777.0, dtype=torch.float64, device="cuda")
        buf[:, 8:-8] = float("nan")
        out = dev.resample_tensor_adjoint(plan, gy_view, n_x, out=buf[:, 8:-8])
        assert out.data_ptr() == buf[:, 8:-8].data_ptr()
        assert torch.isfinite(buf[:, 8:-8]).all()
        assert (buf[:, :8] == 777.0).all() and (buf[:, -8:] == 777.0).all()
        return buf[:, 8:-8]

    assert gy.is_contiguous()
    assert torch.equal(guarded(gy), cols)                                   # interleaved frames
    cf = gy.permute(0, 2, 1).contiguous().permute(0, 2, 1)                  # channel-first storage, viewed channel-last
    assert cf.stride(1) == 1 and torch.equal(cf, gy)
    assert torch.equal(guarded(cf), cols)
    big = torch.zeros(6, n_y, 3, dtype=torch.float64, device="cuda")
    big[::2] = gy
    assert big[::2].stride(0) == 2 * n_y * 3
    assert torch.equal(guarded(big[::2]), cols)                             # non-unit clip stride
    assert torch.equal(dev.resample_tensor_adjoint(plan, cf, n_x), cols)    # (and into a fresh tensor)

    # adjoint identity against the oracle's forward, column (0, 0)
    bank = plan.bank()
    gy0, gx0 = gy[0, :, 0].cpu().numpy(), cols[0, :, 0].cpu().numpy()
    rng = np.random.default_rng(6)
    xs = [rng.standard_normal(n_x) for _ in range(4)]
    edges = [0, n_x - 1] + [b * t + d for t in (tile, tile3) for b in range(1, n_x // t + 1) for d in (-1, 0)]
    for a in sorted(set(edges)):
        e = np.zeros(n_x)
        e[a] = 1.0
        xs.append(e)
    for x in xs:
        lhs = oracle.resample_channel(pl, x, "ref", bank=bank) @ gy0
        scale = oracle.resample_channel(pl, np.abs(x), "ref", bank=np.abs(bank)) @ np.abs(gy0)
        assert abs(lhs - x @ gx0) <= 1e-12 * scale, (lhs, x @ gx0, scale)


def test_truncated_cotangent():
    case, n_x = (48000, 44100, "HQ"), 701
    plan, A = _plan(case), _dense(case, 701, False)
    n_y = A.shape[0] - 5
    gy = np.random.default_rng(13).standard_normal(A.shape[0] + 1)
    gx = _adjoint(plan, gy[:n_y], n_x)
    bound = 1e-13 * (np.abs(A[:n_y]).T @ np.abs(gy[:n_y])) + 1e-300
    assert (np.abs(gx - A[:n_y].T @ gy[:n_y]) <= bound).all()
    with pytest.raises(RuntimeError, match="adjoint job: .*exceeds"):
        _adjoint(plan, gy, n_x)


def test_backward_is_the_column_sums():
    import torch
    from soxr_amd import device as dev
    case, n_x = (48000, 44100, "HQ"), 701
    plan, A = _plan(case), _dense(case, 701, False)
    x = torch.randn(n_x, dtype=torch.float64, device="cuda").requires_grad_()
    y = dev.resample_tensor(plan, x, kernel=dev.KERNEL_EXACT)
    assert y.grad_fn is not None and y.shape == (A.shape[0],)
    y.sum().backward()
    err = np.abs(x.grad.cpu().numpy() - A.sum(0))
    assert (err <= 1e-13 * np.abs(A).sum(0) + 1e-300).all()
    # float32, batch of interleaved channels, default engine choice: same gradient per column
    x3 = torch.randn(2, n_x, 3, device="cuda").requires_grad_()
    dev.resample_tensor(plan, x3).sum().backward()
    A32 = _dense(case, 701, True)
    tt = math.ceil(plan.taps * plan.L / plan.M) + 1
    err = np.abs(x3.grad.cpu().numpy().astype(np.float64) - A32.sum(0)[None, :, None])
    assert (err <= ((tt + 2) * 2.0 ** -24 * np.abs(A32).sum(0))[None, :, None]).all()


@pytest.mark.parametrize("case", [(2, 1, "LQ"), (48000, 44100, "HQ")], ids=lambda c: "%g-%g-%s" % c)
def test_gradcheck(case):
    import torch
    from soxr_amd import device as dev
    plan = _plan(case)
    x = torch.randn(48, 2, dtype=torch.float64, device="cuda").requires_grad_()
    fwd = lambda t: dev.resample_tensor(plan, t, kernel=dev.KERNEL_EXACT)
    assert torch.autograd.gradcheck(fwd, (x,))
    assert torch.autograd.gradgradcheck(fwd, (x,))
    n_y = plan.out_len(48)
    gy = torch.randn(n_y, 2, dtype=torch.float64, device="cuda").requires_grad_()
    adj = lambda t: dev.resample_tensor_adjoint(plan, t, 48)
    assert torch.autograd.gradcheck(adj, (gy,))
    assert torch.autograd.gradgradcheck(adj, (gy,))
    short = torch.randn(n_y - 3, 2, dtype=torch.float64, device="cuda").requires_grad_()
    assert torch.autograd.gradcheck(adj, (short,))  # truncated cotangent: the backward is the truncated forward


def test_without_grad_the_plain_path_runs():
    import torch
    from soxr_amd import device as dev
    plan = _plan((48000, 44100, "HQ"))
    x = torch.randn(4000, 2, device="cuda")
    y_plain = dev.resample_tensor(plan, x)
    assert y_plain.grad_fn is None and not y_plain.requires_grad
    xr = x.clone().requires_grad_()
    with torch.no_grad():
        y_ng = dev.resample_tensor(plan, xr)
    assert y_ng.grad_fn is None and torch.equal(y_ng, y_plain)
    y_g = dev.resample_tensor(plan, xr)
    assert y_g.grad_fn is not None and torch.equal(y_g.detach(), y_plain)
    g_plain = dev.resample_tensor_adjoint(plan, y_plain, 4000)
    assert g_plain.grad_fn is None


def test_determinism_and_bank_changes():
    import torch
    from soxr_amd import device as dev
    for dtype in (torch.float32, torch.float64):
        plan = dev.Plan(48000, 44100, "HQ")  # (a plan of its own: its bank is replaced below)
        n_x = 5 * 160 + 3
        gy = torch.randn(2, plan.out_len(n_x), 2, dtype=dtype, device="cuda")
        a, b = dev.resample_tensor_adjoint(plan, gy, n_x), dev.resample_tensor_adjoint(plan, gy, n_x)
        assert torch.equal(a, b)
        short = dev.resample_tensor_adjoint(plan, gy[:, :300], 333)  # (the lane-per-element kernel)
        plan.set_bank(2 * plan.bank())
        assert torch.equal(dev.resample_tensor_adjoint(plan, gy, n_x), 2 * a)
        assert torch.equal(dev.resample_tensor_adjoint(plan, gy[:, :300], 333), 2 * short)


def test_plans_come_and_go():
    """Twenty plans built, run and deleted: the transposed tables (about 6 MB per plan here) go with their plan."""
    import gc
    import torch
    from soxr_amd import device as dev

    gy = torch.randn(dev.Plan(16000, 44100, "VHQ").out_len(700), dtype=torch.float64, device="cuda")

    def once():
        plan = dev.Plan(16000, 44100, "VHQ")
        out = dev.resample_tensor_adjoint(plan, gy, 700)
        torch.cuda.synchronize()
        del plan
        gc.collect()
        return out

    first = once()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(20):
        assert torch.equal(once(), first)
    assert free0 - torch.cuda.mem_get_info()[0] < 32 << 20


def test_refusals_by_name():
    import torch
    from soxr_amd import _native, device as dev
    plan, interp = _plan((48000, 44100, "HQ")), dev.Plan(44100, 48001, "HQ")
    assert interp.phases
    x = torch.randn(2000, device="cuda").requires_grad_()
    with pytest.raises(RuntimeError, match="adjoint job: .*exact-bank"):  # at forward time, not in the middle of backward
        dev.resample_tensor(interp, x)
    with pytest.raises(RuntimeError, match="adjoint job: .*exact-bank"):
        dev.resample_tensor_adjoint(interp, torch.randn(100, device="cuda"), 100)
    with pytest.raises(RuntimeError, match="adjoint job: .*float32 or float64"):
        dev.resample_tensor_adjoint(plan, torch.zeros(100, dtype=torch.int16, device="cuda"), 200)
    with pytest.raises(ValueError, match="out="):
        dev.resample_tensor(plan, x, out=torch.empty(plan.out_len(2000), device="cuda"))
    gy, gx = torch.randn(plan.out_len(2000), device="cuda"), torch.full((2000,), 5.0, device="cuda")
    args = (gy.data_ptr(), gx.data_ptr(), _native.F32, 1, 1, gy.shape[0], 2000, (0, 1, 1), (0, 1, 1))
    table = np.array([0, gy.shape[0], 0, 2000], np.int64)
    with pytest.raises(RuntimeError, match="adjoint job: .*ragged"):
        plan.run_adjoint(*args, clip_table=table.ctypes.data)
    with pytest.raises(RuntimeError, match="adjoint job: .*AUTO or EXACT"):
        plan.run_adjoint(*args, kernel=_native.KERNEL_FFT)
    torch.cuda.synchronize()
    assert (gx == 5.0).all()  # a refusal never falls through to another path
    plan.run_adjoint(*args, kernel=_native.KERNEL_EXACT)
    assert torch.equal(gx, dev.resample_tensor_adjoint(plan, gy, 2000))
