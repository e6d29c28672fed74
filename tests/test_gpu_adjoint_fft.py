"""GPU: the adjoint on the frequency-domain engine (HIPSOXR_KERNEL_ADJOINT_FFT; csrc/adjoint_fft.hip): gx = A^T gy computed as
the forward float job of the plan's TRANSPOSED plan (L' = M, M' = L, the mirrored prototype) on the kernels KERNEL_FFT runs.

REFERENCE: the oracle's float64 direct form on the transposed bank — oracle.resample_channel(pt_like, gy, "ref", n_out=n_x,
bank=bank'), bank' built here by numpy from Plan.bank() — itself held to the dense A^T gy (A from the oracle's forward on unit
impulses) within 1e-13 |A|^T |gy|, the bound of tests/test_gpu_adjoint.py test_dense_parity_f64.  BARS: those of
tests/test_gpu_fft.py and test_gpu_fft_table.py for the same arithmetic — float32 1e-6 relative RMS and 4e-5 x RMS pointwise;
float64 2e-9 (VHQ) / 1e-6 (HQ: its -128 dB stop band aliases) relative RMS.

The jobs whose launch form is named run once, in a child process on the debug-switch build (tests/_adjoint_fft_probe.py):
the launch log's line carries the form, the row (k, hop_out) and L and M — the transposed plan's, i.e. the forward's swapped.
Every such job is written through out= into a buffer with 8 guard elements either side of every column, twice, to the same
bytes.  Lengths: 1, 7, T'/2, and one frame before, on and behind the kept run of one work item (a pair of blocks) of the row
taken, hop_out recomputed here from T' by fft.hip's rule; three items and a remainder."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import _adjoint_fft_probe as fp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DBG_LIB = os.path.join(os.path.dirname(HERE), "python-soxr_amd", "_variants", "dbg", "libhipsoxr.so")
REL32, POINT32 = 1e-6, 4e-5
REL64 = {"VHQ": 2e-9, "HQ": 1e-6}


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2))) if np.size(a) else 0.0


_PLANS = {}


def _plan(case):
    from soxr_amd import device as dev
    if case not in _PLANS:
        _PLANS[case] = dev.Plan(*case)
    return _PLANS[case]


_PT = {}


def _pt(case):
    """(pt_like, bank'): the transposed plan as the oracle reads one, bank' [M][T'] from the product's float64 bank"""
    if case not in _PT:
        plan = _plan(case)
        L, M, T = plan.L, plan.M, plan.taps
        Tt = fp.transposed_taps(L, M, T)
        g = plan.bank()[:, ::-1].T.reshape(-1)  # the prototype on the fine grid: g[u + L T/2], bank[p][j] = g(L (T/2 - 1 - j) + p)
        s, i = np.arange(M)[:, None], np.arange(Tt)[None, :]
        w = -(M * (Tt // 2 - 1 - i) + s) + L * (T // 2)  # bank'[s][i] = g'(M (T'/2 - 1 - i) + s), g'(u) = g(-u)
        bank_t = np.where((w >= 0) & (w < L * T), g[np.clip(w, 0, L * T - 1)], 0.0)
        assert np.count_nonzero(bank_t) == np.count_nonzero(g) and Tt % 8 == 0
        _PT[case] = (types.SimpleNamespace(L=M, M=L, T=Tt, phases=0), np.ascontiguousarray(bank_t))
    return _PT[case]


def _ref(case, gy, n_x):
    """gx [n_x] float64 for one column gy"""
    from oracle import oracle
    pt, bank_t = _pt(case)
    return oracle.resample_channel(pt, np.asarray(gy, np.float64), "ref", n_out=n_x, bank=bank_t)


def _bars(case, kind, got, ref, tag):
    err = got.astype(np.float64) - ref
    scale = _rms(ref)
    rel = _rms(err) / scale if scale else 0.0
    worst = float(np.abs(err).max()) / scale if scale else 0.0
    print("adjoint_fft %s: rel rms %.3g worst/rms %.3g" % (tag, rel, worst))
    assert got.shape == ref.shape
    if kind == "f32":
        assert rel <= REL32 and worst <= POINT32, (tag, rel, worst)
    else:
        assert rel <= REL64[case[2]], (tag, rel)


# ---------------------------------------------------------------------------------------------------------------------
# the child: parity lengths, layouts, ragged tables — with the launch log
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def results(tmp_path_factory):
    assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
    tmp = tmp_path_factory.mktemp("adjoint_fft")
    env = {key: v for key, v in os.environ.items() if not key.startswith("HIPSOXR_")}
    env.update({"HIPSOXR_LIBRARY": DBG_LIB, "HIPSOXR_DEBUG_LAUNCH_LOG": str(tmp / "launch.log")})
    r = subprocess.run([sys.executable, os.path.join(HERE, "_adjoint_fft_probe.py"), str(tmp / "results.npz")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(tmp / "results.npz")


def _payload(results, name, n_x):
    """guards intact, payload fully written, two runs the same bytes; -> (gy, gx) as [frames, columns] matrices"""
    gy, buf = results["gy_" + name], results["gx_" + name]
    assert buf.shape == (gy.shape[0], n_x + 2 * fp.GUARD, gy.shape[2]) and buf.dtype == gy.dtype
    assert np.all(buf[:, :fp.GUARD] == fp.POISON) and np.all(buf[:, -fp.GUARD:] == fp.POISON), "guard elements were written"
    assert np.isfinite(buf[:, fp.GUARD:-fp.GUARD]).all(), "a payload element was not written"
    assert bool(results["same_" + name]), "two runs of one job differ"
    cols = lambda t: t.transpose(1, 0, 2).reshape(t.shape[1], t.shape[0] * t.shape[2])
    return cols(gy), cols(buf[:, fp.GUARD:-fp.GUARD])


def _one_line(results, key):
    log = str(results[key])
    assert log and log.count("\n") == 0, "one launch per job: %r" % log
    return fp.fields(log)


@pytest.mark.parametrize("case", fp.PARITY, ids=lambda c: "%g-%g-%s" % c)
def test_reference_is_the_dense_transpose(case):
    """The oracle's direct form on the transposed bank IS A^T gy: against the dense matrix of the forward."""
    from oracle import oracle
    plan, pl = _plan(case), oracle.plan(*case)
    bank, rng = plan.bank(), np.random.default_rng(21)
    for n_x in (1, 5, plan.taps // 2, 3 * plan.M + 7):
        eye = np.eye(n_x)
        A = np.stack([oracle.resample_channel(pl, eye[a], "ref", bank=bank) for a in range(n_x)], axis=1)
        assert A.shape == (plan.out_len(n_x), n_x)
        gy = rng.standard_normal(A.shape[0])
        bound = 1e-13 * (np.abs(A).T @ np.abs(gy)) + 1e-300
        err = np.abs(_ref(case, gy, n_x) - A.T @ gy)
        assert (err <= bound).all(), (n_x, float((err / bound).max()))


@pytest.mark.parametrize("kind", ["f32", "f64"])
@pytest.mark.parametrize("case", fp.PARITY, ids=lambda c: "%g-%g-%s" % c)
def test_parity(results, case, kind):
    plan = _plan(case)
    tag = "par_%g_%g_%s_%s" % (case + (kind,))
    row = json.loads(str(results["row_" + tag]))
    Tt = fp.transposed_taps(plan.L, plan.M, plan.taps)
    # the row the engine took for the transposed plan, and its kept run by fft.hip's rule on T'
    assert row["form"] == "pair2" and row["hop_out"] == fp.hop_out(plan.M, plan.L, Tt, row["k"]) > 0, row
    assert row["lengths"] == fp.lengths(Tt, row["hop_out"])
    for n_x in row["lengths"]:
        name = "%s_%d" % (tag, n_x)
        f = _one_line(results, "log_" + name)
        assert (f["form"], int(f["L"]), int(f["M"]), f["kind"], f["window"]) == ("pair2", plan.M, plan.L, kind, "0"), f
        assert (int(f["k"]), int(f["hop_out"])) == (row["k"], row["hop_out"]), (f, row)
        assert int(f["n_blocks"]) == -(-n_x // row["hop_out"])
        gy, gx = _payload(results, name, n_x)
        _bars(case, kind, gx[:, 0], _ref(case, gy[:, 0], n_x), "%s n_x=%d" % (tag, n_x))


FORMS = {"pairs8": "strided2_cp", "strided3": "strided2_st", "planar5": "pair2", "block": "block"}


@pytest.mark.parametrize("name", list(fp.LAYOUTS))
def test_layouts_and_forms(results, name):
    case, kind, _, clips, ch, n_x = fp.LAYOUTS[name]
    plan = _plan(case)
    f = _one_line(results, "log_" + name)
    assert (f["form"], int(f["L"]), int(f["M"]), f["kind"]) == (FORMS[name], plan.M, plan.L, kind), f
    if name == "planar5":
        assert f["grid"].split("x")[1] == "5"
    gy, gx = _payload(results, name, n_x)
    assert gx.shape == (n_x, clips * ch)
    for c in range(clips * ch):
        _bars(case, kind, gx[:, c], _ref(case, gy[:, c], n_x), "%s column %d" % (name, c))


def test_ragged_one_launch(results):
    """Six mono clips of one launch: each within the bars of the reference and of the clip run alone, sentinels intact."""
    case = fp.RAGGED_CASE
    plan = _plan(case)
    f = _one_line(results, "rag_log")
    assert (f["form"], int(f["L"]), int(f["M"]), f["ragged"]) == ("pair2", plan.M, plan.L, "6"), f
    table, gy_all, gx_all = results["rag_table"], results["rag_gy"], results["rag_gx"]
    item = 2 * int(f["hop_out"])
    Tt = fp.transposed_taps(plan.L, plan.M, plan.taps)
    assert list(table[:, 3]) == [0, 1, Tt // 2, item - 1, item + 1, 3 * item + 5] and (table[:, [0, 2]] % 2 == 1).all()
    written = np.zeros(gx_all.shape, bool)
    for c, (go, n_y, xo, n_x) in enumerate(table):
        written[xo:xo + n_x] = True
        got = gx_all[xo:xo + n_x]
        if n_x == 0:
            continue
        ref = _ref(case, gy_all[go:go + n_y], n_x)
        _bars(case, "f32", got, ref, "ragged clip %d" % c)
        alone = results["rag_alone_%d" % c]
        assert _rms(got.astype(np.float64) - alone) <= REL32 * _rms(alone), c
    assert np.all(gx_all[~written] == fp.POISON), "an element between packed clips was written"
    assert np.isfinite(gx_all[written]).all()


def test_ragged_interleaved_stereo(results):
    case = fp.RAGGED_CASE
    plan = _plan(case)
    f = _one_line(results, "rag2_log")
    # (ragged=<columns>: 3 clips x 2 channels; channel pairs, as the forward takes an interleaved stereo table by name)
    assert (f["form"], int(f["L"]), int(f["M"]), f["kind"], f["ragged"]) == ("strided2_cp", plan.M, plan.L, "f64", "6"), f
    for c, n_x in enumerate(results["rag2_n"]):
        gy, gx, alone = results["rag2_gy_%d" % c], results["rag2_gx_%d" % c], results["rag2_alone_%d" % c]
        assert gx.shape == (n_x, 2)
        for col in range(2):
            _bars(case, "f64", gx[:, col], _ref(case, gy[:, col], int(n_x)), "stereo clip %d column %d" % (c, col))
        assert _rms(gx - alone) <= REL64[case[2]] * _rms(alone)


# ---------------------------------------------------------------------------------------------------------------------
# in this process, on the product build
# ---------------------------------------------------------------------------------------------------------------------
def _adjoint(plan, gy, n_x, **kw):
    import torch
    from soxr_amd import device as dev
    kw.setdefault("kernel", dev.KERNEL_ADJOINT_FFT)
    g = torch.from_numpy(gy).cuda() if isinstance(gy, np.ndarray) else gy
    return dev.resample_tensor_adjoint(plan, g, n_x, **kw)


def test_truncated_and_empty_cotangent():
    import torch
    case = (48000, 44100, "VHQ")
    plan, n_x, rng = _plan(case), 2500, np.random.default_rng(31)
    n_y = plan.out_len(n_x) - 700
    gy = rng.standard_normal(n_y)
    gx = _adjoint(plan, gy, n_x).cpu().numpy()
    _bars(case, "f64", gx, _ref(case, gy, n_x), "truncated cotangent")
    for dt in (torch.float32, torch.float64):
        out = torch.full((2, n_x + 16, 3), 5.0, dtype=dt, device="cuda")
        _adjoint(plan, torch.zeros((2, 0, 3), dtype=dt, device="cuda"), n_x, out=out[:, 8:-8])
        assert (out[:, 8:-8] == 0).all() and (out[:, :8] == 5.0).all() and (out[:, -8:] == 5.0).all()


def test_a_nan_stays_in_its_column():
    import torch
    plan, n_x = _plan((48000, 44100, "HQ")), 3100
    for dt in (torch.float32, torch.float64):
        gy = torch.randn(2, plan.out_len(n_x), 1, dtype=dt, device="cuda")
        clean = _adjoint(plan, gy, n_x)
        bad = gy.clone()
        bad[1, 1234, 0] = float("nan")
        got = _adjoint(plan, bad, n_x)
        assert torch.equal(got[0], clean[0]) and torch.isnan(got[1]).any()


@pytest.mark.parametrize("case", [(48000, 44100, "VHQ"), (44100, 48000, "HQ")], ids=lambda c: "%g-%g-%s" % c)
def test_agrees_with_the_exact_adjoint(case):
    import torch
    from soxr_amd import device as dev
    plan, n_x = _plan(case), 6000
    for dt, bar in ((torch.float32, REL32), (torch.float64, 2e-9 if case[2] == "VHQ" else 1e-6)):
        gy = torch.randn(2, plan.out_len(n_x), 2, dtype=dt, device="cuda")
        exact = dev.resample_tensor_adjoint(plan, gy, n_x, kernel=dev.KERNEL_AUTO).double().cpu().numpy()
        fast = _adjoint(plan, gy, n_x).double().cpu().numpy()
        rel = _rms(fast - exact) / _rms(exact)
        print("adjoint_fft vs exact adjoint %s %s: %.3g" % (case, dt, rel))
        assert 0 < rel <= bar


def test_a_custom_bank_is_honoured_and_the_transposed_plan_goes_with_the_tables():
    """pt is derived from Plan.bank: a bank installed from outside shows in the next gradient (twice the bank: twice every
    value, exactly — a power of two commutes with every rounding), the designed one brings the first result back, and
    plans come and go without leaving anything behind."""
    import torch
    from soxr_amd import device as dev
    n_x = 3000
    for dt in (torch.float32, torch.float64):
        plan = dev.Plan(48000, 44100, "HQ")  # (a plan of its own: the module's plans keep their banks)
        gy = torch.randn(plan.out_len(n_x), 2, dtype=dt, device="cuda")
        first = _adjoint(plan, gy, n_x)
        bank = plan.bank()
        plan.set_bank(2.0 * bank)
        assert torch.equal(_adjoint(plan, gy, n_x), 2.0 * first)
        assert torch.equal(dev.resample_tensor_adjoint(plan, gy, n_x), 2.0 * dev.resample_tensor_adjoint(dev.Plan(48000, 44100, "HQ"), gy, n_x))
        plan.set_bank(bank)
        assert torch.equal(_adjoint(plan, gy, n_x), first)
        torch.cuda.synchronize()
        del plan
    for _ in range(3):
        p = dev.Plan(44100, 48000, "VHQ")
        _adjoint(p, torch.randn(p.out_len(500), device="cuda"), 500)
        torch.cuda.synchronize()
        del p


def test_half_is_the_float32_job_rounded_once():
    import torch
    plan, n_x = _plan((48000, 44100, "VHQ")), 3000
    for dt in (torch.float16, torch.bfloat16):
        for shape in ((plan.out_len(n_x),), (plan.out_len(n_x), 2)):
            gy = torch.randn(shape, device="cuda").to(dt)
            got = _adjoint(plan, gy, n_x)
            want = _adjoint(plan, gy.float(), n_x).to(dt)
            assert got.dtype == dt and torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_autograd():
    import torch
    from soxr_amd import device as dev
    K = dev.KERNEL_ADJOINT_FFT
    plan, n = _plan((48000, 44100, "VHQ")), 5000
    x = torch.randn(n, 2, dtype=torch.float64, device="cuda")
    xr = x.clone().requires_grad_()
    y = dev.resample_tensor(plan, xr, kernel=dev.KERNEL_FFT, grad_kernel=K)
    assert y.grad_fn is not None
    gy = torch.randn_like(y)
    y.backward(gy)
    gx = dev.resample_tensor_adjoint(plan, gy, n, kernel=K)
    assert torch.equal(xr.grad, gx)
    # <A x, gy> = <x, A^T gy>: each product is within the float64 class (2e-9 relative RMS) of the exact one, so by
    # Cauchy-Schwarz the two inner products differ by at most the class times the norms
    lhs, rhs = float((y.detach() * gy).sum()), float((x * gx).sum())
    bound = 2e-9 * float(y.detach().norm() * gy.norm() + x.norm() * gx.norm())
    print("adjoint_fft dot test: |lhs - rhs| %.3g, bound %.3g" % (abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound
    # the double backward runs: the adjoint's own backward is the forward with KERNEL_FFT
    gyr = gy.clone().requires_grad_()
    ggx = torch.randn(n, 2, dtype=torch.float64, device="cuda")
    dev.resample_tensor_adjoint(plan, gyr, n, kernel=K).backward(ggx)
    assert torch.equal(gyr.grad, dev.resample_tensor(plan, ggx, kernel=dev.KERNEL_FFT))
    # ... and through the forward's grad_fn: d/d(gy) <A^T gy, ggx> = A ggx
    gy2 = gy.clone().requires_grad_()
    (g2,) = torch.autograd.grad(dev.resample_tensor(plan, xr, kernel=dev.KERNEL_FFT, grad_kernel=K), xr, gy2, create_graph=True)
    g2.backward(ggx)
    assert torch.equal(gy2.grad, gyr.grad)
    # without requires_grad nothing changes, and the defaults keep their bits
    assert dev.resample_tensor(plan, x, grad_kernel=K).grad_fn is None
    xe = x.clone().requires_grad_()
    dev.resample_tensor(plan, xe, kernel=dev.KERNEL_FFT).backward(gy)
    assert torch.equal(xe.grad, dev.resample_tensor_adjoint(plan, gy, n)) and not torch.equal(xe.grad, gx)


def test_ragged_autograd():
    import torch
    from soxr_amd import device as dev, dist
    K = dev.KERNEL_ADJOINT_FFT
    plan, ns = _plan((48000, 44100, "VHQ")), [3000, 1, 4507]
    clips = [torch.randn(n, dtype=torch.float64, device="cuda").requires_grad_() for n in ns]
    ys = dist.resample_ragged(plan, clips, kernel=dev.KERNEL_FFT, grad_kernel=K)
    packed = torch.randn(sum(y.shape[0] for y in ys), dtype=torch.float64, device="cuda")
    gys = list(torch.split(packed, [y.shape[0] for y in ys]))
    torch.autograd.backward(ys, gys)
    want = dist.resample_ragged_adjoint(plan, gys, ns, kernel=K)
    for c, w in zip(clips, want):
        assert torch.equal(c.grad, w)
    lhs = sum(float((y.detach() * g).sum()) for y, g in zip(ys, gys))
    rhs = sum(float((c.detach() * w).sum()) for c, w in zip(clips, want))
    bound = 2e-9 * sum(float(y.detach().norm() * g.norm() + c.detach().norm() * w.norm()) for y, g, c, w in zip(ys, gys, clips, want))
    assert abs(lhs - rhs) <= bound
    # the double backward: the ragged forward with KERNEL_FFT
    gr = [g.clone().requires_grad_() for g in gys]
    gxs = dist.resample_ragged_adjoint(plan, gr, ns, kernel=K)
    torch.autograd.backward(gxs, [torch.randn_like(g) for g in gxs])
    assert all(g.grad is not None and torch.isfinite(g.grad).all() for g in gr)


def test_refusals_by_name():
    import ctypes
    import torch
    from soxr_amd import _native, device as dev
    K = _native.KERNEL_ADJOINT_FFT
    plan, n_x = _plan((48000, 44100, "HQ")), 2000
    gy, gx = torch.randn(plan.out_len(n_x), device="cuda"), torch.full((n_x,), 5.0, device="cuda")
    args = (gy.data_ptr(), gx.data_ptr(), _native.F32, 1, 1, gy.shape[0], n_x, (0, 1, 1), (0, 1, 1))
    with pytest.raises(RuntimeError, match="ADJOINT_FFT.*HQ and VHQ only"):
        dev.Plan(48000, 44100, "MQ").run_adjoint(*args, kernel=K)
    interp = dev.Plan(48000, 44101, "HQ")
    with pytest.raises(RuntimeError, match="ADJOINT_FFT needs an exact-bank plan.*HIPSOXR_KERNEL_ADJOINT,"):
        interp.run_adjoint(*args, kernel=K)
    with pytest.raises(RuntimeError, match="ADJOINT_FFT needs an exact-bank plan"):  # ... at forward time
        dev.resample_tensor(interp, torch.randn(n_x, device="cuda").requires_grad_(), grad_kernel=K)
    with pytest.raises(RuntimeError, match="ADJOINT_FFT serves float32 or float64"):
        dev.resample_tensor_adjoint(plan, torch.zeros(100, dtype=torch.int16, device="cuda"), 200, kernel=K)
    j = _native.Job()
    j.in_, j.out, j.elem, j.kernel, j.n_clips, j.n_channels = gy.data_ptr(), gx.data_ptr(), _native.F32, K, 1, 1
    j.in_frame_stride = j.out_frame_stride = j.in_chan_stride = j.out_chan_stride = 1
    j.in_frames, j.out_frames, j.out_k0 = gy.shape[0], n_x, 3
    err = _native.lib.hipsoxr_run_device_adjoint(plan.handle, ctypes.byref(j), None)
    assert err and b"ADJOINT_FFT: whole cotangents only" in err
    table = np.array([0, gy.shape[0], 0, n_x], np.int64)
    with pytest.raises(RuntimeError, match="ADJOINT_FFT: a clip_table is served by hipsoxr_run_device_adjoint_ragged"):
        plan.run_adjoint(*args, kernel=K, clip_table=table.ctypes.data)
    # a ratio the engine has no form for (13 is not 7-smooth): unavailable — never the exact adjoint
    odd = dev.Plan(13000, 11000, "HQ")
    assert not odd.phases
    with pytest.raises(RuntimeError, match="ADJOINT_FFT.*unavailable for this plan or layout"):
        odd.run_adjoint(gy.data_ptr(), gx.data_ptr(), _native.F32, 1, 1, odd.out_len(n_x), n_x, (0, 1, 1), (0, 1, 1), kernel=K)
    # the forward entries do not know the selector
    y = torch.full((plan.out_len(n_x),), 5.0, device="cuda")
    with pytest.raises(RuntimeError, match="HIPSOXR_KERNEL_ADJOINT_FFT.*hipsoxr_run_device_adjoint"):
        dev.resample_tensor(plan, torch.randn(n_x, device="cuda"), out=y, kernel=K)
    torch.cuda.synchronize()
    assert (gx == 5.0).all() and (y == 5.0).all()  # a refusal never falls through to another path
    plan.run_adjoint(*args, kernel=K)
    assert torch.equal(gx, dev.resample_tensor_adjoint(plan, gy, n_x, kernel=K))
