"""GPU: the ragged form of the transposed operator (csrc/adjoint.hip, `bool RAGGED`; hipsoxr_run_device_adjoint_ragged) and
the autograd pair around dist.resample_ragged.

All logged jobs run in ONE child process (tests/_adjoint_ragged_probe.py) on the debug-switch build, which writes one line
per launch; the interpolated-phase jobs run once more in a second child with the per-lane walk switched on.  The probe
makes the data (lengths are stated in units of Mc and of pb, which it reads from the launch log) and returns every buffer
as it lay in memory; everything is compared here.

Oracle 1 (bitwise): each clip of a ragged job equals the same clip run alone through device.resample_tensor_adjoint — or,
for the 65 600-clip jobs, the clips of one length as one equal-length batch.
Oracle 2: tests/adjoint_ref.scatter in float64 on the clips named per job, with the bounds of tests/test_gpu_adjoint.py —
float64 1e-13 |A|^T|gy|, float32 (Tt + 2) 2^-24 |A32|^T|gy| on the bank rounded to float32; interpolated-phase plans: the
dense matrix and the bounds of tests/test_gpu_adjoint_interp.py.
Memory guard: every buffer is pre-filled with a sentinel; one spare frame lies behind every clip of gx (so between clips
and behind the last) and must keep it."""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import adjoint_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DBG_LIB = os.path.join(os.path.dirname(HERE), "python-soxr_amd", "_variants", "dbg", "libhipsoxr.so")
SENTINEL = 12345.0
F32, F64 = "f32", "f64"
AUTO, EXACT, ADJOINT = 0, 6, 10

HQ = (48000, 44100, "HQ")
PRIME, TRIPLE = (9973, 12289, "QQ"), (16000, 48000, "QQ")  # (tests/test_gpu_adjoint_forms.py: no tile tables; Mc 22)
INTERP = (48000, 44101, "HQ")
INTERP_GEOMETRY = (216, 32, 200)  # taps, phase intervals, ceil(T L / M) + 1 (tests/test_gpu_adjoint_interp.py GEOMETRY)

# a clip is [a, b, c, cut]: n_x = a pb Mc + b Mc + c frames, n_y = out_len(n_x) - cut, or 0 where cut < 0
# {0, 1, Mc-1, 4Mc-1, 4Mc, pb Mc, pb Mc + 1, 3 pb Mc + 5} shuffled, the empty clip in the middle; the clip of 4 Mc frames has
# a truncated cotangent, the one of Mc - 1 frames none at all
TILE_SET = [[1, 0, 1, 0], [0, 0, 1, 0], [3, 0, 5, 0], [0, 4, -1, 0], [0, 0, 0, 0], [1, 0, 0, 0], [0, 1, -1, -1], [0, 4, 0, 3]]
# the same capped below 4 Mc
GATHER_SET = [[0, 4, -1, 0], [0, 0, 1, 0], [0, 4, -1, 0], [0, 4, -1, 0], [0, 0, 0, 0], [0, 4, -1, 0], [0, 1, -1, -1], [0, 4, -1, 3]]
PRIME_SET = [[0, 0, 12289, 0], [0, 0, 1, 0], [0, 0, 0, 0], [0, 0, 12290, 3], [0, 0, 700, 0], [0, 0, 700, -1]]
# around _native.ADJOINT_INTERP_TILE = 256: {0, 1, 255, 256, 257, 513}, then 255 without a cotangent and 513 truncated
INTERP_SET = [[0, 0, 257, 0], [0, 0, 1, 0], [0, 0, 513, 0], [0, 0, 0, 0], [0, 0, 256, 0], [0, 0, 255, 0], [0, 0, 255, -1], [0, 0, 513, 3]]
WRAP = 65600


def _job(name, case, dtype, ch, clips, kernel=AUTO, layout="packed", seed=None, expect=None, check=(), **kw):
    j = dict(name=name, case=list(case), dtype=dtype, ch=ch, clips=clips, kernel=kernel, layout=layout,
             seed=seed if seed is not None else 1000 + len(JOBS), solo="clip")
    j.update(kw)
    JOBS[name] = (j, expect or {}, tuple(check))


JOBS = {}  # name -> (job for the probe, {log field: value}, clips checked against oracle 2)
for _case, _tag in ((HQ, "hq"), (TRIPLE, "triple")):
    for _dt in (F32, F64):
        for _ch in (1, 2):
            _job("tile_%s_%s_%d" % (_tag, _dt, _ch), _case, _dt, _ch, TILE_SET, expect=dict(kernel="adj_tile", ragged=8),
                 check=range(8))
            _job("gather_%s_%s_%d" % (_tag, _dt, _ch), _case, _dt, _ch, GATHER_SET, expect=dict(kernel="adj_gather", ragged=8),
                 check=(0, 1, 6, 7))
_job("tile_hq_split3_f32", HQ, F32, 3, TILE_SET, layout="split", expect=dict(kernel="adj_tile", ragged=8, cg=1), check=(3, 7))
for _dt in (F32, F64):
    _job("prime_" + _dt, PRIME, _dt, 1, PRIME_SET, expect=dict(kernel="adj_gather", ragged=6), check=(1, 3, 4, 5))
    _job("prime_split3_" + _dt, PRIME, _dt, 3, PRIME_SET, layout="split", expect=dict(kernel="adj_gather", ragged=6), check=(0, 4))
_job("prime_strided_f32", PRIME, F32, 1, PRIME_SET, layout="strided", expect=dict(kernel="adj_gather", ragged=6), check=(4,))
_job("gather_hq_strided_f64_2", HQ, F64, 2, GATHER_SET, layout="strided", expect=dict(kernel="adj_gather", ragged=8), check=(0, 7))
for _dt in (F32, F64):
    for _ch in (1, 2):
        _job("interp_%s_%d" % (_dt, _ch), INTERP, _dt, _ch, INTERP_SET, kernel=ADJOINT, expect=dict(kernel="adj_interp", ragged=8),
             check=(0, 1, 4, 5, 6))
# more columns than gridDim.y holds: lengths cycling 0 .. 5, then the same with one clip of 91 frames (>= 4 Mc = 88: tiled)
_job("wrap_gather", TRIPLE, F32, 1, [[0, 0, i % 6, 0] for i in range(WRAP)], seed=77, solo="class",
     expect=dict(kernel="adj_gather", ragged=WRAP, gy=65535))
_job("wrap_tile", TRIPLE, F32, 1, [[0, 0, 91 if i == 40000 else i % 6, 0] for i in range(WRAP)], seed=77, solo="class",
     expect=dict(kernel="adj_tile", ragged=WRAP, gy=65535))
# a caller's device copy of the table against the uploaded one: the same job twice
_job("tabledev_hq_f32_2", HQ, F32, 2, TILE_SET, seed=JOBS["tile_hq_f32_2"][0]["seed"], table_dev=True, solo="none",
     expect=dict(kernel="adj_tile", ragged=8))
# one +inf in the clip of 4 Mc - 1 frames (clip 3: alone it would run the lane-per-element kernel)
_job("inf_tile_hq_f32_1", HQ, F32, 1, TILE_SET, seed=JOBS["tile_hq_f32_1"][0]["seed"], inf=[3], solo="none",
     expect=dict(kernel="adj_tile", ragged=8))
_job("inf_gather_hq_f64_1", HQ, F64, 1, GATHER_SET, seed=JOBS["gather_hq_f64_1"][0]["seed"], inf=[0], solo="none",
     expect=dict(kernel="adj_gather", ragged=8))
INTERP_JOBS = [n for n in JOBS if n.startswith("interp_")]

_child_failed = []  # a fault, abort or time limit in a child: nothing further is started on the GPU from this file


@pytest.fixture(autouse=True)
def _nothing_after_a_failed_child():
    if _child_failed:
        pytest.fail("the probe process failed (%s): no further GPU work from this file" % _child_failed[0])


@functools.lru_cache(maxsize=None)
def _plan(case):
    from soxr_amd import device as dev
    return dev.Plan(*case)


@functools.lru_cache(maxsize=None)
def _bank(case, f32):
    bank = _plan(case).bank()
    if f32:
        bank = bank.astype(np.float32).astype(np.float64)
    bank.setflags(write=False)
    return bank


def _run_probe(tmp, tag, jobs, extra_env):
    assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
    with open(tmp / (tag + ".json"), "w") as f:
        json.dump(jobs, f)
    env = {key: v for key, v in os.environ.items() if not key.startswith("HIPSOXR_")}
    env.update({"HIPSOXR_LIBRARY": DBG_LIB, "HIPSOXR_DEBUG_LAUNCH_LOG": str(tmp / (tag + ".log"))})
    env.update(extra_env)
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "_adjoint_ragged_probe.py"), str(tmp / (tag + ".json")),
                            str(tmp / (tag + ".npz"))], env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _child_failed.append("time limit")
        raise
    if r.returncode != 0:
        _child_failed.append("exit status %d" % r.returncode)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(tmp / (tag + ".npz"))


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("adjoint_ragged")


@pytest.fixture(scope="module")
def results(tmp):
    return _run_probe(tmp, "all", [j for j, _, _ in JOBS.values()], {})


@pytest.fixture(scope="module")
def lane_results(tmp, results):
    jobs = [dict(JOBS[n][0], solo="none") for n in INTERP_JOBS]
    return _run_probe(tmp, "lane", jobs, {"HIPSOXR_DEBUG_ADJ_INTERP_PER_LANE": "1"})


def _parse(log):
    assert log and log.count("\n") == 0, "one launch per ragged job: %r" % log
    f = dict(tok.split("=", 1) for tok in log.split())
    out = {k: (v if k in ("kernel", "walk") else int(v)) for k, v in f.items() if k != "grid"}
    out["gx"], out["gy"], out["gz"] = (int(v) for v in f["grid"].split("x"))
    return out


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _clips(name, res):
    """memory guard checked; -> [(gy [n_y, ch], gx [n_x, ch])] per clip, from the buffers as they lay in memory"""
    job = JOBS[name][0]
    ch, table = job["ch"], res["table_" + name]
    _, _, yf, yc, xf, xc = (int(v) for v in res["geom_" + name])
    gy, gx = res["gy_" + name], res["gx_" + name]
    assert gx.dtype == (np.float32 if job["dtype"] == F32 else np.float64)
    written = np.zeros(gx.shape, bool)
    out = []
    es = gx.itemsize
    for y0, n_y, x0, n_x in table:
        cy = np.lib.stride_tricks.as_strided(gy[y0:], (n_y, ch), (yf * es, yc * es)) if n_y else np.zeros((0, ch), gy.dtype)
        idx = x0 + np.arange(n_x)[:, None] * xf + np.arange(ch)[None, :] * xc
        assert not written[idx].any(), "the test's clips overlap"
        written[idx] = True
        out.append((np.array(cy), gx[idx]))
    spare = gx[~written]
    assert spare.size == ch * len(table), "one spare frame behind every clip"
    assert np.all(spare == SENTINEL), "an element between packed clips (or behind the last) was written"
    return out


def _solo(name, res):
    ch, table, flat = JOBS[name][0]["ch"], res["table_" + name], res["solo_" + name]
    out, pos = [], 0
    for n_x in table[:, 3]:
        out.append(flat[pos:pos + n_x * ch].reshape(n_x, ch))
        pos += n_x * ch
    assert pos == flat.size
    return out


@functools.lru_cache(maxsize=None)
def _interp_dense(kind, n_x):
    """tests/test_gpu_adjoint_interp.py _dense_n: the engine's own coefficients from the oracle's forward on unit impulses"""
    from oracle import oracle
    plan, pl = _plan(INTERP), oracle.plan(*INTERP)
    assert (plan.taps, plan.phases, math.ceil(plan.taps * plan.L / plan.M) + 1) == INTERP_GEOMETRY
    eye = np.eye(n_x, dtype=np.float32 if kind == F32 else np.float64)
    mode = "port_f32" if kind == F32 else "port_f64"
    A = np.stack([oracle.resample_channel(pl, eye[a], mode, bank=plan.bank()) for a in range(n_x)], axis=1).astype(np.float64)
    assert A.shape == (plan.out_len(n_x), n_x)
    return A


def _reference(case, kind, gy, n_x):
    """-> (A^T gy, bound) per element, gy [n_y, ch] (n_y may be short of out_len(n_x): a truncated cotangent)"""
    plan, g = _plan(case), gy.astype(np.float64)
    if g.shape[0] == 0:  # no cotangent: A^T gy is an empty sum, exactly 0 (adjoint_ref.scatter takes no empty gy)
        return np.zeros((n_x, g.shape[1])), np.zeros((n_x, g.shape[1]))
    if plan.phases:
        A = _interp_dense(kind, 257)[:g.shape[0], :n_x]  # (column a does not depend on the job's length)
        want, mag, terms = A.T @ g, np.abs(A).T @ np.abs(g), INTERP_GEOMETRY[2]
    else:
        want, mag = adjoint_ref.scatter(plan.L, plan.M, _bank(case, kind == F32), g, n_x)
        terms = math.ceil(plan.taps * plan.L / plan.M) + 1
    return want, (1e-13 * mag + 1e-300 if kind == F64 else (terms + 2) * 2.0 ** -24 * mag)


@pytest.mark.parametrize("name", [n for n in JOBS if JOBS[n][0]["solo"] == "clip"])
def test_each_clip_equals_the_clip_run_alone(results, name):
    job, expect, check = JOBS[name]
    case, kind = tuple(job["case"]), job["dtype"]
    plan = _plan(case)
    log = _parse(str(results["log_" + name]))
    print(name, "launch:", str(results["log_" + name]))
    assert {k: log[k] for k in expect} == expect, log
    assert log["width"] == (4 if kind == F32 else 8) and (log["L"], log["M"]) == (plan.L, plan.M)
    mc, pb = int(results["geom_" + name][0]), int(results["geom_" + name][1])
    table = results["table_" + name]
    longest = int(table[:, 3].max())
    if log["kernel"] == "adj_tile":  # the frame axis is sized by the longest clip; Mc and pb are the launcher's
        assert log["pb"] == pb and log["n_st"] == -(-mc // 16) and log["gx"] == -(-(-(-longest // mc)) // pb), (log, mc, pb)
        assert longest >= 4 * mc and sorted(table[:, 3])[:4] == [0, 1, mc - 1, 4 * mc - 1]
    elif log["kernel"] == "adj_gather":
        assert log["gx"] == -(-longest * job["ch"] // 256)
        assert not plan.phases and (case == PRIME or longest == 4 * mc - 1)
    else:
        assert log["walk"] == "union" and log["gx"] == -(-longest // log["tile"]) and log["gy"] == 8 * job["ch"]
    clips, solo = _clips(name, results), _solo(name, results)
    for c, ((gy, gx), alone) in enumerate(zip(clips, solo)):
        assert np.isfinite(gx).all(), "clip %d: an element was not written" % c
        assert np.array_equal(_bits(gx), _bits(alone.astype(gx.dtype))), "clip %d differs from the same clip run alone" % c
        if gy.shape[0] == 0:
            assert not gx.any() and not np.signbit(gx).any(), "clip %d has no cotangent: +0 everywhere" % c
    worst = 0.0
    for c in check:
        gy, gx = clips[c]
        if plan.phases and gx.shape[0] > 257:
            continue
        want, bound = _reference(case, kind, gy, gx.shape[0])
        err = np.abs(gx.astype(np.float64) - want)
        if err.size:
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (c, worst)
    print("adjoint ragged %s: clips %s against float64, worst error/bound %.4f" % (name, list(check), worst))


def test_interp_walks_agree(results, lane_results):
    for name in INTERP_JOBS:
        log = _parse(str(lane_results["log_" + name]))
        assert log["kernel"] == "adj_interp" and log["walk"] == "lane" and log["ragged"] == 8, log
        assert np.array_equal(lane_results["gy_" + name], results["gy_" + name])
        _clips(name, lane_results)  # (the guard)
        assert np.array_equal(_bits(lane_results["gx_" + name]), _bits(results["gx_" + name])), name


@pytest.mark.parametrize("name", ["wrap_gather", "wrap_tile"])
def test_more_columns_than_grid_y(results, name):
    job, expect, _ = JOBS[name]
    log = _parse(str(results["log_" + name]))
    print(name, "launch:", str(results["log_" + name]))
    assert {k: log[k] for k in expect} == expect, log
    table, gx, solo = results["table_" + name], results["gx_" + name], results["solo_" + name]
    n_x = table[:, 3]
    assert len(table) == WRAP > 65535 and (n_x[:65535] % 6 == np.arange(65535) % 6).sum() >= 65534
    start = np.concatenate([[0], np.cumsum(n_x)[:-1]])
    written = np.zeros(gx.shape, bool)
    for n in sorted(set(n_x)):  # one comparison per length class
        idx = np.flatnonzero(n_x == n)
        if n == 0:
            continue
        at = table[idx, 2][:, None] + np.arange(n)[None, :]
        written[at] = True
        assert np.array_equal(_bits(gx[at]), _bits(solo[start[idx][:, None] + np.arange(n)[None, :]])), "clips of %d frames" % n
        assert np.isfinite(gx[at]).all() and np.abs(gx[at]).max() > 0
    assert (~written).sum() == WRAP and np.all(gx[~written] == SENTINEL), "a spare frame was written"


def test_a_supplied_device_table_gives_the_same_bits(results):
    a, b = "tile_hq_f32_2", "tabledev_hq_f32_2"
    assert _parse(str(results["log_" + b]))["ragged"] == 8
    assert np.array_equal(results["table_" + a], results["table_" + b]) and np.array_equal(results["gy_" + a], results["gy_" + b])
    assert np.array_equal(_bits(results["gx_" + a]), _bits(results["gx_" + b]))


@pytest.mark.parametrize("base,name,clip", [("tile_hq_f32_1", "inf_tile_hq_f32_1", 3), ("gather_hq_f64_1", "inf_gather_hq_f64_1", 0)])
def test_non_finite_cotangent_stays_in_its_clip(results, base, name, clip):
    """csrc/adjoint.hip REACH, for the form the RAGGED launch took (compared exactly, multiplied through by L):
         k_adj_gather   -(T/2 + 2 M/L)      < a - k M/L <= T/2
         k_adj_tile     -(T/2 + 15 + 4 M/L) < a - k M/L <= T/2 + 15"""
    log = _parse(str(results["log_" + name]))
    assert {k: log[k] for k in JOBS[name][1]} == JOBS[name][1], log
    plan = _plan(HQ)
    L, M, H = plan.L, plan.M, plan.taps // 2
    assert np.array_equal(results["table_" + name], results["table_" + base])
    fin, inf = _clips(base, results), _clips(name, results)
    for c, ((gy0, gx0), (gy1, gx1)) in enumerate(zip(fin, inf)):
        if c != clip:
            assert np.array_equal(gy0, gy1) and np.array_equal(_bits(gx0), _bits(gx1)), "clip %d changed" % c
    (gy0, gx0), (gy1, gx1) = fin[clip], inf[clip]
    k = gy1.shape[0] // 2
    assert np.isposinf(gy1[k, 0]) and np.array_equal(np.delete(gy1, k, 0), np.delete(gy0, k, 0))
    off = np.arange(gx1.shape[0], dtype=np.int64) * L - k * M  # (a - k M/L) L
    below, above = ((H + 15) * L + 4 * M, (H + 15) * L) if log["kernel"] == "adj_tile" else (H * L + 2 * M, H * L)
    inside = (off > -below) & (off <= above)
    hit = ~np.isfinite(gx1[:, 0])
    print("non-finite %s: %d frames non-finite, documented reach %d of %d" % (name, hit.sum(), inside.sum(), hit.size))
    assert hit.any() and inside.any() and not inside.all()
    assert not hit[~inside].any(), "the non-finite sample spread past the documented reach"
    assert np.array_equal(_bits(gx1[~inside]), _bits(gx0[~inside]))


# ---------------------------------------------------------------------------------------------------------------------
# the Python surface: dist.resample_ragged_adjoint, dist.resample_ragged and autograd (the product build, this process)
# ---------------------------------------------------------------------------------------------------------------------
def _three(dtype, ch=2, grad=(True, True, True), seed=3):
    import torch
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, ch, dtype=dtype, generator=g).cuda().requires_grad_(r) for n, r in zip((700, 0, 1900), grad)]


def test_resample_ragged_without_grad_is_the_ragged_job():
    import torch
    from soxr_amd import device as dev, dist
    plan = _plan(HQ)
    clips = _three(torch.float64, grad=(False, False, False))
    ys = dist.resample_ragged(plan, clips, kernel=dev.KERNEL_EXACT)
    job = dist.RaggedJob(plan, clips, kernel=dev.KERNEL_EXACT)
    job.launch()
    assert [y.shape for y in ys] == [(plan.out_len(n), 2) for n in (700, 0, 1900)]
    assert all(y.grad_fn is None and torch.equal(y, w) for y, w in zip(ys, job.outputs()))
    req = [c.clone().requires_grad_() for c in clips]
    with torch.no_grad():
        ng = dist.resample_ragged(plan, req, kernel=dev.KERNEL_EXACT)
    assert all(y.grad_fn is None and torch.equal(y, w) for y, w in zip(ng, ys))
    gr = dist.resample_ragged(plan, req, kernel=dev.KERNEL_EXACT)
    assert all(y.grad_fn is not None and torch.equal(y.detach(), w) for y, w in zip(gr, ys))


def test_grad_is_the_ragged_adjoint_bit_for_bit():
    import torch
    from soxr_amd import device as dev, dist
    plan = _plan(HQ)
    clips = _three(torch.float64, grad=(True, True, False))
    ys = dist.resample_ragged(plan, clips, kernel=dev.KERNEL_EXACT)
    g = torch.Generator().manual_seed(9)
    gys = [torch.randn(y.shape, dtype=y.dtype, generator=g).cuda() for y in ys]
    torch.autograd.backward(ys, gys)
    want = dist.resample_ragged_adjoint(plan, gys, [700, 0, 1900])
    assert [w.shape for w in want] == [c.shape for c in clips] and all(w.grad_fn is None for w in want)
    assert torch.equal(clips[0].grad, want[0]) and clips[1].grad.shape == (0, 2)
    assert clips[2].grad is None  # no requires_grad, no grad
    for w, gy, n in zip(want, gys, (700, 0, 1900)):  # ... and each clip is the clip run alone
        assert torch.equal(w, dev.resample_tensor_adjoint(plan, gy, n))
    mono = [torch.randn(n, dtype=torch.float32, generator=g).cuda().requires_grad_() for n in (333, 5)]
    ym = dist.resample_ragged(plan, mono)
    assert [y.shape for y in ym] == [(plan.out_len(333),), (plan.out_len(5),)]
    (ym[0].sum() + 2 * ym[1].sum()).backward()
    ones = [torch.ones_like(ym[0]), 2 * torch.ones_like(ym[1])]
    wm = dist.resample_ragged_adjoint(plan, ones, [333, 5])
    assert all(torch.equal(m.grad, w) and m.grad.shape == m.shape for m, w in zip(mono, wm))


def test_gradcheck_and_double_backward():
    import torch
    from soxr_amd import device as dev, dist
    plan = _plan(HQ)
    g = torch.Generator().manual_seed(4)
    small = [torch.randn(n, 2, dtype=torch.float64, generator=g).cuda().requires_grad_() for n in (23, 0, 40)]
    fwd = lambda *cs: tuple(dist.resample_ragged(plan, list(cs), kernel=dev.KERNEL_EXACT))
    assert torch.autograd.gradcheck(fwd, tuple(small))
    assert torch.autograd.gradgradcheck(fwd, tuple(small))
    gys = [torch.randn(plan.out_len(n) - cut, 2, dtype=torch.float64, generator=g).cuda().requires_grad_()
           for n, cut in ((23, 0), (0, 0), (40, 3))]
    adj = lambda *gs: tuple(dist.resample_ragged_adjoint(plan, list(gs), [23, 0, 40]))
    assert torch.autograd.gradcheck(adj, tuple(gys))
    assert torch.autograd.gradgradcheck(adj, tuple(gys))


def test_dot_product_identity_f64():
    """<A x, g> = <x, A^T g> over the pair of ragged operators, clips (700, 0, 1900), stereo float64, to 1e-12 relative to
    sum |g| (|A| |x|) — the scale and the bound of tests/test_gpu_adjoint.py's identity."""
    import torch
    from soxr_amd import device as dev, dist
    plan = _plan(HQ)
    xs = _three(torch.float64, grad=(False, False, False))
    ys = dist.resample_ragged(plan, xs, kernel=dev.KERNEL_EXACT)
    g = torch.Generator().manual_seed(10)
    gys = [torch.randn(y.shape, dtype=y.dtype, generator=g).cuda() for y in ys]
    gxs = dist.resample_ragged_adjoint(plan, gys, [700, 0, 1900])
    for x, y, gy, gx in zip(xs, ys, gys, gxs):
        if x.shape[0] == 0:
            continue
        _, mag = adjoint_ref.scatter(plan.L, plan.M, _bank(HQ, False), gy.cpu().numpy(), x.shape[0])
        lhs, rhs = float((y * gy).sum()), float((x * gx).sum())
        assert abs(lhs - rhs) <= 1e-12 * float((x.abs().cpu().numpy() * mag).sum()), (lhs, rhs)


def test_dot_product_identity_f32_on_the_tile_form_job():
    """The float32 pair on the lengths of the tile-form job (Mc = 160, 64 periods per workgroup slab at most).  The forward
    is within (T + 2) 2^-24 |A32||x| of A32 x per element (T products and the output rounding), the adjoint within
    (Tt + 2) 2^-24 |A32|^T|g| of A32^T g — the bound of the float32 adjoint tests — so with the two dot products summed in
    float64 the identity holds to (T + Tt + 4) 2^-24 sum |x| (|A32|^T |g|)."""
    import torch
    from soxr_amd import device as dev, dist
    plan = _plan(HQ)
    mc, pb = 160, 64
    assert max(-(-16 // plan.M), -(-64 // plan.L)) * plan.M == mc
    lengths = [a * pb * mc + b * mc + c for a, b, c, _ in TILE_SET]
    g = torch.Generator().manual_seed(12)
    xs = [torch.randn(n, dtype=torch.float32, generator=g).cuda() for n in lengths]
    ys = dist.resample_ragged(plan, xs, kernel=dev.KERNEL_EXACT)
    gys = [torch.randn(y.shape, dtype=y.dtype, generator=g).cuda() for y in ys]
    gxs = dist.resample_ragged_adjoint(plan, gys, lengths)
    tt = math.ceil(plan.taps * plan.L / plan.M) + 1
    lhs = sum(float((y.double() * gy.double()).sum()) for y, gy in zip(ys, gys))
    rhs = sum(float((x.double() * gx.double()).sum()) for x, gx in zip(xs, gxs))
    scale = 0.0
    for x, gy in zip(xs, gys):
        if x.shape[0]:
            _, mag = adjoint_ref.scatter(plan.L, plan.M, _bank(HQ, True), gy.cpu().numpy(), x.shape[0])
            scale += float((np.abs(x.cpu().numpy().astype(np.float64)) * mag).sum())
    bound = (plan.taps + tt + 4) * 2.0 ** -24 * scale
    print("ragged dot-product identity f32: |lhs - rhs| / bound = %.4g" % (abs(lhs - rhs) / bound))
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


def test_interpolated_plan_needs_grad_kernel():
    import torch
    from soxr_amd import device as dev, dist
    interp = _plan(INTERP)
    g = torch.Generator().manual_seed(6)
    clips = [torch.randn(n, dtype=torch.float64, generator=g).cuda().requires_grad_() for n in (300, 0, 120)]
    with pytest.raises(RuntimeError, match="adjoint job: .*exact-bank"):  # when the forward is called
        dist.resample_ragged(interp, clips, kernel=dev.KERNEL_EXACT)
    with pytest.raises(RuntimeError, match="adjoint job: .*exact-bank"):
        dist.resample_ragged_adjoint(interp, [c.detach() for c in clips], [300, 0, 120])
    with pytest.raises(RuntimeError, match="adjoint job: .*float32 or float64"):
        dist.resample_ragged_adjoint(_plan(HQ), [torch.zeros(10, dtype=torch.int16, device="cuda")], [11])
    ys = dist.resample_ragged(interp, clips, kernel=dev.KERNEL_EXACT, grad_kernel=dev.KERNEL_ADJOINT)
    gys = [torch.randn(y.shape, dtype=y.dtype, generator=g).cuda() for y in ys]
    torch.autograd.backward(ys, gys)
    for c, gy in zip(clips, gys):
        assert torch.equal(c.grad, dev.resample_tensor_adjoint(interp, gy, c.shape[0], kernel=dev.KERNEL_ADJOINT))
