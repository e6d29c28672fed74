"""GPU: the gradient of per-clip rates — hipsoxr_run_device_vr_ragged_adjoint, the transpose of the ragged variable-rate
launch, as ONE launch of the VR form of k_adj_interp (csrc/adjoint.hip; vr_adjoint_rules.h), and the Python surface on it
(dist.resample_varispeed_adjoint, dist.resample_varispeed(..., grad_kernel=KERNEL_ADJOINT)).  The parent has neither the
entry, the function nor the keyword: every test here fails there.

All GPU work runs in probe children (tests/_vr_ragged_adjoint_probe.py) on the debug-switch build, which writes one line per
launch: one child for everything on the product's walk (UNION), one with HIPSOXR_DEBUG_ADJ_INTERP_PER_LANE for the per-lane
walk.  A child that faults, aborts or runs into its time limit ends all GPU work of this file.

Expected values: the adjoint formula is not restated here.  For each (plan, ratio, width) the dense matrix A at N_DENSE = 777
frames comes from the ORACLE's forward on unit impulses (oracle.vr_run in port mode: on a unit impulse it returns the very
coefficient the engine multiplies by); a job of n_x frames and n_y cotangent samples uses A[:n_y, :n_x].  Ratios drawn at
random get a matrix of their clip's own size.
Bounds, per element (tests/test_gpu_adjoint_interp.py's, with the term count of a clip's own ratio):
    float64  1e-13 |A|^T |gy|;   float32  (terms + 2) 2^-24 |A32|^T |gy|,   terms = ceil(T / io_ratio) + 1
— one fma chain of at most `terms` products in the element's width; no column of A has more non-zeros than that (asserted).
Shapes: clip lengths 0, 1, 2, 33, 255, 256, 257, 513, 700 in scrambled order (tile = 256 frames: 257, 513 and 700 cross tile
seams; at ratio 0.5 with T = 216 a tile reads about 944 cotangent samples: chunk seams of 256 are crossed), ratios the plan's
maximum, 1.0, 0.9070294784580499, 0.5, 1.1 (1 - 2^-40) and random ones, n_y full and truncated by 7, by 1 and to 0, float32
and float64, mono, [frames, 2] and [frames, 3], cotangents cut from one buffer with gaps."""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from vr_sim import q64

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DBG_LIB = os.path.join(os.path.dirname(HERE), "python-soxr_amd", "_variants", "dbg", "libhipsoxr.so")
GAP, GUARD, POISON = 3, 8, 12345.0   # the probe's
F32, F64 = "f32", "f64"
NP = {F32: np.float32, F64: np.float64}
AUTO, ADJOINT = 0, 10
N_DENSE = 777

MAIN = (17600, 16000, "HQ")     # the largest io ratio: 1.1
STEEP = (48000, 44100, "VHQ")
TAPS = {MAIN: 216, STEEP: 296}
LENGTHS = [257, 0, 700, 1, 513, 33, 256, 2, 255]
# n_y = vr_out_len - cut ("all": no cotangent at all).  Cut by 7 and by 1 the last frames still lie within reach of the last
# sample; LONG_CUT leaves a tail of frames that no output reads
LONG_CUT = 300
CUTS = {0: [0, 0, 7, 0, 1, "all", 0, 0, 0], 1: [7, 0, 0, 0, 0, 0, 1, 0, "all"], 3: [0, 0, LONG_CUT, 0, "all", 7, 0, 0, 1]}


def _fixed(case):
    top = case[0] / case[1]
    return [top, 1.0, 0.9070294784580499, 0.5] + ([1.1 * (1 - 2.0 ** -40)] if case == MAIN else [])


def _cycle(case, shift, n=len(LENGTHS)):
    f = _fixed(case)
    return [f[(i + shift) % len(f)] for i in range(n)]


JOBS = {}  # env -> [job]; a table job's name says plan, type, channels and which ratios


def _table(envs, name, case, kind, ch, ratios, cuts, **kw):
    seed = 7000 + len(JOBS.get("union", []))   # (the same cotangents on both walks)
    for env in envs:
        j = dict(kind="table", name=name, case=list(case), dtype=kind, ch=ch, lengths=LENGTHS, ratios=ratios, cuts=cuts, seed=seed, kernel=ADJOINT)
        j.update(kw)
        if env == "lane":
            j.update(solo=False, mono=False, poke=[])
        JOBS.setdefault(env, []).append(j)


for _case, _tag in ((MAIN, "main"), (STEEP, "steep")):
    for _kind in (F32, F64):
        for _shift in (0, 1, 3):
            _table(("union", "lane") if _shift == 1 else ("union",), "%s_%s_1_s%d" % (_tag, _kind, _shift), _case, _kind, 1,
                   _cycle(_case, _shift), CUTS[_shift], solo=True, table_dev=_shift == 3, kernel=AUTO if _shift == 3 else ADJOINT)
for _kind in (F32, F64):
    _table(("union",), "main_%s_1_rnd" % _kind, MAIN, _kind, 1, [float(r) for r in np.random.default_rng(99).uniform(0.5, 1.1, len(LENGTHS))],
           [0, 0, LONG_CUT, 0, 7, 0, 0, 0, 1], solo=True)
    for _ch in (2, 3):
        _table(("union", "lane") if _ch == 3 else ("union",), "main_%s_%d_s1" % (_kind, _ch), MAIN, _kind, _ch, _cycle(MAIN, 1), CUTS[1],
               solo=True, mono=True)
# a NaN and an Inf at one gy[k]: [clip, k, value]; clip 1 is 700 frames at 0.5 (k = 601 sits at frame 300: its support crosses
# the tile seam at 256; k = 0: cut at the clip's start), clip 0 is 257 frames at 1.0 (k = 256: cut at the clip's end)
POKE_LENGTHS, POKES = [257, 700, 33], [[1, 601, "nan"], [1, 0, "inf"], [0, 256, "inf"], [2, 5, "nan"]]
for _kind in (F32, F64):
    JOBS["union"].append(dict(kind="table", name="poke_" + _kind, case=list(MAIN), dtype=_kind, ch=1, lengths=POKE_LENGTHS, ratios=[1.0, 0.5, 1.1],
                              cuts=[0, 0, 0], seed=31, kernel=ADJOINT, poke=POKES))
FOLD_RATIOS = _cycle(MAIN, 0, 7)
PY_LENGTHS, PY_RATIOS = [700, 33, 0, 257, 1], [0.9070294784580499, 1.1, 1.0, 0.5, 1.0]
JOBS["union"] += [dict(kind="fold", name="fold", case=list(MAIN), n_clips=65536, frames=3, ratios=FOLD_RATIOS, seed=77),
                  dict(kind="py", name="py", case=list(MAIN), lengths=PY_LENGTHS, ratios=PY_RATIOS, seed=55),
                  dict(kind="const", name="const")]
ENVS = {"union": {}, "lane": {"HIPSOXR_DEBUG_ADJ_INTERP_PER_LANE": "1"}}
# a child imports torch, designs two plans and runs a few hundred launches of at most 700 frames, each waited for (union: also
# one launch over 65536 clips and a gradcheck of 40 frames): seconds; the limits leave room for a cold start
TIMEOUT = {"union": 240, "lane": 120}

_child_failed = []  # a fault, abort or time limit in a child: nothing further is started on the GPU from this file
_results = {}


@pytest.fixture(autouse=True)
def _nothing_after_a_failed_child():
    if _child_failed:
        pytest.fail("a probe process failed (%s): no further GPU work from this file" % _child_failed[0])


@pytest.fixture(scope="module")
def run_env(tmp_path_factory):
    """-> the results of one environment's child process (started on first use, once)"""
    def get(env_name):
        if env_name in _results:
            return _results[env_name]
        if _child_failed:
            pytest.fail("a probe process failed (%s): no further GPU work from this file" % _child_failed[0])
        tmp = tmp_path_factory.mktemp("vr_ragged_adjoint_" + env_name)
        assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
        with open(tmp / "jobs.json", "w") as f:
            json.dump(JOBS[env_name], f)
        env = {key: v for key, v in os.environ.items() if not key.startswith("HIPSOXR_")}
        env.update({"HIPSOXR_LIBRARY": DBG_LIB, "HIPSOXR_DEBUG_LAUNCH_LOG": str(tmp / "launch.log")})
        env.update(ENVS[env_name])
        try:
            r = subprocess.run([sys.executable, os.path.join(HERE, "_vr_ragged_adjoint_probe.py"), str(tmp / "jobs.json"), str(tmp / "out.npz")],
                               env=env, capture_output=True, text=True, timeout=TIMEOUT[env_name])
        except subprocess.TimeoutExpired:
            _child_failed.append("%s: time limit" % env_name)
            raise
        if r.returncode != 0:
            _child_failed.append("%s: exit status %d" % (env_name, r.returncode))
        assert r.returncode == 0, r.stderr[-3000:]
        _results[env_name] = np.load(tmp / "out.npz")
        return _results[env_name]
    return get


# ---------------------------------------------------------------------------------------------------------------------
# expected values
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plan(case):
    from soxr_amd import device as dev
    plan = dev.Plan(*case, vr=True)
    assert plan.taps == TAPS[case] and plan.phases > 0
    return plan


@functools.lru_cache(maxsize=None)
def _oracle_plan(case):
    from oracle import oracle
    return oracle.VrPlan(*case)


def _terms(case, ratio):
    return math.ceil(TAPS[case] / ratio) + 1


@functools.lru_cache(maxsize=None)
def _dense_n(case, ratio, kind, n_x):
    """A [vr_out_len(n_x), n_x] float64 of the forward of n_x frames at `ratio`: column a is the oracle's forward on the
    unit impulse at frame a, in the width `kind`"""
    from oracle import oracle
    vp, n_y = _oracle_plan(case), _plan(case).vr_out_len(n_x, ratio)
    mode, one = "port_f32" if kind == F32 else "port_f64", np.ones(1)
    if n_x == 0 or n_y == 0:
        return np.zeros((n_y, n_x))
    A = np.stack([oracle.vr_run(vp, one, mode, n_y, 0, q64(ratio), 0, in_abs0=a) for a in range(n_x)], axis=1).astype(np.float64)
    assert (A != 0).sum(0).max() <= _terms(case, ratio), "a frame is read by more outputs than the bound counts terms"
    A.setflags(write=False)
    return A


def _dense(case, ratio, kind, n_y, n_x):
    assert n_x <= N_DENSE
    plan = _plan(case)
    assert n_y <= plan.vr_out_len(n_x, ratio)
    A = _dense_n(case, ratio, kind, N_DENSE if ratio in _fixed(case) else n_x)
    return A[:n_y, :n_x]


def _bound(case, ratio, kind, A, gy):
    mag = np.abs(A).T @ np.abs(gy.astype(np.float64))
    return (1e-13 if kind == F64 else (_terms(case, ratio) + 2) * 2.0 ** -24) * mag, mag


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize])


def _line(log):
    text = str(log)
    assert text and text.count("\n") == 0, "one launch for the whole table: %r" % text
    return dict(tok.split("=", 1) for tok in text.split())


def _job(env, name):
    return next(j for j in JOBS[env] if j.get("name") == name)


def _clips(res, name):
    """-> per clip (gy [n_y, ch], gx [n_x, ch], ratio), and the mask of the gx buffer's elements that belong to no clip"""
    table, gy, gx, ratios = res["table_" + name], res["gy_" + name], res["gx_" + name], res["ratios_" + name]
    ch = gy.shape[1]
    free = np.ones(gx.shape[0], bool)
    out = []
    for (go, n_y, xo, n_x), r in zip(table, ratios):
        assert go % ch == 0 and xo % ch == 0
        out.append((gy[go // ch:go // ch + n_y], gx[xo // ch:xo // ch + n_x], float(r)))
        assert free[xo // ch:xo // ch + n_x].all(), "the test's own table overlaps"
        free[xo // ch:xo // ch + n_x] = False
    assert free[:GUARD].all() and free[-GUARD:].all()
    return out, free


def _table_names(env, pred=lambda j: True):
    return [j["name"] for j in JOBS[env] if j.get("kind") == "table" and "poke" not in j["name"] and pred(j)]


# ---------------------------------------------------------------------------------------------------------------------
# 1, 3, 7: every clip of every table within the bound of A^T gy, on both walks; packed output; one launch
# ---------------------------------------------------------------------------------------------------------------------
def _check_table(res, env, name):
    from soxr_amd import _native
    job = _job(env, name)
    case, kind, ch = tuple(job["case"]), job["dtype"], job["ch"]
    plan = _plan(case)
    f = _line(res["log_" + name])
    assert f["kernel"] == "adj_interp" and f["vr"] == "1" and f["ragged"] == str(len(LENGTHS)) and f["walk"] == env
    assert (int(f["width"]), int(f["T"]), int(f["P"]), int(f["tile"])) == (NP[kind]().itemsize, plan.taps, plan.phases, _native.ADJOINT_INTERP_TILE)
    assert f["grid"] == "%dx%dx1" % (-(-max(LENGTHS) // _native.ADJOINT_INTERP_TILE), len(LENGTHS) * ch)
    clips, free = _clips(res, name)
    gx_buf = res["gx_" + name]
    assert gx_buf.dtype == NP[kind] and np.all(gx_buf[free] == POISON), "an element outside every clip's gx range was written"
    worst = 0.0
    for c, ((gy, gx, ratio), n_x, cut) in enumerate(zip(clips, job["lengths"], job["cuts"])):
        n_y = 0 if cut == "all" else max(0, plan.vr_out_len(n_x, ratio) - cut)
        assert gy.shape == (n_y, ch) and gx.shape == (n_x, ch)
        assert not np.any(gx == POISON) and np.isfinite(gx).all(), "a frame of clip %d was not written" % c
        A = _dense(case, ratio, kind, n_y, n_x)
        for k in range(ch):
            bound, mag = _bound(case, ratio, kind, A, gy[:, k])
            err = np.abs(gx[:, k].astype(np.float64) - A.T @ gy[:, k].astype(np.float64))
            if n_x:
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (name, c, k, float((err / np.maximum(bound, 1e-300)).max()))
            # a frame no output reads — the tail behind a truncated cotangent's reach, all of a clip without cotangent — is +0
            assert not _bits(gx[:, k])[mag == 0].any(), "a frame no cotangent sample reaches is not +0 by bits"
            if cut == LONG_CUT:
                assert n_y > 0 and (mag == 0).sum() >= 40 and (mag != 0).sum() >= 400, "this clip was to have an unread tail"
        if n_y == 0:
            assert not _bits(gx).any()
    print("vr ragged adjoint %s [%s]: worst error/bound %.4f" % (name, env, worst))
    return worst


@pytest.mark.parametrize("name", _table_names("union"))
def test_every_clip_is_within_the_bound_union_walk(run_env, name):
    _check_table(run_env("union"), "union", name)


@pytest.mark.parametrize("name", _table_names("lane"))
def test_every_clip_is_within_the_bound_per_lane_walk(run_env, name):
    res = run_env("lane")
    _check_table(res, "lane", name)
    # same terms in the same order either way: the walks agree by bits
    assert np.array_equal(res["gy_" + name], run_env("union")["gy_" + name])
    assert np.array_equal(_bits(res["gx_" + name]), _bits(run_env("union")["gx_" + name]))


def test_dense_slices_are_the_shorter_jobs():
    for case, ratio in ((MAIN, 0.5), (MAIN, 1.1), (STEEP, 0.9070294784580499)):
        for kind in (F32, F64):
            for n in (5, 40):
                n_y = _plan(case).vr_out_len(n, ratio)
                assert n_y > 0 and np.array_equal(_dense_n(case, ratio, kind, n), _dense_n(case, ratio, kind, N_DENSE)[:n_y, :n])


# ---------------------------------------------------------------------------------------------------------------------
# 2: bit identity
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _table_names("union", lambda j: j.get("solo")))
def test_each_clip_has_the_bits_of_the_clip_alone(run_env, name):
    res = run_env("union")
    clips, _ = _clips(res, name)
    solo, pos = res["solo_" + name], 0
    for c, (_, gx, _) in enumerate(clips):
        one = solo[pos:pos + gx.shape[0] + 2 * GUARD]
        pos += gx.shape[0] + 2 * GUARD
        assert np.all(one[:GUARD] == POISON) and np.all(one[-GUARD:] == POISON), "guard elements of the clip run alone were written"
        assert np.array_equal(_bits(one[GUARD:-GUARD]), _bits(gx)), "clip %d differs from the same clip in a table of its own" % c
    assert pos == solo.shape[0]


@pytest.mark.parametrize("name", _table_names("union", lambda j: j.get("mono")))
def test_each_interleaved_column_has_the_bits_of_the_column_run_mono(run_env, name):
    res = run_env("union")
    clips, _ = _clips(res, name)
    packed = np.concatenate([gx for _, gx, _ in clips])
    assert packed.shape[1] in (2, 3) and packed.shape == res["mono_" + name].shape
    assert np.array_equal(_bits(packed), _bits(res["mono_" + name]))


def test_auto_and_adjoint_are_the_same_launch():
    """the s3 tables run under HIPSOXR_KERNEL_AUTO with a caller's device table, the others under _ADJOINT with an uploaded one:
    all are held to the same bound above; here, that the selectors really differ in the jobs"""
    assert {_job("union", n)["kernel"] for n in _table_names("union")} == {AUTO, ADJOINT}


# ---------------------------------------------------------------------------------------------------------------------
# 4: the reach of a non-finite cotangent sample
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [F32, F64])
def test_a_non_finite_sample_changes_exactly_its_true_support(run_env, kind):
    res = run_env("union")
    name = "poke_" + kind
    table, base = res["table_" + name], res["gx_" + name]
    H = TAPS[MAIN] // 2
    assert np.isfinite(base[base != POISON]).all()
    for i, (c, k, what) in enumerate(POKES):
        got = res["poke_%s_%d" % (name, i)]
        _, n_y, xo, n_x = (int(v) for v in table[c])
        assert k < n_y
        q = (k * q64(float(res["ratios_" + name][c]))) >> 64
        lo, hi = max(0, q - (H - 1)), min(n_x, q + H + 1)   # frames q - (H - 1) .. q + H, clipped to [0, n_x)
        assert lo < hi
        hit = np.zeros(base.shape[0], bool)
        hit[xo + lo:xo + hi] = True
        assert not np.isfinite(got[hit]).any(), "a frame of the sample's support stayed finite (%s at clip %d, k = %d)" % (what, c, k)
        assert np.array_equal(_bits(got[~hit]), _bits(base[~hit])), "a frame outside the support changed (%s at clip %d, k = %d)" % (what, c, k)


# ---------------------------------------------------------------------------------------------------------------------
# 5, 6, 7: the Python surface
# ---------------------------------------------------------------------------------------------------------------------
def _split(flat, lengths):
    pos, out = 0, []
    for n in lengths:
        out.append(flat[pos:pos + n])
        pos += n
    assert pos == flat.shape[0]
    return out


def test_transpose_identity_against_the_product_s_forward(run_env):
    res = run_env("union")
    n_y = [int(n) for n in res["ny_py"]]
    assert n_y == [_plan(MAIN).vr_out_len(n, r) for n, r in zip(PY_LENGTHS, PY_RATIOS)]
    xs, ys, ws, gxs = (_split(res[k + "_py"], L) for k, L in (("x", PY_LENGTHS), ("y", n_y), ("w", n_y), ("gx", PY_LENGTHS)))
    for x, y, w, gx, n, r in zip(xs, ys, ws, gxs, PY_LENGTHS, PY_RATIOS):
        assert x.dtype == np.float64 and gx.dtype == np.float64
        A = _dense(MAIN, r, F64, len(y), n)
        scale = float(np.abs(w) @ (np.abs(A) @ np.abs(x)))
        lhs, rhs = float(y @ w), float(x @ gx)
        print("vr ragged adjoint transpose identity n_x=%d ratio=%g: |<Ax,w> - <x,A^T w>| / scale = %.3g" % (n, r, abs(lhs - rhs) / max(scale, 1e-300)))
        assert abs(lhs - rhs) <= 1e-12 * scale
    assert np.array_equal(_bits(res["gx_py"]), _bits(res["gxauto_py"])), "KERNEL_AUTO and KERNEL_ADJOINT differ"


def test_autograd(run_env):
    res = run_env("union")
    n_y = [int(n) for n in res["ny_py"]]
    idx = [int(i) for i in res["grad_idx_py"]]
    assert idx == [0, 2, 3, 4]
    assert np.array_equal(_bits(res["yg_py"]), _bits(res["y_py"])), "the forward with grad_kernel differs from the call without it"
    assert res["has_grad_fn_py"].all()
    want = np.concatenate([g for i, g in enumerate(_split(res["gx_py"], PY_LENGTHS)) if i in idx])
    assert np.array_equal(_bits(res["grad_py"]), _bits(want)), "autograd.grad is not resample_varispeed_adjoint on the weights"
    assert list(res["grad_none_py"]) == [i not in idx for i in range(len(PY_LENGTHS))], "a clip without requires_grad got a gradient"
    assert np.array_equal(_bits(res["gg_py"]), _bits(res["fwd_v_py"])), "the double backward is not the forward on the cotangent"
    assert np.array_equal(_bits(res["gop_py"]), _bits(res["fwd_v_py"])), "the operator's own backward is not the forward"
    assert len(res["fwd_v_py"]) == sum(n_y[i] for i in idx)
    assert bool(res["gradcheck_py"])


def test_launch_log_one_line_per_table_and_the_constant_rate_line_as_it_was(run_env):
    res = run_env("union")
    f = _line(res["log_py"])
    assert f["kernel"] == "adj_interp" and f["vr"] == "1" and f["ragged"] == str(len(PY_LENGTHS)) and f["walk"] == "union"
    b = _line(res["log_backward_py"])   # the backward of the whole batch: one launch of the same kernel
    assert b["kernel"] == "adj_interp" and b["vr"] == "1" and b["ragged"] == str(len(PY_LENGTHS))
    d = [ln for ln in str(res["log_double_py"]).split("\n") if ln.strip()]
    assert len(d) == 1 and "kernel=adj_" not in d[0] and " vr=1" in d[0], "the double backward is one forward launch: %r" % d
    text = str(res["log_const"])
    c = _line(text)
    assert c["kernel"] == "adj_interp" and "vr=" not in text and "ragged=" not in text
    assert list(c) == ["kernel", "width", "L", "M", "T", "P", "tile", "chunk", "lds", "walk", "grid", "block"], "the constant-rate line's fields"
    v = list(f)
    assert v[:12] == list(c) and v[12:] == ["vr", "ragged"]
    assert np.isfinite(res["gx_const"]).all() and res["gx_const"].shape == (300,)


# ---------------------------------------------------------------------------------------------------------------------
# 8: more columns than one grid holds
# ---------------------------------------------------------------------------------------------------------------------
def test_more_columns_than_grid_y(run_env):
    res = run_env("union")
    f = _line(res["log_fold"])
    assert f["kernel"] == "adj_interp" and f["vr"] == "1" and f["ragged"] == "65536" and f["grid"] == "1x65535x1"
    table, gy, gx = res["table_fold"], res["gy_fold"], res["gx_fold"].reshape(65536, 4)
    assert np.all(gx[:, 3] == POISON), "the element behind a clip was written"
    out = gx[:, :3]
    n_cls = len(FOLD_RATIOS)
    for cls, ratio in enumerate(FOLD_RATIOS):
        rows = out[cls::n_cls]
        assert np.array_equal(_bits(rows), np.broadcast_to(_bits(rows[:1]), rows.shape)), "a clip differs from clip 0 of its ratio class"
        go, n_y, _, n_x = (int(v) for v in table[cls])
        assert n_x == 3 and n_y == _plan(MAIN).vr_out_len(3, ratio) and n_y >= 2
        A = _dense(MAIN, ratio, F32, n_y, 3)
        g = gy[go:go + n_y]
        bound, _ = _bound(MAIN, ratio, F32, A, g)
        err = np.abs(rows[0].astype(np.float64) - A.T @ g.astype(np.float64))
        assert (err <= bound).all() and np.abs(rows[0]).max() > 0
    assert 65536 % n_cls != 0 and table.shape == (65536, 4)
