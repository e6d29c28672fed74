"""GPU: the two-stage form on a clip table — float32 / float64 clips of an interpolated-phase plan (Plan.phases != 0) under
KERNEL_AUTO with unit frame strides as a CONSTANT number of launches (csrc/twostage.hip launch_two_stage_ragged): one ragged
polyphase launch (k_poly<.., RAGGED>), one ragged FFT-stage launch, and one ragged launch of the exact engine's interpolated
kernels for the clips too short for the form — where the parent ran one polyphase launch and one FFT launch per admitted clip.

One child process per environment (tests/_ragged_two_stage_probe.py) on the debug-switch build, with a time limit of its own;
after a failed child nothing further is started from this file.  The probe makes the tables (nine clips, stated in units of the
polyphase tile U = 256 R of the job's own log line) and returns every buffer as it lay in memory; everything is compared here.

Environments: the default; HIPSOXR_DEBUG_POLY_R=1 (a tile is 256 outputs: the smallest admitted clip is 32 tiles and more,
so the persistent walk and the skip test work at the smallest admitted size); HIPSOXR_DEBUG_POLY_MID_BUDGET lowered (the range
cut: several launch pairs, the same bits).
Plans: 48000 -> 44101 (down: polyphase stage first, MQ 0), 44101 -> 48000 (up: FFT stage first, MQ 1), 44100 -> 16001 (down, MQ 1)
on HQ, float32; 48000 -> 44101 and 44101 -> 48000 on VHQ, float64.  (MQ = floor(Ms / Ls) of the polyphase stage is 0 or 1 for
every ratio the form takes: the MQ -1 instances are not reachable through a plan.  Each job's log line is checked for its MQ
and its tap count T.)  And, default environment only, one job for every other ragged instance a plan can launch — twenty (T, MQ,
type) in all, the census of tests/test_gpu_poly_instances.py; float64 on an HQ plan at 1e-6, its float32 form's bar.

Launch count (fails on the parent, which writes two lines per admitted clip and none with ragged=): exactly one kernel=poly
line with ragged=<admitted columns>, exactly one FFT line with the same ragged=, exactly one interp* line with ragged=<short
non-empty clips>; the poly grid is poly_grid_x of the longest clip over all columns.
Values: every admitted column on windows of 3000 outputs — head, tail, one interior tile edge — against the oracle's float64
direct form, relative RMS <= 1e-6 (float32) / 2e-9 (float64) of max(rms(ref), 0.05): the bars of tests/test_gpu_two_stage.py.
Short clips: bitwise equal to device.resample_tensor(..., kernel=KERNEL_EXACT) on the clip alone.
Memory: every element outside the clips' outputs (one spare frame behind every clip at the least) keeps the sentinel; no payload
element still holds it."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DBG_LIB = os.path.join(os.path.dirname(HERE), "python-soxr_amd", "_variants", "dbg", "libhipsoxr.so")
SENTINEL = 12345.0
NP = {"f32": np.float32, "f64": np.float64}
TOL = {"f32": 1e-6, "f64": 2e-9}
TOL_F64_HQ = 1e-6  # float64 on an HQ plan (a 20-bit recipe): the bar its float32 form meets on the same filter

DOWN, UP, STEEP = (48000, 44101), (44101, 48000), (44100, 16001)
CUT_BUDGET = 300000  # bytes of intermediate per range in the "cut" environment: two to four of the tables' columns

ENVS = {
    "default": {},
    "r1": {"HIPSOXR_DEBUG_POLY_R": "1"},
    "cut": {"HIPSOXR_DEBUG_POLY_MID_BUDGET": str(CUT_BUDGET)},
}
TIMEOUT = {"default": 240, "r1": 180, "cut": 120}

JOBS = {}  # (env, name) -> job for the probe (+ "mq", "t2": the MQ and the tap count T its poly line must show)


def _job(env, name, rates, quality, dtype, ch, layout, mq, seed=None, **kw):
    j = dict(name=name, case=[rates[0], rates[1], quality], dtype=dtype, ch=ch, layout=layout, mq=mq, seed=7000 + len(JOBS) if seed is None else seed)
    j.update(kw)
    JOBS[(env, name)] = j


_job("default", "down_f32_packed", DOWN, "HQ", "f32", 1, "packed", 0, t2=12)
_job("default", "up_f32_split2", UP, "HQ", "f32", 2, "split", 1, t2=20)
_job("default", "steep_f32_rows", STEEP, "HQ", "f32", 1, "rows", 1, t2=28)
_job("default", "down_f64_split2", DOWN, "VHQ", "f64", 2, "split", 0, t2=16)
_job("default", "up_f64_packed", UP, "VHQ", "f64", 1, "packed", 1, t2=28)
_job("r1", "down_f32_packed", DOWN, "HQ", "f32", 1, "packed", 0, t2=12)
_job("r1", "up_f32_split2", UP, "HQ", "f32", 2, "split", 1, t2=20)
_job("r1", "steep_f32_rows", STEEP, "HQ", "f32", 1, "rows", 1, t2=28)
_job("r1", "up_f64_packed", UP, "VHQ", "f64", 1, "packed", 1, t2=28)
# ... with 40 more clips of the smallest admitted size: 46 columns share the chip, so a column has fewer workgroups than tiles
_job("r1", "walk_f32_packed", DOWN, "HQ", "f32", 1, "packed", 0, t2=12, extra=40)
# the range cut: the default environment's jobs again (same seed, same table), the intermediate budget lowered
for _n in ("down_f32_packed", "up_f32_split2", "down_f64_split2"):
    _j = JOBS[("default", _n)]
    _job("cut", _n, _j["case"][:2], _j["case"][2], _j["dtype"], _j["ch"], _j["layout"], _j["mq"], seed=_j["seed"], t2=_j["t2"], solo_auto=False)

# every other ragged instance a plan can launch — k_poly<float | double, T, MQ, RAGGED> for the (T, MQ) and types that
# tests/test_gpu_poly_instances.py lists as reachable, whose census reads these jobs' log lines: the same table, layouts and checks
for _t2, _mq, _rates, _quality, _dtypes in (
        (16, 0, (48000, 44101), "VHQ", ("f32",)), (20, 0, (48000, 32001), "VHQ", ("f32", "f64")), (24, 0, (48000, 27941), "VHQ", ("f32", "f64")),
        (28, 0, (48000, 96734), "VHQ", ("f32", "f64")), (12, 0, (48000, 45887), "HQ", ("f64",)), (20, 1, (44101, 48000), "HQ", ("f64",)),
        (24, 1, (48000, 20962), "HQ", ("f32", "f64")), (32, 1, (44100, 12986), "HQ", ("f32", "f64")), (40, 1, (48000, 12986), "HQ", ("f32",)),
        (48, 1, (48000, 13983), "VHQ", ("f32",))):
    for _dtype in _dtypes:
        _job("default", "t%d_mq%d_%s" % (_t2, _mq, _dtype), _rates, _quality, _dtype, 1, "rows" if _t2 % 8 else "packed", _mq, t2=_t2)

PY_JOBS = [
    dict(kind="py_ragged", name="py_ragged", case=[DOWN[0], DOWN[1], "HQ"], seed=11, lengths=[9000, 150, 0, 12000, 8500], grad_lengths=[300, 0, 120]),
    dict(kind="py_batch", name="py_batch", case=[DOWN[0], DOWN[1], "HQ"], seed=12, lengths=[3000, 12000, 1, 9500, 20000]),
]

_child_failed = []  # a fault, abort or time limit in a child: nothing further is started on the GPU from this file
_results = {}


@pytest.fixture(autouse=True)
def _nothing_after_a_failed_child():
    if _child_failed:
        pytest.fail("a probe process failed (%s): no further GPU work from this file" % _child_failed[0])


def run_child(env_name, tmp_path_factory):
    """-> the results of one environment's child process (started on first use, once per session: tests/test_gpu_poly_instances.py
    reads the default child's log lines for its census)"""
    if env_name in _results:
        return _results[env_name]
    if _child_failed:
        pytest.fail("a probe process failed (%s): no further GPU work from this file" % _child_failed[0])
    tmp = tmp_path_factory.mktemp("ragged_two_stage_" + env_name)
    assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
    jobs = [dict(j) for (e, _), j in JOBS.items() if e == env_name]
    if env_name == "cut":  # the uncut job's own table: its tile size (a launch over fewer columns may pick another R)
        for j in jobs:
            j["u"] = int(run_child("default", tmp_path_factory)["geom_" + j["name"]][0])
    with open(tmp / "jobs.json", "w") as f:
        json.dump(jobs + (PY_JOBS if env_name == "default" else []), f)
    env = {key: v for key, v in os.environ.items() if not key.startswith("HIPSOXR_")}
    env.update({"HIPSOXR_LIBRARY": DBG_LIB, "HIPSOXR_DEBUG_LAUNCH_LOG": str(tmp / "launch.log")})
    env.update(ENVS[env_name])
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "_ragged_two_stage_probe.py"), str(tmp / "jobs.json"), str(tmp / "out.npz")],
                           env=env, capture_output=True, text=True, timeout=TIMEOUT[env_name])
    except subprocess.TimeoutExpired:
        _child_failed.append("%s: time limit" % env_name)
        raise
    if r.returncode != 0:
        _child_failed.append("%s: exit status %d" % (env_name, r.returncode))
    assert r.returncode == 0, r.stderr[-3000:]
    print("ragged two-stage child %s: %d jobs, %.1f s (time limit %d s)" % (env_name, len(jobs), time.time() - t0, TIMEOUT[env_name]))
    _results[env_name] = np.load(tmp / "out.npz")
    return _results[env_name]


@pytest.fixture(scope="module")
def run_env(tmp_path_factory):
    """-> the results of one environment's child process (started on first use, once)"""
    return lambda env_name: run_child(env_name, tmp_path_factory)


def _lines(log):
    return [dict(tok.split("=", 1) for tok in ln.split()) for ln in str(log).split("\n") if ln.strip()]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize])


def _rms(v):
    return float(np.sqrt(np.mean(np.square(v, dtype=np.float64))))


def _admitted(row):
    return min(int(row[1]), int(row[3])) >= 8192


def _clips(key, res):
    """memory guard checked; -> [(x [n_in, ch], y [out_frames, ch])] per clip, from the buffers as they lay in memory"""
    job = JOBS[key]
    name, ch, table = job["name"], job["ch"], res["table_" + job["name"]]
    _, _, _, xc, yc, _ = (int(v) for v in res["geom_" + name])
    x, y = res["x_" + name], res["y_" + name]
    assert y.dtype == NP[job["dtype"]]
    written = np.zeros(y.shape, bool)
    out = []
    for x0, n_in, y0, n_out in table:
        xi = x0 + np.arange(n_in)[:, None] + np.arange(ch)[None, :] * xc
        yi = y0 + np.arange(n_out)[:, None] + np.arange(ch)[None, :] * yc
        assert not written[yi].any(), "the test's clips overlap"
        written[yi] = True
        out.append((x[xi], y[yi]))
    for x0, n_in, y0, n_out in table:  # one spare frame behind every clip's columns
        assert not any(written[y0 + n_out + c * yc] for c in range(ch)), "the test's table leaves no spare frame"
    spare = y[~written]
    assert np.all(spare == SENTINEL), "an element outside the clips' outputs was written"
    for c, (_, yv) in enumerate(out):
        assert not np.any(yv == SENTINEL), "%s clip %d: a payload element was not written" % (key, c)
    return out


def _pad(job, t2):
    """poly_rules.h two_stage_mid: the intermediate runs `pad` samples past both ends — the polyphase half-width in samples of the
    intermediate (T2 / 2 up; T2 / 2 * Ls / Ms = T2 / 2 * 2 f_out / f_in down) + 4, rounded up to a multiple of 8"""
    fi, fo = job["case"][0], job["case"][1]
    half = t2 / 2 if fo > fi else t2 / 2 * (2 * fo / fi)
    return (int(np.ceil(half)) + 4 + 7) // 8 * 8


def _n_mid(job, row, t2):
    """the intermediate of a column: 2 n + 2 pad up; down 2 n_out' + 2 pad, n_out' the outputs it is sized for — the clip's own, or,
    truncated below the plan's output length, as far past them as the FFT stage's filter reaches (a quarter of its taps, hundreds:
    the 7 outputs these tables truncate by lie well inside), the plan's output length at the most (poly_rules.h two_stage_mid_outputs)"""
    fi, fo = job["case"][0], job["case"][1]
    if fo > fi:
        return 2 * int(row[1]) + 2 * _pad(job, t2)
    g = int(np.gcd(fi, fo))
    full = (2 * int(row[1]) * (fo // g) + fi // g) // (2 * (fi // g))
    assert 0 <= full - int(row[3]) <= 7
    return 2 * full + 2 * _pad(job, t2)


def _grid_x(tiles, per_cu, n_cu, cols):
    """poly_rules.h poly_grid_x"""
    gx = min(tiles, max(1, max(per_cu, 1) * n_cu // cols))
    return gx & ~7 if gx > 8 else gx


def _ids(keys):
    return ["%s-%s" % k for k in keys]


_ALL = list(JOBS)
_UNCUT = [k for k in JOBS if k[0] != "cut"]


def _check_launches(key, res, pairs):
    """the job's log: `pairs` polyphase + FFT launch pairs (one per range of columns), one interp* launch; -> the poly lines"""
    job = JOBS[key]
    name, ch, table = job["name"], job["ch"], res["table_" + job["name"]]
    u, m, _, _, _, n_cu = (int(v) for v in res["geom_" + name])
    lines = _lines(res["log_" + name])
    poly = [f for f in lines if f.get("kernel") in ("poly", "poly2")]
    fft = [f for f in lines if "form" in f]
    interp = [f for f in lines if str(f.get("kernel", "")).startswith("interp")]
    assert len(poly) + len(fft) + len(interp) == len(lines), lines
    admitted = [r for r in table if _admitted(r)]
    short = [r for r in table if r[3] > 0 and not _admitted(r)]
    extra = int(job.get("extra", 0))
    assert len(admitted) == 6 + extra and len(short) == 2 and len(table) == 9 + extra, "the probe's table: six admitted clips (+ extra), two short ones, one empty"
    assert len(poly) == pairs and len(fft) == pairs, "a constant number of launches: %r" % str(res["log_" + name])
    assert all(f["kernel"] == "poly" for f in poly), "k_poly2 has no ragged form"
    assert [f["ragged"] for f in poly] == [f["ragged"] for f in fft], (poly, fft)
    assert sum(int(f["ragged"]) for f in poly) == len(admitted) * ch
    assert all(f["form"] != "none" and f["window"] == "0" for f in fft), fft
    assert len(interp) == 1 and interp[0]["ragged"] == str(len(short)), interp
    up = job["case"][1] > job["case"][0]
    kinds = ["fft" if "form" in f else "poly" if f.get("kernel") == "poly" else "interp" for f in lines]
    assert kinds == (["fft", "poly"] if up else ["poly", "fft"]) * pairs + ["interp"], kinds
    for f in poly:
        assert int(f["T"]) == job["t2"], f
        assert int(f["MQ"]) == job["mq"] and int(f["width"]) == {"f32": 4, "f64": 8}[job["dtype"]] and f["il"] == "0" and f["split"] == "0", f
        assert 256 * int(f["R"]) == u or key[0] == "cut", "the table was made for the launcher's own R"
    return poly, admitted


@pytest.mark.parametrize("key", _UNCUT, ids=_ids(_UNCUT))
def test_a_constant_number_of_launches(key, run_env):
    """one kernel=poly line with ragged=<admitted columns>, one FFT line with the same, one interp* line with ragged=<short
    clips>; the poly grid is poly_grid_x of the longest clip over all columns"""
    job = JOBS[key]
    res = run_env(key[0])
    poly, admitted = _check_launches(key, res, 1)
    f, ch = poly[0], job["ch"]
    u, m, _, _, _, n_cu = (int(v) for v in res["geom_" + job["name"]])
    table = res["table_" + job["name"]]
    cols = len(admitted) * ch
    assert int(f["ragged"]) == cols == int(f["cols"])
    # the table holds the lengths it was to hold, in units of the launcher's own U
    outs = [int(v) for v in table[:, 3]]
    assert outs[1:7] == [m * u, m * u - 1, (m + 5) * u + 77, m * u + 1, (m + 2) * u + 3, 0] and outs[7] == 100
    assert max(outs) == outs[3] and min(int(table[0, 1]), outs[0]) == 8192 and min(int(table[8, 1]), outs[8]) == 8191
    assert all(min(int(r[1]), int(r[3])) == 8192 for r in table[9:]), "the extra clips are of the smallest admitted size"
    assert m * u > 8192 and all(_admitted(r) for r in table[1:6])
    if key[0] == "r1":
        assert u == 256 and m >= 33, "a tile of 256 outputs: the smallest admitted clip is 32 tiles and more"
    # the polyphase stage's outputs per column: the job's outputs (up) / the intermediate (down: 2 n_out + 2 pad)
    up = job["case"][1] > job["case"][0]
    poly_out = [int(r[3]) if up else _n_mid(job, r, int(f["T"])) for r in admitted]
    longest = max(poly_out)
    assert int(f["n_out"]) == longest
    tiles = -(-longest // u)
    gx, gy, gz = (int(v) for v in f["grid"].split("x"))
    assert int(f["tiles"]) == tiles and (gy, gz) == (cols, 1)
    assert gx in {_grid_x(tiles, per_cu, n_cu, cols) for per_cu in range(1, 9)}, (gx, tiles, n_cu, cols)
    if key[0] == "r1":
        assert min(poly_out) >= 32 * u, "the smallest admitted clip is 32 tiles or more"
    if job.get("extra"):  # enough columns that a column's workgroups are fewer than its tiles: the persistent walk, at every size
        assert gx < -(-min(poly_out) // u), "workgroups walk several tiles of the smallest admitted clip too: %d workgroups" % gx


@pytest.mark.parametrize("key", _ALL, ids=_ids(_ALL))
def test_admitted_columns_match_the_oracle_and_memory_is_kept(key, run_env, oracle):
    """windows of 3000 outputs at the head, the tail and one interior tile edge of every admitted column against the oracle's
    float64 direct form; the sentinels"""
    job = JOBS[key]
    res = run_env(key[0])
    got = _clips(key, res)
    u = int(res["geom_" + job["name"]][0])
    pl = oracle.plan(*job["case"])
    tol, worst = TOL_F64_HQ if (job["dtype"], job["case"][2]) == ("f64", "HQ") else TOL[job["dtype"]], 0.
    for c, (x, y) in enumerate(got):
        if not _admitted(res["table_" + job["name"]][c]):
            continue
        n_out = y.shape[0]
        edge = (n_out // (2 * u)) * u  # a tile edge of the job's outputs (up) / near one of the intermediate's (down), inside the clip
        for ch in range(job["ch"]):
            for k0 in (0, n_out - 3000, edge - 1500):
                ref = oracle.resample_channel(pl, x[:, ch].astype(np.float64), "ref", k0=k0, n_out=3000)
                err = _rms(y[k0:k0 + 3000, ch].astype(np.float64) - ref) / max(_rms(ref), 0.05)
                worst = max(worst, err)
                assert err <= tol, "%s clip %d channel %d window at %d: %.3g" % (key, c, ch, k0, err)
    diffs = res["autodiff_" + job["name"]]
    print("ragged two-stage %s-%s: worst relative RMS %.3g (bar %.0e); largest difference to the clip alone under AUTO %.3g"
          % (key[0], key[1], worst, tol, float(diffs.max())))


@pytest.mark.parametrize("key", _ALL, ids=_ids(_ALL))
def test_short_clips_equal_the_clip_run_alone(key, run_env):
    """bitwise: the exact engine's bits, as the clip has alone"""
    job = JOBS[key]
    res = run_env(key[0])
    got, flat, pos = _clips(key, res), res["short_" + job["name"]], 0
    for c, (_, y) in enumerate(got):
        row = res["table_" + job["name"]][c]
        if row[3] == 0 or _admitted(row):
            continue
        want = flat[pos:pos + y.size].reshape(y.shape)
        pos += y.size
        assert np.array_equal(_bits(y), _bits(want)), "%s clip %d of %d frames" % (key, c, len(y))
    assert pos == flat.size and pos > 0


@pytest.mark.parametrize("name", [k[1] for k in JOBS if k[0] == "cut"])
def test_range_cut_gives_the_same_bits_in_more_launch_pairs(name, run_env):
    """the intermediate budget lowered: one launch pair per range of columns, ranges as poly_rules.h cuts them, the uncut bits"""
    ref, res = run_env("default"), run_env("cut")
    job = JOBS[("cut", name)]
    table, es = res["table_" + name], {"f32": 4, "f64": 8}[job["dtype"]]
    assert np.array_equal(table, ref["table_" + name]) and np.array_equal(_bits(res["x_" + name]), _bits(ref["x_" + name]))
    # the ranges, restated: columns in table order, n_mid rounded up to 8 elements, at most CUT_BUDGET bytes (one column at least)
    t2 = int([f for f in _lines(ref["log_" + name]) if f.get("kernel") == "poly"][0]["T"])
    want, count, used = [], 0, 0
    for row in table:
        for _ in range(job["ch"] if _admitted(row) else 0):
            elems = -(-_n_mid(job, row, t2) // 8) * 8
            if count and (used + elems) * es > CUT_BUDGET:
                want.append(count)
                count, used = 0, 0
            count += 1
            used += elems
    want.append(count)
    assert len(want) >= 2, "the budget does not cut the table"
    poly, _ = _check_launches(("cut", name), res, len(want))
    assert [int(f["ragged"]) for f in poly] == want, (poly, want)
    assert np.array_equal(_bits(res["y_" + name]), _bits(ref["y_" + name])), "the cut launch's bits differ from the uncut one's"


def test_resample_ragged_under_defaults(run_env, oracle):
    """dist.resample_ragged(plan, clips) on float32 mono clips: three launches; admitted clips in the two-stage class of the
    oracle, short clips bit-equal to the clip alone on the exact engine; the double backward with KERNEL_ADJOINT runs"""
    res = run_env("default")
    job = PY_JOBS[0]
    lines = _lines(res["log_py_ragged"])
    assert [f.get("kernel", f.get("form")) for f in lines][0] == "poly" and len(lines) == 3, lines
    assert lines[0]["ragged"] == "2" and lines[1]["ragged"] == "2" and "form" in lines[1] and lines[2]["kernel"].startswith("interp") and lines[2]["ragged"] == "2"
    pl = oracle.plan(*job["case"])
    x, y, ex, xp, yp = res["x_py_ragged"], res["y_py_ragged"], res["exact_py_ragged"], 0, 0
    assert y.dtype == np.float32 and y.shape == ex.shape
    for n, n_out in zip(job["lengths"], (int(v) for v in res["nout_py_ragged"])):
        got, alone = y[yp:yp + n_out], ex[yp:yp + n_out]
        if min(n, n_out) >= 8192:
            for k0 in (0, n_out - 3000):
                ref = oracle.resample_channel(pl, x[xp:xp + n].astype(np.float64), "ref", k0=k0, n_out=3000)
                assert _rms(got[k0:k0 + 3000].astype(np.float64) - ref) <= 1e-6 * max(_rms(ref), 0.05), (n, k0)
            assert not np.array_equal(got, alone), "an admitted clip is the two-stage form's, not the exact engine's"
        else:
            assert np.array_equal(_bits(got), _bits(alone)), n
        xp, yp = xp + n, yp + n_out
    assert yp == len(y)
    assert res["ggw_py_ragged"].size > 0 and np.array_equal(_bits(res["ggw_py_ragged"]), _bits(res["ggw_want_py_ragged"]))


def test_resample_batch_float32_host_corpus(run_env, oracle, soxr):
    res = run_env("default")
    job = PY_JOBS[1]
    lines = _lines(res["log_py_batch"])
    assert len([f for f in lines if f.get("kernel") == "poly"]) == 1 and len([f for f in lines if "form" in f]) == 1, lines
    assert [f["ragged"] for f in lines if str(f.get("kernel", "")).startswith("interp")] == ["2"], lines
    pl = oracle.plan(*job["case"])
    x, y, xp, yp = res["x_py_batch"], res["y_py_batch"], 0, 0
    for n in job["lengths"]:
        alone = soxr.resample(x[xp:xp + n], job["case"][0], job["case"][1], quality=job["case"][2])   # (the host surface: the exact engine)
        n_out = len(alone)
        got = y[yp:yp + n_out]
        if min(n, n_out) >= 8192:
            for k0 in (0, n_out - 3000):
                ref = oracle.resample_channel(pl, x[xp:xp + n].astype(np.float64), "ref", k0=k0, n_out=3000)
                assert _rms(got[k0:k0 + 3000].astype(np.float64) - ref) <= 1e-6 * max(_rms(ref), 0.05), (n, k0)
        else:
            assert np.array_equal(_bits(got), _bits(alone)), n
        xp, yp = xp + n, yp + n_out
    assert yp == len(y)
