"""GPU: every launch form of the transposed operator (csrc/adjoint.hip, adj_launch) against a float64 reference.

adj_launch asks csrc/adjoint_rules.h (adj_tile_form, adj_gather_grid), which decides: lane-per-element kernel or period-tiled
kernel; 64, 32 or 16 lanes per slab; the 80 KB or the 160 KB LDS limit; channel groups (by shift or by division); z
workgroups per slab against n_waves waves per workgroup; and the gridDim.y wrap at 65535 columns.  The debug-switch build
writes one line per launch (HIPSOXR_DEBUG_LAUNCH_LOG, adj_launch_log), so a case here names the property its launch must
show and the test reads it from the log — the rule is not restated (tests/c/adjoint_rules_check.cpp holds the same table
against the rule on the CPU).  All jobs
run in ONE child process (tests/_adjoint_probe.py) into guarded, NaN-filled buffers; everything is compared here.

Per case: the launch form; 8 guard elements either side of every column untouched and every payload element written;
per-element error within the bounds of tests/test_gpu_adjoint.py — float64 1e-13 |A|^T|gy|, float32
(Tt + 2) 2^-24 |A32|^T|gy| on the bank rounded to float32.  Reference: the dense matrix from the oracle's forward on
unit impulses up to 4000 frames, tests/adjoint_ref.py (pinned to it by tests/test_adjoint_ref.py) above.  Every column of
a batch has random data of its own; column 0 of the batches of one (plan, length, type) is one shared vector that also
runs alone as a mono job — another launch form — and must come out with the same bits everywhere.

Non-finite cotangents (adjoint.hip's header, "REACH"): a non-finite gy[k] makes every gx[a] non-finite whose true
support holds k, and leaves every gx[a] outside the documented reach with the bits of the run without it."""
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
GUARD, POISON = 8, 12345.0
F32, F64 = "f32", "f64"
DTYPE = {F32: np.float32, F64: np.float64}

DOWN_QQ, DOWN_LQ = (44100, 8000, "QQ"), (48000, 11025, "LQ")      # Mc 441, 28 phase tiles; Mc 640, 40 phase tiles
UP_640, UP_441 = (11025, 48000, "LQ"), (8000, 44100, "LQ")         # Lc 640; Lc 441: long slab rows
PRIME, TRIPLE = (9973, 12289, "QQ"), (16000, 48000, "QQ")          # Lc 12289: no tile tables; Mc 22
NF_CASE = (48000, 44100, "HQ")

# name -> (plan, n_x, clips, channels, type, {log field: value}).  The log must show the stated form; a case is resized,
# never its assertion changed, if a later launch rule moves it.
FORMS = {
    # (a) 40 columns of one workgroup each: 14 workgroups of 2 waves per slab
    "a_f32": (DOWN_QQ, 3533, 40, 1, F32, dict(kernel="adj_tile", block=128, gz=14)),
    "a_f64": (DOWN_QQ, 3533, 40, 1, F64, dict(kernel="adj_tile", block=128, gz=14)),
    # (b) a training batch: one workgroup of 16 waves per slab, 28 tiles -> 2 tiles on waves 0-11, 1 on 12-15
    "b_f32": (DOWN_QQ, 3533, 600, 1, F32, dict(kernel="adj_tile", block=1024, gz=1, n_st=28)),
    "b_f64": (DOWN_QQ, 3533, 600, 1, F64, dict(kernel="adj_tile", block=1024, gz=1, n_st=28)),
    # (c) 40 tiles -> 3 on waves 0-7, 2 on the rest
    "c_f32": (DOWN_LQ, 3205, 600, 1, F32, dict(kernel="adj_tile", block=1024, gz=1, n_st=40)),
    # (d) channel groups: 2 and 4 (lane -> (period, channel) by shift), 5 (by division)
    "d2_f64": (DOWN_QQ, 3533, 300, 2, F64, dict(kernel="adj_tile", cg=2, pb=32, block=640)),
    "d4_f32": (DOWN_QQ, 3533, 300, 4, F32, dict(kernel="adj_tile", cg=4, pb=16, block=640)),
    "d5_f64": (DOWN_QQ, 3533, 200, 5, F64, dict(kernel="adj_tile", cg=5, pb=12, block=384)),
    # (e) 70 channels: float32 2 groups of 64 (the last with 6 live channels), float64 3 groups of 32 on 32 lanes
    "e_f32": (DOWN_QQ, 3533, 40, 70, F32, dict(kernel="adj_tile", lanes=64, cg=64, gy=80, gz=1)),
    "e_f64": (DOWN_QQ, 3533, 40, 70, F64, dict(kernel="adj_tile", lanes=32, cg=32, gy=120)),
    # (f, g) slabs above 80 KB: the 160 KB limit
    "f_f64": (UP_640, 597, 1, 1, F64, dict(kernel="adj_tile", lanes=16, lds=87176)),
    "g_f64": (UP_441, 329, 1, 8, F64, dict(kernel="adj_tile", lanes=32, lds=141120)),
    # (h) a tile-capable plan and a long enough job, but no lane count fits LDS
    "h_f64": (UP_640, 597, 1, 64, F64, dict(kernel="adj_gather")),
    # (i) no tile tables; frames of periods q = 0, 1 and 2
    "i_f32": (PRIME, 2 * 9973 + 5, 1, 1, F32, dict(kernel="adj_gather")),
    "i_f64": (PRIME, 2 * 9973 + 5, 1, 1, F64, dict(kernel="adj_gather")),
    "i3_f32": (PRIME, 2 * 9973 + 5, 1, 3, F32, dict(kernel="adj_gather")),
    "i3_f64": (PRIME, 2 * 9973 + 5, 1, 3, F64, dict(kernel="adj_gather")),
    # (j, k) more columns than gridDim.y holds: the last 65 come from the column loop
    "j_f32": (TRIPLE, 91, 65600, 1, F32, dict(kernel="adj_tile", gy=65535)),
    "k_f32": (TRIPLE, 5, 65600, 1, F32, dict(kernel="adj_gather", gy=65535)),
    # (l) the threshold 4 Mc = 88 frames; 64 periods of 22 frames = 1408: one workgroup exactly full, then one frame more
    "l87_f64": (TRIPLE, 87, 1, 1, F64, dict(kernel="adj_gather")),
    "l88_f64": (TRIPLE, 88, 1, 1, F64, dict(kernel="adj_tile", gx=1)),
    "l1408_f64": (TRIPLE, 1408, 1, 1, F64, dict(kernel="adj_tile", pb=64, gx=1)),
    "l1409_f64": (TRIPLE, 1409, 1, 1, F64, dict(kernel="adj_tile", pb=64, gx=2)),
}
SHARED_COL0 = [n for n in FORMS if n[0] in "abcde"]  # column 0 also runs alone: mono_<plan>_<n_x>_<type>
NF_JOBS = {"tile": 4000, "gather": 600}              # 48k -> 44.1k HQ: 4000 frames tiled, 600 (< 4 Mc = 640) lane per element


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


@functools.lru_cache(maxsize=None)
def _dense(case, n_x, f32):
    from oracle import oracle
    A = adjoint_ref.dense(oracle, oracle.plan(*case), _bank(case, f32), n_x)
    assert A.shape == (_plan(case).out_len(n_x), n_x)
    A.setflags(write=False)
    return A


def _mono_name(case, n_x, kind):
    return "mono_%d_%d_%s_%d_%s" % (case[0], case[1], case[2], n_x, kind)


def _parse(log):
    """one launch line -> {field: value}; grid=XxYxZ becomes gx, gy, gz"""
    assert log and log.count("\n") == 0, "one launch per job: %r" % log
    f = dict(tok.split("=", 1) for tok in log.split())
    out = {k: (v if k == "kernel" else int(v)) for k, v in f.items() if k != "grid"}
    out["gx"], out["gy"], out["gz"] = (int(v) for v in f["grid"].split("x"))
    return out


def _make_jobs():
    rng = np.random.default_rng(4141)
    out, col0 = {}, {}
    for name, (case, n_x, clips, ch, kind, _) in FORMS.items():
        n_y = _plan(case).out_len(n_x)
        gy = rng.standard_normal((clips, n_y, ch)).astype(DTYPE[kind])
        if name in SHARED_COL0:
            mono = _mono_name(case, n_x, kind)
            if mono not in col0:
                col0[mono] = rng.standard_normal(n_y).astype(DTYPE[kind])
                out[mono] = (case, n_x, col0[mono].reshape(1, n_y, 1))
            gy[0, :, 0] = col0[mono]
        out[name] = (case, n_x, gy)
    for kern, n_x in NF_JOBS.items():
        n_y = _plan(NF_CASE).out_len(n_x)
        for kind in (F32, F64):
            base = rng.standard_normal((1, n_y, 1)).astype(DTYPE[kind])
            for tag, v in (("base", None), ("inf", np.inf), ("nan", np.nan)):
                gy = base.copy()
                if v is not None:
                    gy[0, n_y // 2, 0] = v
                out["nf_%s_%s_%s" % (kern, kind, tag)] = (NF_CASE, n_x, gy)
    return out


@pytest.fixture(scope="module")
def jobs():
    """name -> (plan, n_x, gy [clips, n_y, channels])"""
    return _make_jobs()


@pytest.fixture(scope="module")
def results(jobs, tmp_path_factory):
    """The probe's results: one child process for the whole file."""
    assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
    tmp = tmp_path_factory.mktemp("adjoint_forms")
    meta = [{"name": n, "case": list(case), "n_x": n_x} for n, (case, n_x, _) in jobs.items()]
    np.savez(tmp / "jobs.npz", meta=np.array(json.dumps(meta)), **{"gy_" + n: gy for n, (_, _, gy) in jobs.items()})
    env = {key: v for key, v in os.environ.items() if not key.startswith("HIPSOXR_")}
    env.update({"HIPSOXR_LIBRARY": DBG_LIB, "HIPSOXR_DEBUG_LAUNCH_LOG": str(tmp / "launch.log")})
    r = subprocess.run([sys.executable, os.path.join(HERE, "_adjoint_probe.py"), str(tmp / "jobs.npz"), str(tmp / "results.npz")],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(tmp / "results.npz")


def _payload(name, jobs, results):
    """guards checked; -> (the job's gy, gx payload) as [frames, columns] matrices, column = clip * channels + channel"""
    case, n_x, gy = jobs[name]
    buf = results["gx_" + name]
    assert buf.shape == (gy.shape[0], n_x + 2 * GUARD, gy.shape[2]) and buf.dtype == gy.dtype
    assert np.all(buf[:, :GUARD] == POISON) and np.all(buf[:, -GUARD:] == POISON), "guard elements were written"
    cols = lambda t: t.transpose(1, 0, 2).reshape(t.shape[1], -1)
    return cols(gy), cols(buf[:, GUARD:-GUARD])


def _reference(case, n_x, kind, gy):
    """-> (A^T gy, |A|^T |gy|) in float64 for the matrix of the type's bank"""
    g = gy.astype(np.float64)
    if n_x <= 4000:
        A = _dense(case, n_x, kind == F32)
        return A.T @ g, np.abs(A).T @ np.abs(g)
    plan = _plan(case)
    return adjoint_ref.scatter(plan.L, plan.M, _bank(case, kind == F32), g, n_x)


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("name", list(FORMS))
def test_form_guards_and_parity(jobs, results, name):
    case, n_x, clips, ch, kind, expect = FORMS[name]
    plan = _plan(case)
    log = _parse(str(results["log_" + name]))
    print(name, "launch:", str(results["log_" + name]))
    assert log["width"] == (4 if kind == F32 else 8) and (log["L"], log["M"]) == (plan.L, plan.M)
    assert {k: log[k] for k in expect} == expect, log
    if log["kernel"] == "adj_tile":
        assert 0 < log["cg"] * log["pb"] <= log["lanes"]
        assert log["gy"] == min(clips * -(-ch // log["cg"]), 65535)
    if name[0] in "bc":  # z == 1: wave w of 16 takes tiles w, w + 16, ...
        per_wave = [len(range(w, log["n_st"], log["block"] // 64)) for w in range(16)]
        assert per_wave == ([2] * 12 + [1] * 4 if name[0] == "b" else [3] * 8 + [2] * 8)
    if name[0] == "i":
        assert n_x // plan.M == 2 and n_x % plan.M > 0  # periods q = 0, 1 and (partly) 2
    gy, gx = _payload(name, jobs, results)
    assert np.isfinite(gx).all(), "a payload element was not written"
    want, mag = _reference(case, n_x, kind, gy)
    if kind == F64:
        bound = 1e-13 * mag + 1e-300
    else:  # any float32 summation order of at most Tt terms, plus the output rounding
        bound = (math.ceil(plan.taps * plan.L / plan.M) + 1 + 2) * 2.0 ** -24 * mag
    err = np.abs(gx.astype(np.float64) - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("adjoint forms %s: %d columns, worst error/bound %.4f" % (name, gx.shape[1], ratio))
    assert (err <= bound).all(), ratio
    if name in SHARED_COL0:  # the same column alone, as a mono job: another launch form, the same bits
        mono = _mono_name(case, n_x, kind)
        mlog = _parse(str(results["log_" + mono]))
        assert mlog["kernel"] == "adj_tile" and (mlog["block"], mlog["gz"], mlog["cg"]) != (log["block"], log["gz"], log["cg"]), mlog
        mgy, mgx = _payload(mono, jobs, results)
        assert np.array_equal(mgy[:, 0], gy[:, 0])
        assert np.array_equal(_bits(mgx[:, 0]), _bits(gx[:, 0])), "column 0 differs from the same column run alone"


@pytest.mark.parametrize("kind", [F32, F64])
@pytest.mark.parametrize("kern", list(NF_JOBS))
def test_non_finite_cotangent_reach(jobs, results, kern, kind):
    """adjoint.hip REACH: gy[k] is read by gx[a] only where
         k_adj_gather   -(T/2 + 2 M/L)      < a - k M/L <= T/2
         k_adj_tile     -(T/2 + 15 + 4 M/L) < a - k M/L <= T/2 + 15
    (compared exactly, multiplied through by L)."""
    from oracle import oracle
    plan, n_x = _plan(NF_CASE), NF_JOBS[kern]
    L, M, H = plan.L, plan.M, plan.taps // 2
    names = {t: "nf_%s_%s_%s" % (kern, kind, t) for t in ("base", "inf", "nan")}
    for nm in names.values():
        log = _parse(str(results["log_" + nm]))
        assert log["kernel"] == "adj_" + kern, log
    gy, base = _payload(names["base"], jobs, results)
    k = gy.shape[0] // 2
    assert np.isfinite(base).all()
    a = np.arange(n_x, dtype=np.int64)
    off = a * L - k * M  # (a - k M/L) L
    below, above = ((H + 15) * L + 4 * M, (H + 15) * L) if kern == "tile" else (H * L + 2 * M, H * L)
    inside = (off > -below) & (off <= above)
    assert below <= (H + 16) * L + 8 * M and inside.any() and not inside[0] and not inside[-1]  # (a mid-signal sample)
    # true support: row k of the dense matrix, from the oracle's forward on the unit impulses of the reach
    pl, bank = oracle.plan(*NF_CASE), _bank(NF_CASE, kind == F32)
    support = np.zeros(n_x, bool)
    for ai in np.flatnonzero(inside):
        e = np.zeros(n_x)
        e[ai] = 1.0
        support[ai] = oracle.resample_channel(pl, e, "ref", bank=bank)[k] != 0.0
    assert support.sum() > plan.taps // 2
    for tag in ("inf", "nan"):
        g2, gx = _payload(names[tag], jobs, results)
        assert not np.isfinite(g2[k, 0]) and np.array_equal(np.delete(g2[:, 0], k), np.delete(gy[:, 0], k))
        hit = ~np.isfinite(gx[:, 0])
        print("non-finite %s %s %s: true support %d frames, non-finite %d, documented reach %d" % (kern, kind, tag, support.sum(), hit.sum(), inside.sum()))
        assert hit[support].all(), "a gx element whose support holds the non-finite sample is finite"
        assert np.array_equal(_bits(gx[~inside, 0]), _bits(base[~inside, 0])), "the non-finite sample spread past the documented reach"
