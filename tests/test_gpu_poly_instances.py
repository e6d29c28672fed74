"""GPU: every kernel instance of the two-stage form's polyphase stage that a plan can launch (csrc/twostage.hip, poly_kernel)
against the oracle's float64 direct form, knowingly, and its long runs.

poly_kernel expands HIPSOXR_POLY_TAPS / HIPSOXR_POLY2_TAPS to 152 kernels: k_poly<Real, TT, MQ, RAGGED> (10 tap counts x MQ
{0, 1, -1} x float32 / float64 x 2) and k_poly2<TT, MQ, IL> (8 x 2 x 2), each with its own unrolled tap loop and register-window
shift.  The census below parses the two macros, enumerates the instances and wants every one either launched by a job here —
the instance read from the debug-switch build's launch log (HIPSOXR_DEBUG_LAUNCH_LOG: kernel, width, T, MQ, il, split,
ragged=), never re-derived from the rules — or listed in UNREACHABLE with its reason in words.  60 are reachable:
(T2, MQ) in REACHABLE for float32, the same up to 32 taps for float64 (a longer float64 table does not fit LDS), each also in
ragged form (the jobs of tests/test_gpu_ragged_two_stage.py, whose default child this file shares), and the ten of up to 40
taps on k_poly2 with IL true (interleaved stereo) and false (a split mono column).

One child process per environment (tests/_poly_instances_probe.py) — the default, and HIPSOXR_POLY_NO_PAIR=1, which sends
float32 jobs of up to 40 taps to k_poly — each with a time limit of its own; after a failed child nothing further is started.

Leg A, the smallest size: one clip of 8192 (+ 3) frames on its shorter side — a split column: the first length poly_form
splits — mono for k_poly, interleaved stereo for k_poly2 IL.  Every column, whole signal, against
oracle.resample_channel(plan, x, "ref"); 8 guard elements either side of every column intact, no NaN left, twice the same bytes.
Leg B, long runs: the same plans with 1024 columns of the leg-A length (and one job of 8 interleaved channels per family).
A column then has one workgroup and fewer workgroups than tiles: runs of up to 12 outputs per thread with their repeated window
shift, the persistent walk with the next tile's span prefetched, and k_poly's staging loop behind the 8 x 256 prefetched
samples (a span above 2048 samples) — all asserted from the launch line.  Per column on the device against the same job under
KERNEL_EXACT; the first, middle and last column against the oracle as in leg A.

Bars, per column, white noise of RMS 0.25 seeded per column: relative RMS <= 1e-6 (float32), 2e-9 (float64 VHQ) — the bars of
tests/test_gpu_two_stage.py — and 1e-6 (float64 HQ: what the HQ float32 form meets on the same filter; WHOLE_BAR of
tests/_table_probe.py for the FFT stage); pointwise, the largest error <= 10 x that bar x the column's RMS (the proportion
test_two_stage_split_columns holds float32 to; Gaussian error over 4e4 samples peaks near 4.4 sigma).
A job is resized, never its assertion changed, if a later launch rule moves it off its form or run length."""
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import test_gpu_ragged_two_stage as ragged  # leg C: the ragged instances' jobs and their child process

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DBG_LIB = os.path.join(ROOT, "python-soxr_amd", "_variants", "dbg", "libhipsoxr.so")
SOURCE = os.path.join(ROOT, "python-soxr_amd", "csrc", "twostage.hip")
GUARD, POISON = 8, 12345.0
F32, F64 = "f32", "f64"
NP = {F32: np.float32, F64: np.float64}
WIDTH = {F32: 4, F64: 8}

# (T2, MQ) -> the plan that reaches it (n_taps of poly_design in brackets: 0.3 tap or more inside its interval)
REACHABLE = {
    (12, 0): (48000, 45887, "HQ"),    # (10.2)
    (16, 0): (48000, 44101, "VHQ"),   # (14.2)
    (20, 0): (48000, 32001, "VHQ"),   # (19.3)
    (24, 0): (48000, 27941, "VHQ"),   # (21.9)
    (28, 0): (48000, 96734, "VHQ"),   # (25.3, up)
    (20, 1): (44101, 48000, "HQ"),    # (18.6, up)
    (24, 1): (48000, 20962, "HQ"),    # (21.2)
    (28, 1): (44101, 48000, "VHQ"),   # (25.3, up)
    (32, 1): (44100, 12986, "HQ"),    # (30.9)
    (40, 1): (48000, 12986, "HQ"),    # (33.6)
    (48, 1): (48000, 13983, "VHQ"),   # (42.8)
}
# (T2, MQ) -> (plan, frames): a short phase period Ls (rate pairs with a common factor), the first length whose column splits
SPLIT = {
    (12, 0): ((44100, 36322, "HQ"), 18723),   # Ls 18161 (11.7)
    (16, 0): ((48000, 39723, "VHQ"), 13571),  # Ls 13241 (15.7)
    (20, 0): ((48000, 31227, "VHQ"), 13563),  # Ls 10409 (19.7)
    (24, 0): ((48000, 29001, "VHQ"), 13560),  # Ls 9667 (21.1)
    (28, 0): ((48000, 25059, "VHQ"), 15691),  # Ls 8353 (24.3): the first admitted length (8192 outputs) splits
    (20, 1): ((44100, 83896, "HQ"), 9372),    # Ls 10487 (18.6, up)
    (24, 1): ((44100, 19322, "HQ"), 18706),   # Ls 9661 (21.1)
    (28, 1): ((44100, 61688, "VHQ"), 9372),   # Ls 7711 (25.3, up)
    (32, 1): ((96000, 42755, "VHQ"), 18393),  # Ls 8551 (28.3)
    (40, 1): ((44100, 17138, "VHQ"), 21079),  # Ls 8569 (32.3)
}
F64_MAX_TAPS, POLY2_MAX_TAPS = 32, 40
LEG_B_COLUMNS, LEG_B_MAX_OUTPUTS, LEG_B_MIN_CLIPS = 1024, 64 << 20, 256

# ---- the census: every instance poly_kernel can name is a case or has a reason ------------------------------------------
# an instance: ("poly", type, T, MQ, ragged) | ("poly2", T, MQ, IL)
R_T8 = "T2 = 8: poly_design never asks for fewer than 9.6 taps"
R_T56 = "T2 = 56: its table exceeds poly_design's 100 KiB test"
R_MQ = "MQ -1: Ms / Ls < 2 for every ratio the form admits"
R_PAIR = "no ratio produces this (T2, MQ)"
R_F64 = "float64 at 40 taps and more: the table does not fit LDS, the exact engine keeps the job"
UNREACHABLE = {}
for _t in (8, 12, 16, 20, 24, 28, 32, 40, 48, 56):
    for _mq in (0, 1, -1):
        _why = R_T8 if _t == 8 else R_T56 if _t == 56 else R_MQ if _mq < 0 else None if (_t, _mq) in REACHABLE else R_PAIR
        for _kind in (F32, F64):
            _w = _why or (R_F64 if _kind == F64 and _t > F64_MAX_TAPS else None)
            if _w:
                UNREACHABLE[("poly", _kind, _t, _mq, False)] = UNREACHABLE[("poly", _kind, _t, _mq, True)] = _w
        if _t <= POLY2_MAX_TAPS and _mq >= 0 and _why:
            UNREACHABLE[("poly2", _t, _mq, True)] = UNREACHABLE[("poly2", _t, _mq, False)] = _why


def parse_taps():
    """-> (k_poly's tap counts, k_poly2's) as twostage.hip's two macros list them"""
    with open(SOURCE) as f:
        src = f.read()
    out = []
    for macro in ("HIPSOXR_POLY_TAPS", "HIPSOXR_POLY2_TAPS"):
        m = re.search(r"#define\s+%s\(X\)((?:\s*X\(\d+\))+)" % macro, src)
        assert m, macro
        out.append([int(v) for v in re.findall(r"X\((\d+)\)", m.group(1))])
    return out


def all_instances():
    taps, taps2 = parse_taps()
    inst = [("poly", kind, t, mq, rg) for kind in (F32, F64) for t in taps for mq in (0, 1, -1) for rg in (False, True)]
    return inst + [("poly2", t, mq, il) for t in taps2 for mq in (0, 1) for il in (True, False)]


def instance_of(f):
    """a parsed polyphase launch line -> the instance it names"""
    if f["kernel"] == "poly2":
        assert f["width"] == 4 and f["il"] != f["split"] and "ragged" not in f, f
        return ("poly2", f["T"], f["MQ"], bool(f["il"]))
    assert f["kernel"] == "poly" and not f["il"] and not f["split"], f
    return ("poly", {4: F32, 8: F64}[f["width"]], f["T"], f["MQ"], "ragged" in f)


# ---- the jobs ----------------------------------------------------------------------------------------------------------
ENVS = {"default": {}, "no_pair": {"HIPSOXR_POLY_NO_PAIR": "1"}}
# seconds, from the first measured run (profiles/NOTES_poly_instances.md): the children took 3.3 s and 2.9 s, of which 1.5 s
# and 1.0 s were the jobs and the rest the start of the process — the part that varies from machine to machine: 60 s for it
# (the suite's other probes allow their start as much) and twenty times the jobs' own time
TIMEOUT = {"default": 90, "no_pair": 80}
JOBS = {}  # name -> job for the probe + "env", "expect": the fields its launch line must show


def _add(name, env, leg, case, kind, frames, clips, ch, expect):
    JOBS[name] = dict(name=name, env=env, leg=leg, case=list(case), dtype=kind, frames=frames, clips=clips, ch=ch, seed=4000 + len(JOBS),
                      expect=dict(expect, width=WIDTH[kind]))


def _shorter_side_8192(case):
    """the least frame count with 8192 frames or more either side (out_len = floor(n L / M + 1/2)), plus a few"""
    fi, fo = case[0], case[1]
    n = 8192 if fo >= fi else -(-(2 * 8192 - 1) * fi // (2 * fo))
    return n + 3


for (_t, _mq), _case in REACHABLE.items():
    _n, _tag = _shorter_side_8192(_case), "%d_%d" % (_t, _mq)
    _forms = [("poly_f32", "no_pair", F32, 1, dict(kernel="poly", T=_t, MQ=_mq, il=0, split=0))]
    if _t <= F64_MAX_TAPS:
        _forms.append(("poly_f64", "default", F64, 1, dict(kernel="poly", T=_t, MQ=_mq, il=0, split=0)))
    if _t <= POLY2_MAX_TAPS:
        _forms.append(("pair", "default", F32, 2, dict(kernel="poly2", T=_t, MQ=_mq, il=1, split=0)))
    for _form, _env, _kind, _ch, _expect in _forms:
        _add("A_%s_%s" % (_form, _tag), _env, "A", _case, _kind, _n, 1, _ch, _expect)
        _add("B_%s_%s" % (_form, _tag), _env, "B", _case, _kind, _n, LEG_B_COLUMNS, _ch, _expect)
for (_t, _mq), (_case, _n) in SPLIT.items():
    _expect, _tag = dict(kernel="poly2", T=_t, MQ=_mq, il=0, split=1), "%d_%d" % (_t, _mq)
    _outs = (2 * _n * _case[1] + _case[0]) // (2 * _case[0])
    _add("A_split_" + _tag, "default", "A", _case, F32, _n, 1, 1, _expect)
    _add("B_split_" + _tag, "default", "B", _case, F32, _n, max(LEG_B_MIN_CLIPS, min(LEG_B_COLUMNS, LEG_B_MAX_OUTPUTS // _outs)), 1, _expect)
# 8 interleaved channels: four channel pairs (k_poly2) / four channels (k_poly under NO_PAIR) per workgroup, 1024 grid rows each
_add("B_pair_8ch", "default", "B", REACHABLE[(16, 0)], F32, _shorter_side_8192(REACHABLE[(16, 0)]), 1024, 8, dict(kernel="poly2", T=16, MQ=0, il=1, split=0, lg_cg=2))
_add("B_poly_8ch", "no_pair", "B", REACHABLE[(16, 0)], F32, _shorter_side_8192(REACHABLE[(16, 0)]), 512, 8, dict(kernel="poly", T=16, MQ=0, il=0, split=0, lg_cg=2))
LEG_A = [n for n, j in JOBS.items() if j["leg"] == "A"]
LEG_B = [n for n, j in JOBS.items() if j["leg"] == "B"]
assert len(LEG_A) == 40 and len(LEG_B) == 42

_child_failed = ragged._child_failed  # one list for both files: a fault, abort or time limit in a child of either
_results, _wall = {}, {}


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
        tmp = tmp_path_factory.mktemp("poly_instances_" + env_name)
        assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
        with open(tmp / "jobs.json", "w") as f:
            json.dump([{k: v for k, v in j.items() if k not in ("env", "expect")} for j in JOBS.values() if j["env"] == env_name], f)
        env = {key: v for key, v in os.environ.items() if not key.startswith("HIPSOXR_")}
        env.update({"HIPSOXR_LIBRARY": DBG_LIB, "HIPSOXR_DEBUG_LAUNCH_LOG": str(tmp / "launch.log")})
        env.update(ENVS[env_name])
        t0 = time.time()
        try:
            r = subprocess.run([sys.executable, os.path.join(HERE, "_poly_instances_probe.py"), str(tmp / "jobs.json"), str(tmp / "out.npz")],
                               env=env, capture_output=True, text=True, timeout=TIMEOUT[env_name])
        except subprocess.TimeoutExpired as e:
            _child_failed.append("%s: time limit, last case started: %s" % (env_name, (e.stdout or b"").decode(errors="replace").strip().splitlines()[-1:]))
            raise
        _wall[env_name] = time.time() - t0
        if r.returncode != 0:
            _child_failed.append("%s: exit status %d" % (env_name, r.returncode))
        started = [ln for ln in r.stdout.splitlines() if ln.startswith("POLY_CASE ")]
        assert r.returncode == 0, ("last case started: " + (started[-1] if started else "none"), r.stderr[-3000:])
        _results[env_name] = np.load(tmp / "out.npz")
        print("poly instances child %s: %d jobs, %.1f s (in the child: %.1f s)" % (env_name, len(started), _wall[env_name], float(_results[env_name]["wall"])))
        return _results[env_name]
    return get


def _parse(line):
    """one polyphase launch line -> {field: value}; grid=XxYxZ becomes gx, gy, gz"""
    f = dict(tok.split("=", 1) for tok in line.split())
    out = {k: (v if k == "kernel" else float(v) if k == "conf" else int(v)) for k, v in f.items() if k != "grid"}
    out["gx"], out["gy"], out["gz"] = (int(v) for v in f["grid"].split("x"))
    return out


def _poly_lines(log):
    return [_parse(ln) for ln in str(log).splitlines() if ln.startswith("kernel=poly")]


def _launch(name, res):
    """the job's one polyphase launch, with the form and instance the job was made for"""
    job = JOBS[name]
    poly = _poly_lines(res["log_" + name])
    assert len(poly) == 1, "one polyphase launch per job: %r" % str(res["log_" + name])
    f = poly[0]
    print(name, "launch:", str(res["log_" + name]).replace("\n", " | "))
    assert {k: f[k] for k in job["expect"]} == job["expect"], f
    assert "ragged" not in f and f["block"] == 256
    assert 1 <= f["R"] <= 12 and f["lane_mul"] % 2 == 1 and f["tiles"] == -(-f["n_out"] // (256 * f["R"]))
    assert 1 <= f["gx"] <= f["tiles"] and f["gy"] == f["cols"] == job["clips"] * job["ch"] // ((2 if f["il"] else 1) << f["lg_cg"]) and f["gz"] == 1
    assert f["lds"] <= 160 * 1024
    if f["split"]:  # member 1 is the longer one; member 2 ends inside a tile
        assert 0 < f["m2_n_out"] <= f["n_out"] and f["m2_n_out"] % (256 * f["R"]) != 0
    else:
        assert f["m2_n_out"] == f["n_out"]
    return f


def _rms(v):
    return float(np.sqrt(np.mean(np.square(v, dtype=np.float64))))


def _bar(job):
    return 1e-6 if job["dtype"] == F32 or job["case"][2] == "HQ" else 2e-9


_shares = {}  # (name, what) -> the largest share of its bar


def _against_the_oracle(oracle, name, x, y, what):
    """one column, whole signal: relative RMS and the largest error at the job's bars"""
    job = JOBS[name]
    pl = oracle.plan(*job["case"])
    ref = oracle.resample_channel(pl, x.astype(np.float64), "ref")
    assert y.shape == ref.shape, "exact output shape"
    d = y.astype(np.float64) - ref
    bar, rms = _bar(job), _rms(ref)
    rel, peak = _rms(d) / rms, float(np.abs(d).max())
    print("poly instances %s %s: relative RMS %.3g (bar %.0e), largest error %.3g (bar %.3g)" % (name, what, rel, bar, peak, 10 * bar * rms))
    _shares[(name, "oracle rms")] = max(_shares.get((name, "oracle rms"), 0.), rel / bar)
    _shares[(name, "oracle max")] = max(_shares.get((name, "oracle max"), 0.), peak / (10 * bar * rms))
    assert rms > 0.05, "white noise of RMS 0.25 through a filter that keeps a quarter of its band or more"
    assert rel <= bar, (name, what, rel)
    assert peak <= 10 * bar * rms, (name, what, peak)


@pytest.mark.parametrize("name", LEG_A)
def test_smallest_size_every_column_against_the_oracle(name, run_env, oracle):
    job = JOBS[name]
    res = run_env(job["env"])
    f = _launch(name, res)
    x, buf = res["x_" + name], res["y_" + name]
    n_out = buf.shape[1] - 2 * GUARD
    assert x.shape == (1, job["frames"], job["ch"]) and buf.shape[::2] == (1, job["ch"]) and buf.dtype == NP[job["dtype"]]
    assert 8192 <= min(job["frames"], n_out) and (f["split"] or min(job["frames"], n_out) <= 8192 + 8), "the smallest size the form admits"
    assert np.all(buf[:, :GUARD] == POISON) and np.all(buf[:, -GUARD:] == POISON), "guard elements were written"
    y = buf[:, GUARD:-GUARD]
    assert not np.isnan(y).any(), "a payload element was not written"
    assert np.isfinite(y).all()
    assert bool(res["same_" + name]), "the same job again gave other bytes"
    for c in range(job["ch"]):
        _against_the_oracle(oracle, name, x[0, :, c], y[0, :, c], "column %d" % c)


@pytest.mark.parametrize("name", LEG_B)
def test_long_runs_every_column_against_the_exact_engine(name, run_env, oracle):
    job = JOBS[name]
    res = run_env(job["env"])
    f = _launch(name, res)
    small = _poly_lines(res["log_" + name.replace("B_", "A_", 1)]) if name.replace("B_", "A_", 1) in JOBS else None
    # the run lengths this leg is for, from the launch line
    assert f["gx"] < f["tiles"], "a workgroup walks more than one tile"
    if small:
        assert f["R"] >= small[0]["R"], "runs at least as long as the smallest size's"
    if job["dtype"] == F32:
        assert f["R"] >= 3, "the repeated window shift: runs of three outputs and more"
    guards_ok, still_nan, not_finite = (int(v) for v in res["ok_" + name])
    assert guards_ok == 1, "guard elements were written"
    assert still_nan == 0, "a payload element was not written"
    assert not_finite == 0
    rel, peak, rms = res["rel_" + name], res["max_" + name], res["rms_" + name]
    assert rel.shape == peak.shape == rms.shape == (job["clips"], job["ch"])
    bar = _bar(job)
    share_rms, share_max = float((rel / bar).max()), float((peak / (10 * bar * rms)).max())
    print("poly instances %s: R %d, grid x %d, tiles %d; over %d columns against the exact engine: largest relative RMS %.3g (bar %.0e), "
          "largest error over its bar %.3f" % (name, f["R"], f["gx"], f["tiles"], rel.size, float(rel.max()), bar, share_max))
    _shares[(name, "exact rms")], _shares[(name, "exact max")] = share_rms, share_max
    assert np.all(rms > 0.05), "white noise of RMS 0.25 through a filter that keeps a quarter of its band or more, every column"
    assert np.all(rel > 0), "the exact engine's bits: the polyphase launch did not write the result"
    assert np.all(rel <= bar), (name, float(rel.max()), np.argwhere(rel > bar)[:4].tolist())
    assert np.all(peak <= 10 * bar * rms), (name, share_max, np.argwhere(peak > 10 * bar * rms)[:4].tolist())
    cols = [tuple(int(v) for v in c) for c in res["cols_" + name]]
    assert cols == [(0, 0), (job["clips"] // 2, job["ch"] // 2), (job["clips"] - 1, job["ch"] - 1)]
    for i, c in enumerate(cols):
        _against_the_oracle(oracle, name, res["x_" + name][i], res["y_" + name][i], "clip %d channel %d" % c)


def test_long_runs_reach_the_run_lengths_they_are_for(run_env):
    """over leg B: R = 12 on a k_poly float32 job, R >= 8 on a k_poly2 job, and for a k_poly float32 job of each MQ a tile whose
    source span (256 R Ms / Ls + T + 4 samples) exceeds the 2048 prefetched ones: the staging loop behind them runs"""
    rows = []
    for name in LEG_B:
        job = JOBS[name]
        f = _poly_lines(run_env(job["env"])["log_" + name])[0]
        L, M = _lowest_terms(job["case"])
        ratio = 2 * M / L if job["case"][1] > job["case"][0] else M / (2 * L)  # Ms / Ls of the polyphase stage
        rows.append((name, f["kernel"], f["width"], f["MQ"], f["R"], f["gx"], f["tiles"], 256 * f["R"] * ratio + f["T"] + 4))
        print("leg B %-20s %-5s width %d MQ %2d R %2d grid x %d tiles %3d span %.0f" % rows[-1])
    poly32 = [r for r in rows if r[1] == "poly" and r[2] == 4]
    assert any(r[4] == 12 for r in poly32), "no k_poly float32 job with runs of 12"
    assert any(r[4] >= 8 for r in rows if r[1] == "poly2"), "no k_poly2 job with runs of 8 and more"
    for mq in (0, 1):
        assert any(r[7] > 2048 for r in poly32 if r[3] == mq), "no k_poly float32 job of MQ %d stages a span beyond its prefetched samples" % mq


def _lowest_terms(case):
    """out / in = L / M in lowest terms (integer rates)"""
    g = int(np.gcd(int(case[0]), int(case[1])))
    return int(case[1]) // g, int(case[0]) // g


def test_census_every_instance_is_a_case_or_has_a_reason(run_env, tmp_path_factory):
    instances = all_instances()
    assert len(instances) == len(set(instances)) == 152, len(instances)
    wanted = {}  # instance -> the jobs made for it
    for name, job in JOBS.items():
        e = job["expect"]
        inst = ("poly2", e["T"], e["MQ"], bool(e["il"])) if e["kernel"] == "poly2" else ("poly", job["dtype"], e["T"], e["MQ"], False)
        wanted.setdefault(inst, []).append(name)
    for key, job in ragged.JOBS.items():
        if key[0] == "default":
            wanted.setdefault(("poly", job["dtype"], job["t2"], job["mq"], True), []).append("ragged " + key[1])
    # what the logs say was launched: every polyphase line of every job
    launched = {}
    for name, job in JOBS.items():
        for f in _poly_lines(run_env(job["env"])["log_" + name]):
            launched.setdefault(instance_of(f), []).append(name)
    rres = ragged.run_child("default", tmp_path_factory)
    for key, job in ragged.JOBS.items():
        if key[0] == "default":
            for f in _poly_lines(rres["log_" + job["name"]]):
                launched.setdefault(instance_of(f), []).append("ragged " + key[1])
    mark = {}
    for inst in instances:
        assert (inst in wanted) != (inst in UNREACHABLE), "%r: %s" % (inst, "a case AND a reason" if inst in wanted else "neither a case nor a reason why it cannot be launched")
        if inst in UNREACHABLE:
            mark[inst] = "U"
        else:  # (the values of these jobs are checked by their own cases, here and in the ragged file: F = its jobs landed elsewhere)
            mark[inst] = "R" if set(wanted[inst]) <= set(launched.get(inst, [])) else "F"
    assert set(wanted) | set(UNREACHABLE) == set(instances), "a case or a reason for an instance poly_kernel does not have"
    taps, taps2 = parse_taps()
    print("census: R reached, F failed, U unreachable (tests/test_gpu_poly_instances.py UNREACHABLE)")
    print("%-26s %s" % ("T2", " ".join("%3d" % t for t in taps)))
    for kind in (F32, F64):
        for rg in (False, True):
            for mq in (0, 1, -1):
                print("%-26s %s" % ("k_poly %s MQ %2d%s" % (kind, mq, " ragged" if rg else ""), " ".join("%3s" % mark[("poly", kind, t, mq, rg)] for t in taps)))
    for il in (True, False):
        for mq in (0, 1):
            print("%-26s %s" % ("k_poly2 MQ %d %s" % (mq, "IL" if il else "split"), " ".join("%3s" % mark[("poly2", t, mq, il)] for t in taps2)))
    count = {m: sum(v == m for v in mark.values()) for m in "RFU"}
    print("census: %d R, %d F, %d U of %d" % (count["R"], count["F"], count["U"], len(instances)))
    for why in (R_T8, R_T56, R_MQ, R_PAIR, R_F64):
        print("  U %3d: %s" % (sum(v == why for v in UNREACHABLE.values()), why))
    for env_name, t in sorted(_wall.items()):
        print("child %s: %.1f s (time limit %d s)" % (env_name, t, TIMEOUT[env_name]))
    worst = {}
    for (name, what), v in _shares.items():
        k = (name[0], JOBS[name]["expect"]["kernel"], JOBS[name]["dtype"], what)
        if v > worst.get(k, (0, ""))[0]:
            worst[k] = (v, name)
    for k, (v, name) in sorted(worst.items()):
        print("largest share of its bar: leg %s %s %s %s: %.3f (%s)" % (k + (v, name)))
    named = [(inst, jobs) for inst, jobs in launched.items() if inst in UNREACHABLE or inst not in mark]
    assert not named, "a launch line names an unreachable instance: %r" % named
    assert (count["R"], count["F"], count["U"]) == (60, 0, 92), count
