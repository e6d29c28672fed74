"""GPU: ragged variable-rate batches — hipsoxr_run_device_vr_ragged, a clip table on a variable-rate plan with an io ratio per
clip (speed perturbation), as ONE launch of the VR && RAGGED form of k_interp, k_interp_wave or k_interp_tile
(csrc/kernels_interp.h; kernels.hip launch_ragged_vr).  The parent has neither the entry nor the keyword: every test here
fails there.

One child process per environment (tests/_vr_ragged_probe.py) on the debug-switch build, which writes one line per launch.
The probe makes the data (lengths are stated in units of U, the outputs of one column per workgroup of the form the job is to
reach: 256 lane, 32 wave, the KO of the job's own log line for the tile form) and returns every buffer as it lay in memory;
everything is compared here, bit for bit — no tolerance appears anywhere.

Reference A (every clip of every job): a fresh TensorStream(..., vr=True) of the product with the job's type, channel count,
dither flag and seed, set_io_ratio(r, 1.0), fed the clip with last=True — same frames, and the same frame count as
Plan.vr_out_len.  Reference B (three short clips of the mono wave jobs, per type): the CPU oracle driven by tests/vr_sim.py,
`VrSim(...).set_io_ratio(r); feed(x, last=True)` in port mode.
Ratios of one table: the plan's own, 1.0 (every output in one phase interval), 0.5, 0.9070294784580499 and the plan's ratio
x (1 - 2^-40); adjacent clips differ, two clips share one.
Memory guard: every buffer is pre-filled with a sentinel; one spare frame lies behind every clip of the output and must keep
it, and one behind every clip of the input, where a read past the clip's end would meet it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from vr_sim import VrSim

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DBG_LIB = os.path.join(os.path.dirname(HERE), "python-soxr_amd", "_variants", "dbg", "libhipsoxr.so")
SENTINEL = {"f32": 12345.0, "f64": 12345.0, "i32": 1234567, "i16": 12345}
NP = {"f32": np.float32, "f64": np.float64, "i32": np.int32, "i16": np.int16}
AUTO, GATHER, EXACT = 0, 1, 6

MAIN = (17600, 16000, "HQ")     # the largest io ratio: 1.1
STEEP = (48000, 44100, "VHQ")


def _ratios(case, n):
    top = case[0] / case[1]
    cyc = [top, 1.0, 0.5, 0.9070294784580499, top * (1 - 2.0 ** -40), 1.0, top]
    return [cyc[i % len(cyc)] for i in range(n)]


ENVS = {
    "default": {},
    "lane": {"HIPSOXR_NO_INTERP_WAVE": "1", "HIPSOXR_NO_INTERP_TILE": "1"},
    "tile": {"HIPSOXR_NO_INTERP_WAVE": "1"},
}
TIMEOUT = {"default": 240, "lane": 90, "tile": 180}

# a clip is [m, add, cut]: m U + add outputs wanted, out_frames = that - cut; ["in", n, cut]: n input frames outright.
# m in {0, 1, 2} x add in {-1, 0, +1}; an empty clip (0 frames); a clip shorter than taps / 2 (5 frames); one truncated clip
# (7 outputs below vr_out_len); the longest (clip 2) not last
BASE = [[0, 1, 0], [1, -1, 0], [2, 1, 0], [1, 0, 0], ["in", 0, 0], [1, 1, 0], [2, -1, 0], ["in", 5, 0], [2, 0, 0], [2, 0, 7], [0, 0, 0]]
CHECK_B = (0, 1, 9)             # reference B on the clips of 1, U - 1 and 2 U - 7 (truncated) outputs
# ... for the tile form further clips of U outputs, until the table reaches the form under the launcher's cost model: a
# variable-rate workgroup of KO outputs costs 116 lane-outputs each (kernels.hip interp_tile_form: 2.9e-4 against 2.5e-6 us per
# output x tap with the wave form off), 1.4x / 1.7x that as a pair, so with at most 256 workgroups a mono table needs more than
# 116 KO outputs and a stereo one more than 0.85 x 116 KO per channel: 11 + 125 clips, about 140 KO outputs per channel
TILE = BASE + [[1, 0, 0]] * 125

JOBS = {}  # (env, name) -> (job for the probe, expected kernel, {log field: value}, clips checked against reference B)


def _job(env, name, case, dtype, ch, clips, unit, kernel=EXACT, expect_kernel=None, expect=None, check=(), **kw):
    j = dict(name=name, case=list(case), dtype=dtype, ch=ch, clips=clips, unit=unit, kernel=kernel, seed=4000 + len(JOBS),
             ratios=_ratios(case, len(clips)))
    j.update(kw)
    JOBS[(env, name)] = (j, expect_kernel, expect or {}, tuple(check))


I16 = dict(dither=True, dither_seed=5, data="square", counter=True)   # full-scale square wave: the filter's overshoot saturates
# ---- default environment: the wave form.  Four types packed mono; the layouts once each; the other plan
_job("default", "wave_f32_1", MAIN, "f32", 1, BASE, 32, kernel=AUTO, expect_kernel="interp_wave", check=CHECK_B)
_job("default", "wave_f64_1", MAIN, "f64", 1, BASE, 32, expect_kernel="interp_wave", check=CHECK_B, table_dev=True)
_job("default", "wave_i32_1", MAIN, "i32", 1, BASE, 32, kernel=GATHER, expect_kernel="interp_wave", check=CHECK_B)
_job("default", "wave_i16_1", MAIN, "i16", 1, BASE, 32, kernel=AUTO, expect_kernel="interp_wave", check=CHECK_B, table_dev=True, **I16)
_job("default", "wave_f32_2", MAIN, "f32", 2, BASE, 32, expect_kernel="interp_wave")
_job("default", "wave_i16_3", MAIN, "i16", 3, BASE, 32, expect_kernel="interp_wave", table_dev=True, **I16)
_job("default", "wave_f64_2_split", MAIN, "f64", 2, BASE, 32, layout="split", expect_kernel="interp_wave")
_job("default", "wave_f32_2_strided", MAIN, "f32", 2, BASE, 32, layout="strided", expect_kernel="interp_wave", table_dev=True)
_job("default", "wave_vhq_f32_1", STEEP, "f32", 1, BASE, 32, expect_kernel="interp_wave", check=CHECK_B)
# ---- lane per output (wave and tile off)
_job("lane", "lane_f32_1", MAIN, "f32", 1, BASE, 256, kernel=AUTO, expect_kernel="interp", check=(0, 9))
_job("lane", "lane_i16_1", MAIN, "i16", 1, BASE, 256, expect_kernel="interp", table_dev=True, **I16)
_job("lane", "lane_f32_2", MAIN, "f32", 2, BASE, 256, expect_kernel="interp", expect=dict(ch_fast=1))
# ---- the tile form (wave off): mono, and stereo for the pair / twin mode
_job("tile", "tile_f32_1", MAIN, "f32", 1, TILE, "KO", expect_kernel="interp_tile", expect=dict(pair=0, twin=0))
_job("tile", "tile_f32_2", MAIN, "f32", 2, TILE, "KO", kernel=AUTO, expect_kernel="interp_tile", expect=dict(pair=1), table_dev=True)
_job("tile", "tile_i16_1", MAIN, "i16", 1, TILE, "KO", expect_kernel="interp_tile", expect=dict(pair=0, twin=0), **I16)

FOLD = dict(kind="fold", name="fold", case=list(MAIN), n_clips=65536, frames=3, cut=30000, seed=77, ratios=_ratios(MAIN, 7))
GUARD = dict(kind="guard", case=[48000, 44101, "HQ"], lengths=[700, 0, 33, 1500], seed=12)
PY = [dict(kind="py", name="py_f32_2", case=list(MAIN), dtype="f32", ch=2, seed=21, lengths=[3000, 1, 0, 700, 64], ratios=_ratios(MAIN, 5)),
      dict(kind="py", name="py_i16_1", case=list(MAIN), dtype="i16", ch=1, seed=22, lengths=[500, 0, 2000], ratios=[0.93, 1.1, 1.07], dither_seed=9)]

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
        tmp = tmp_path_factory.mktemp("vr_ragged_" + env_name)
        assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
        jobs = [j for (e, _), (j, _, _, _) in JOBS.items() if e == env_name]
        if env_name == "default":  # the guard is asked before everything else and after it
            jobs = [dict(GUARD, name="before")] + jobs + [FOLD] + PY + [dict(GUARD, name="after")]
        with open(tmp / "jobs.json", "w") as f:
            json.dump(jobs, f)
        env = {key: v for key, v in os.environ.items() if not key.startswith("HIPSOXR_")}
        env.update({"HIPSOXR_LIBRARY": DBG_LIB, "HIPSOXR_DEBUG_LAUNCH_LOG": str(tmp / "launch.log")})
        env.update(ENVS[env_name])
        try:
            r = subprocess.run([sys.executable, os.path.join(HERE, "_vr_ragged_probe.py"), str(tmp / "jobs.json"), str(tmp / "out.npz")],
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


def _lines(log):
    return [dict(tok.split("=", 1) for tok in ln.split()) for ln in str(log).split("\n") if ln.strip()]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.itemsize])


def _clips(key, res):
    """memory guard checked; -> [(x [n_in, ch], y [out_frames, ch])] per clip, from the buffers as they lay in memory"""
    job = JOBS[key][0]
    name, ch, table = job["name"], job["ch"], res["table_" + job["name"]]
    _, xf, xc, yf, yc = (int(v) for v in res["geom_" + name])
    x, y = res["x_" + name], res["y_" + name]
    assert y.dtype == NP[job["dtype"]]
    written, read = np.zeros(y.shape, bool), np.zeros(x.shape, bool)
    out = []
    for x0, n_in, y0, n_out in table:
        xi = x0 + np.arange(n_in)[:, None] * xf + np.arange(ch)[None, :] * xc
        yi = y0 + np.arange(n_out)[:, None] * yf + np.arange(ch)[None, :] * yc
        assert not written[yi].any(), "the test's clips overlap"
        written[yi], read[xi] = True, True
        out.append((x[xi], y[yi]))
    spare = y[~written]
    assert spare.size == ch * len(table), "one spare frame behind every clip"
    assert np.all(spare == SENTINEL[job["dtype"]]), "an element between packed clips (or behind the last) was written"
    assert np.all(x[~read] == SENTINEL[job["dtype"]]) and (~read).sum() >= ch * len(table), "the input gaps hold sentinels"
    return out


@pytest.mark.parametrize("key", sorted(JOBS), ids=lambda k: "%s-%s" % k)
def test_each_clip_is_the_variable_rate_stream_of_its_ratio(key, run_env, oracle):
    job, kernel, expect, check = JOBS[key]
    res = run_env(key[0])
    name, ch, dt = job["name"], job["ch"], NP[job["dtype"]]
    table, ratios = res["table_" + name], res["ratios_" + name]
    # ---- the launch: ONE line, the form by name, vr=1, ragged=<clips>, the longest clip's grid over all columns
    lines = _lines(res["log_" + name])
    assert len(lines) == 1, "one launch for the whole table: %r" % (lines,)
    ln = lines[0]
    assert ln["kernel"] == kernel and ln["vr"] == "1" and ln["ragged"] == str(len(table)), ln
    for k, v in expect.items():
        assert ln[k] == str(v), (k, ln)
    u = int(res["geom_" + name][0])
    gx, gy, _ = (int(v) for v in ln["grid"].split("x"))
    longest = int(table[:, 3].max())
    per_wg = {"interp": 256, "interp_wave": 32, "interp_tile": int(ln.get("KO", 0))}[kernel]
    assert per_wg == u, "the lengths were made for this form's unit"
    if kernel == "interp" and ln["ch_fast"] == "1":
        assert (gx, gy) == (-(-longest * ch // 256), len(table))
    else:
        cols = len(table) * (ch // 2 if ln.get("pair") == "1" else ch)
        assert (gx, gy) == (-(-longest // per_wg), cols)
    assert longest == 2 * u + 1 and sorted(set(int(v) for v in table[:, 3]))[:2] == [0, 1], "the table holds what it was made to hold"
    # ---- reference A: frames and frame count of the per-clip streams
    clips = _clips(key, res)
    refa, lens = res["refa_" + name], res["refa_len_" + name]
    assert refa.dtype == dt
    pos, truncated = 0, 0
    for c, ((x, y), n_ref) in enumerate(zip(clips, lens)):
        ref = refa[pos * ch:(pos + n_ref) * ch].reshape(n_ref, ch)
        pos += n_ref
        n_out = len(y)
        # (a clip made for `want` outputs may own one more at a ratio below 1: the least input that reaches them)
        assert n_ref - 8 <= n_out <= n_ref and (n_out == n_ref or job["clips"][c][0] != "in"), (c, n_out, n_ref)
        truncated += n_ref - n_out >= 7
        assert np.array_equal(_bits(y), _bits(ref[:n_out])), "clip %d (ratio %r, %d -> %d frames)" % (c, ratios[c], len(x), n_out)
    assert truncated == 1 and pos * ch == len(refa)
    assert int(lens[4]) == 0 and len(clips[4][0]) == 0 and len(clips[7][0]) == 5 and int(lens[7]) > 0, "the empty and the short clip"
    # ---- the clip counter: the sum of the streams' counts, and not zero
    # (a stream counts all of its frames, so the equality is asked of the same clips with nothing cut — the probe's second
    #  launch, whose frames are the streams' whole output; the job itself counts its own frames: at most `dropped` fewer)
    got_count, stream_count, full_count = (int(v) for v in res["count_" + name])
    if job.get("counter"):
        assert stream_count > 0, "the square wave saturates the streams' outputs"
        assert full_count == stream_count
        assert np.array_equal(_bits(res["full_" + name]), _bits(refa))
        dropped = (int(lens.sum()) - int(table[:, 3].sum())) * ch
        assert 7 * ch <= dropped and stream_count - dropped <= got_count <= stream_count and got_count > 0
    # ---- reference B: the CPU oracle on the independent clock
    oracle_clips = 0
    for c in check:
        x, y = clips[c]
        sim = VrSim(_Seeded(oracle, job), job["case"][0], job["case"][1], job["case"][2], dt)
        sim.set_io_ratio(float(ratios[c]), 0)
        want = sim.feed(x[:, 0], last=True)
        assert len(want) >= len(y) > 0
        assert np.array_equal(_bits(y[:, 0]), _bits(want[:len(y)].astype(dt))), "clip %d against the oracle" % c
        oracle_clips += sim.o.clips
    if check and job.get("counter"):
        assert oracle_clips > 0, "chosen on the CPU oracle: these clips saturate, the counter cannot pass on zero"


class _Seeded:
    """the oracle with the job's dither flag and seed in its output stage (VrSim passes channel and position alone)"""

    def __init__(self, o, job):
        self._o, self._dither, self._seed, self.clips = o, bool(job.get("dither", False)), int(job.get("dither_seed", 0)), 0

    def __getattr__(self, n):
        return getattr(self._o, n)

    def quantize(self, v, dtype, channel=0, k0=0):
        q, n = self._o.quantize(v, dtype, channel=channel, k0=k0, dither=self._dither, seed=self._seed)
        self.clips += n
        return q, n


def test_more_columns_than_the_grid_holds_fold_into_two_launches(run_env):
    res = run_env("default")
    lines, lines2 = _lines(res["log_fold"]), _lines(res["log2_fold"])
    assert [ln["ragged"] for ln in lines] == ["65535", "1"] and all(ln["vr"] == "1" and ln["kernel"] == "interp_wave" for ln in lines)
    assert [ln["ragged"] for ln in lines2] == ["30000", "35536"]
    y, y2, table = res["y_fold"], res["y2_fold"], res["table_fold"]
    assert np.array_equal(_bits(y), _bits(y2)), "the fold's two ranges against the same table as two jobs"
    assert len(table) == 65536 and np.all(table[:, 1] == 3) and sorted(set(int(v) for v in table[:, 3])) == [3, 6]
    ends = table[:, 2] + table[:, 3]
    assert np.all(y[ends] == 12345.0) and (y != 12345.0).sum() == int(table[:, 3].sum()), "one spare frame behind every clip, all else written"
    pos = 0
    for c, n in zip(res["picks_fold"], res["pickref_len_fold"]):
        y0, n_out = int(table[c, 2]), int(table[c, 3])
        assert n == n_out and np.array_equal(_bits(y[y0:y0 + n_out]), _bits(res["pickref_fold"][pos:pos + n])), c
        pos += n


@pytest.mark.parametrize("job", PY, ids=lambda j: j["name"])
def test_python_surface(job, run_env):
    res = run_env("default")
    name = job["name"]
    lines = _lines(res["log_" + name])
    assert len(lines) == 1 and lines[0]["vr"] == "1" and lines[0]["ragged"] == str(len(job["lengths"])), lines
    assert np.array_equal(res["lens_" + name], res["refa_len_" + name]), "vr_out_len is the stream's frame count"
    assert res["lens_" + name].min() == 0 and res["lens_" + name].max() > 600
    assert np.array_equal(_bits(res["vs_" + name]), _bits(res["refa_" + name])), "resample_varispeed against the streams"
    assert np.array_equal(_bits(res["job_" + name]), _bits(res["refa_" + name])), "RaggedJob(io_ratios=...) on a second torch stream"
    assert res["inplace_" + name].all(), "clips are used where they lie"
    if job["dtype"] in ("f32", "f64"):
        assert "no gradient is served" in str(res["grad_" + name])


def test_what_existed_before_is_unchanged_after(run_env):
    """The RAGGED argument structs grew a clock pointer and the VR kernels a branch: a constant-rate ragged job of an
    interpolated-phase plan and a variable-rate stream with a slew return after the new launches what they returned before
    them — and the ragged job what each clip returns alone."""
    res = run_env("default")
    for k in ("ragged_", "stream_", "solo_"):
        assert np.array_equal(_bits(res[k + "before"]), _bits(res[k + "after"])), k
    lines = _lines(res["log_after"])
    assert len(lines) == 1 and lines[0]["vr"] == "0" and lines[0]["ragged"] == "4" and lines[0]["kernel"] == "interp_wave"
    y, solo = res["ragged_after"], res["solo_after"]
    assert y[-1] == 12345.0 and np.array_equal(_bits(y[:-1]), _bits(solo))
    assert len(res["stream_after"]) > 3000
