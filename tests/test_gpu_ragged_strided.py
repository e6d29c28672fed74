"""GPU: clip tables of INTERLEAVED and STRIDED clips — `[frames, channels]`, the layout dist.RaggedJob builds for every
multichannel clip — on the frequency-domain engine and on the two-stage form.

Exact-bank plans, the engine BY NAME (KERNEL_FFT, KERNEL_FFT_PCM): ONE launch of k_fft_strided2, whose workgroups read their
clip's row of the table (csrc/fft.hip; the work-item map and the table conditions are csrc/fft_ragged_rules.h) — channel pairs
(CP = true: even channel counts, float32 / float64 / int16) or single columns at a frame stride (CP = false).  The parent
refuses every one of these jobs ("FFT engine unavailable for this ragged job"), so these tests fail without the feature.
Interpolated-phase plans under KERNEL_AUTO: the two-stage form over the table (csrc/twostage.hip launch_two_stage_ragged) with
the caller's frame stride on the caller's side of both stages — one ragged polyphase launch, one ragged FFT-stage launch, one
ragged launch of the exact engine for the short clips — where the parent ran two launches per admitted clip.

One child process per environment (tests/_ragged_strided_probe.py) on the debug-switch build, with a time limit of its own;
after a failed child nothing further is started from this file.  The probe makes the tables and returns every buffer as it
lay in memory; everything is compared here.  Environments: the default; HIPSOXR_FFT_NO_XCD_MAP (the stereo job again: it takes
the strided form without the map).

Tables (exact bank): nine clips in units of the job's own hop_out H — out frames {0, 1, H-1, H, H+1, 2H+1, 19H+5, 3H+3
truncated by 7 below out_len, 2H}, shuffled, the longest (20 blocks: more than one item per XCD in both forms) not last.
Values: every clip and channel against oracle.resample(..., mode="ref"), the float64 direct form: relative RMS <= 1e-6
(float32) / 2e-9 (float64, VHQ) of max(rms(ref), 0.05); the first and last 300 outputs on their own within 4 tol 0.25 — the
bars of tests/test_gpu_dist.py::test_ragged_job_is_one_launch_of_the_fft_engine.  int16: equal to oracle.quantize of the
float32 ragged KERNEL_FFT job of the same table, per column, with the same seed, and the counter to the host's count — the
identity of tests/test_gpu_fft_pcm.py.  Bitwise anchor: five equal-length clips at a constant distance as a table and as one
equal-length batch at that clip stride — the same row, the same kernel, the same bits.
Memory: every element outside the clips' outputs (one spare frame behind every clip) keeps the sentinel; no payload element does
(float buffers; an int16 result may hold the sentinel's value by right, and its payload is pinned by the identity above)."""
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
SENTINEL = {"f32": 12345.0, "f64": 12345.0, "i16": 12345}
NP = {"f32": np.float32, "f64": np.float64, "i16": np.int16}
TOL = {"f32": 1e-6, "f64": 2e-9}
AUTO, FFT, FFT_PCM = 0, 5, 9

ENVS = {"default": {}, "nomap": {"HIPSOXR_FFT_NO_XCD_MAP": "1"}}
TIMEOUT = {"default": 300, "nomap": 120}

JOBS = {}  # (env, name) -> job for the probe (+ "form": the launch form its log line must show)


def _job(env, name, kind, **kw):
    j = dict(name=name, kind=kind, seed=9000 + len(JOBS))
    j.update(kw)
    JOBS[(env, name)] = j


VHQ, HQ, UP, DOWN = [48000, 44100, "VHQ"], [48000, 44100, "HQ"], [44100, 48000, "HQ"], [44100, 16000, "HQ"]
# CP = true: one (Real, Real) word per frame
_job("default", "cp_vhq_f32_2", "fft", case=VHQ, dtype="f32", ch=2, kernel=FFT, form="strided2_cp")
_job("default", "cp_vhq_f64_4", "fft", case=VHQ, dtype="f64", ch=4, kernel=FFT, form="strided2_cp")
_job("default", "cp_up_hq_f32_2", "fft", case=UP, dtype="f32", ch=2, kernel=FFT, form="strided2_cp")
_job("default", "cp_down_hq_f32_8", "fft", case=DOWN, dtype="f32", ch=8, kernel=FFT, form="strided2_cp")
_job("default", "cp_hq_i16_2_dither", "fft", case=HQ, dtype="i16", ch=2, kernel=FFT_PCM, dither=True, dither_seed=5, form="strided2_cp")
_job("default", "cp_hq_i16_2_counter", "fft", case=HQ, dtype="i16", ch=2, kernel=FFT_PCM, dither=True, dither_seed=5, data="square", counter=True,
     form="strided2_cp")
# CP = false: one column at a frame stride
_job("default", "st_vhq_f32_3", "fft", case=VHQ, dtype="f32", ch=3, kernel=FFT, form="strided2_st")
_job("default", "st_vhq_f64_3", "fft", case=VHQ, dtype="f64", ch=3, kernel=FFT, form="strided2_st")
_job("default", "st_vhq_f32_col2", "fft", case=VHQ, dtype="f32", ch=1, kernel=FFT, layout="col2", form="strided2_st")
# without the XCD map: the stereo job on the strided form, plain (item, column) ids
_job("nomap", "cp_vhq_f32_2", "fft", case=VHQ, dtype="f32", ch=2, kernel=FFT, form="strided2_st", seed=JOBS[("default", "cp_vhq_f32_2")]["seed"])
FFT_JOBS = [k for k, j in JOBS.items() if j["kind"] == "fft"]
FLOAT_JOBS = [k for k in FFT_JOBS if JOBS[k]["dtype"] != "i16"]
PCM_JOBS = [k for k in FFT_JOBS if JOBS[k]["dtype"] == "i16"]

_job("default", "anchor_cp", "anchor", case=VHQ, dtype="f32", ch=2, frames=30011, form="strided2_cp")
_job("default", "anchor_st", "anchor", case=VHQ, dtype="f32", ch=3, frames=30011, form="strided2_st")
_job("default", "refusal_i16_odd", "refusal", case=HQ)

# the two-stage form: nine clips in units of the polyphase tile, admitted and short ones mixed
_job("default", "ts_down_f32_2", "twostage", case=[48000, 44101, "HQ"], dtype="f32", ch=2)
_job("default", "ts_up_f64_2", "twostage", case=[44101, 48000, "VHQ"], dtype="f64", ch=2)
_job("default", "ts_steep_f32_3", "twostage", case=[44100, 16001, "HQ"], dtype="f32", ch=3)
TS_JOBS = [k for k, j in JOBS.items() if j["kind"] == "twostage"]

_job("default", "py_ragged", "py_ragged", case=[48000, 44101, "HQ"], lengths=[9000, 150, 0, 12000, 8500])
_job("default", "py_batch", "py_batch", case=[48000, 44100, "HQ"], lengths=[3000, 12000, 1, 7000, 5, 9000, 20000], block_bytes=120000)

_child_failed = []  # a fault, abort or time limit in a child: nothing further is started on the GPU from this file
_results = {}


@pytest.fixture(autouse=True)
def _nothing_after_a_failed_child():
    if _child_failed:
        pytest.fail("a probe process failed (%s): no further GPU work from this file" % _child_failed[0])


@pytest.fixture(scope="module")
def run_env(tmp_path_factory):
    """-> the results of one environment's child process (started on first use, once)"""
    def run(env_name):
        if env_name in _results:
            return _results[env_name]
        if _child_failed:
            pytest.fail("a probe process failed (%s): no further GPU work from this file" % _child_failed[0])
        tmp = tmp_path_factory.mktemp("ragged_strided_" + env_name)
        assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
        with open(tmp / "jobs.json", "w") as f:
            json.dump([j for (e, _), j in JOBS.items() if e == env_name], f)
        env = {key: v for key, v in os.environ.items() if not key.startswith("HIPSOXR_")}
        env.update({"HIPSOXR_LIBRARY": DBG_LIB, "HIPSOXR_DEBUG_LAUNCH_LOG": str(tmp / "launch.log")})
        env.update(ENVS[env_name])
        t0 = time.time()
        try:
            r = subprocess.run([sys.executable, os.path.join(HERE, "_ragged_strided_probe.py"), str(tmp / "jobs.json"), str(tmp / "out.npz")],
                               env=env, capture_output=True, text=True, timeout=TIMEOUT[env_name])
        except subprocess.TimeoutExpired:
            _child_failed.append("%s: time limit" % env_name)
            raise
        if r.returncode != 0:
            _child_failed.append("%s: exit status %d" % (env_name, r.returncode))
        assert r.returncode == 0, r.stderr[-3000:]
        print("ragged strided child %s: %.1f s (time limit %d s)" % (env_name, time.time() - t0, TIMEOUT[env_name]))
        _results[env_name] = np.load(tmp / "out.npz")
        return _results[env_name]
    return run


def _lines(log):
    return [dict(tok.split("=", 1) for tok in ln.split()) for ln in str(log).split("\n") if ln.strip()]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.itemsize])


def _rms(v):
    return float(np.sqrt(np.mean(np.square(v, dtype=np.float64)))) if len(v) else 0.


def _ids(keys):
    return ["%s-%s" % k for k in keys]


def _clips(key, res, ybuf=None, sentinel=None):
    """memory guard checked; -> [(x [n_in, ch], y [out_frames, ch])] per clip, from the buffers as they lay in memory"""
    job = JOBS[key]
    name, ch, table = job["name"], job["ch"], res["table_" + job["name"]]
    _, _, xf, xc, yf, yc = (int(v) for v in res["geom_" + name])
    x, y = res["x_" + name], (res["y_" + name] if ybuf is None else ybuf)
    sent = SENTINEL[job["dtype"]] if sentinel is None else sentinel
    if ybuf is None:
        assert y.dtype == NP[job["dtype"]]
    written = np.zeros(y.shape, bool)
    out = []
    for x0, n_in, y0, n_out in table:
        xi = x0 + np.arange(n_in)[:, None] * xf + np.arange(ch)[None, :] * xc
        yi = y0 + np.arange(n_out)[:, None] * yf + np.arange(ch)[None, :] * yc
        assert not written[yi].any(), "the test's clips overlap"
        written[yi] = True
        out.append((x[xi], y[yi]))
    for x0, n_in, y0, n_out in table:  # one spare frame behind every clip
        assert not any(written[y0 + n_out * yf + c * yc] for c in range(ch)), "the test's table leaves no spare frame"
    assert np.all(y[~written] == sent), "an element outside the clips' outputs was written"
    if y.dtype != np.int16:  # (an int16 result may hold the sentinel's value by right: there the identity with the float job's
        for c, (_, yv) in enumerate(out):  # values, whose own buffer is checked here, says that every payload element was written)
            assert not np.any(yv == sent), "%s clip %d: a payload element was not written" % (key, c)
    return out


def _check_against_ref(oracle, case, x, y, tol, what):
    """one clip [frames, ch] against the float64 direct form: the whole clip, and its first and last 300 outputs on their own"""
    worst = 0.
    for ch in range(x.shape[1]):
        ref = oracle.resample(np.ascontiguousarray(x[:, ch]).astype(np.float64), *case, mode="ref")
        assert len(ref) >= len(y), what
        ref, got = ref[:len(y)], y[:, ch].astype(np.float64)
        if not len(ref):
            continue
        err = _rms(got - ref) / max(_rms(ref), 0.05)
        worst = max(worst, err)
        assert err <= tol, "%s channel %d: %.3g" % (what, ch, err)
        w = min(len(ref), 300)
        assert _rms(got[:w] - ref[:w]) <= 4 * tol * 0.25 and _rms(got[-w:] - ref[-w:]) <= 4 * tol * 0.25, "%s channel %d: head / tail" % (what, ch)
    return worst


# ---- exact-bank plans: the frequency-domain engine by name -----------------------------------------------------------------
@pytest.mark.parametrize("key", FFT_JOBS, ids=_ids(FFT_JOBS))
def test_one_launch_of_the_strided_kernel(key, run_env):
    """exactly one form=strided2_cp / strided2_st line per job, ending in ragged=<columns>; the table holds the lengths it was
    to hold in units of the line's own hop_out; the grid is the longest clip's"""
    job = JOBS[key]
    res = run_env(key[0])
    log = str(res["log_" + job["name"]])
    lines = _lines(log)
    assert len(lines) == 1, "one launch per ragged job: %r" % log
    f, ch = lines[0], job["ch"]
    table = res["table_" + job["name"]]
    assert f["form"] == job["form"] and f["window"] == "0", f
    assert log.strip().endswith(" ragged=%d" % (len(table) * ch)), log
    assert f["kind"] == job["dtype"], f
    h = int(f["hop_out"])
    assert h == int(res["geom_" + job["name"]][0]), "the table was made for the launcher's own block size"
    outs = [int(v) for v in table[:, 3]]
    assert outs == [h + 1, 0, 19 * h + 5, 1, 3 * h + 3 - 7, h - 1, 2 * h + 1, h, 2 * h]
    assert max(outs) < 100000 and int(f["n_blocks"]) == 20
    gx, gy, gz = (int(v) for v in f["grid"].split("x"))
    if key[0] == "nomap" or ch == 1:   # plain ids: pairs of blocks along x, (clip, channel) columns along y
        assert (gx, gy, gz) == (10, len(table) * ch, 1)
    else:                              # the XCD map: the longest clip's items, rounded up to 8, times the channel units; the clip in y
        items, units = (20, ch // 2) if job["form"] == "strided2_cp" else (10, ch)
        assert (gx, gy, gz) == (-(-items // 8) * 8 * units, len(table), 1) and items > 8


@pytest.mark.parametrize("key", FLOAT_JOBS, ids=_ids(FLOAT_JOBS))
def test_float_clips_match_the_oracle_and_memory_is_kept(key, run_env, oracle):
    job = JOBS[key]
    res = run_env(key[0])
    worst = 0.
    for c, (x, y) in enumerate(_clips(key, res)):
        worst = max(worst, _check_against_ref(oracle, job["case"], x, y, TOL[job["dtype"]], "%s-%s clip %d of %d frames" % (key[0], key[1], c, len(y))))
    print("ragged strided %s-%s: worst relative RMS %.3g (bar %.0e)" % (key[0], key[1], worst, TOL[job["dtype"]]))


@pytest.mark.parametrize("key", PCM_JOBS, ids=_ids(PCM_JOBS))
def test_int16_is_the_float_job_through_the_output_stage(key, run_env, oracle):
    """int16 channel pairs == oracle.quantize of the float32 ragged KERNEL_FFT job of the same table, per column, same seed,
    dither keyed by the output index within the clip; the counter == the host's count"""
    job = JOBS[key]
    res = run_env(key[0])
    name = job["name"]
    flines = _lines(res["logf_" + name])
    assert len(flines) == 1 and flines[0]["form"] == "strided2_cp" and flines[0]["hop_out"] == _lines(res["log_" + name])[0]["hop_out"], flines
    got = _clips(key, res)
    flt = _clips(key, res, ybuf=res["yf_" + name], sentinel=SENTINEL["f32"])
    clips, ndiff, total = 0, 0, 0
    for c, ((_, y), (_, yf)) in enumerate(zip(got, flt)):
        for ch in range(job["ch"]):
            want, n = oracle.quantize(np.ascontiguousarray(yf[:, ch]), np.int16, channel=ch, k0=0, dither=job["dither"], seed=job["dither_seed"])
            clips += n
            ndiff += int(np.count_nonzero(y[:, ch] != want))
            total += len(want)
    count = int(res["count_" + name][0])
    print("ragged strided %s: %d of %d differ, device clips %d host clips %d" % (name, ndiff, total, count, clips))
    assert ndiff == 0
    if job.get("counter"):
        assert clips > 0, "the test's data does not clip"
        assert count == clips


@pytest.mark.parametrize("name", ["anchor_cp", "anchor_st"])
def test_a_table_of_equal_clips_has_the_bits_of_the_equal_length_batch(name, run_env):
    """five equal-length clips at a constant distance: the table's launch and the equal-length batch job with that clip stride
    take the same row, the same kernel and the same arithmetic"""
    res = run_env("default")
    job = JOBS[("default", name)]
    a, b = _lines(res["log_" + name]), _lines(res["logeq_" + name])
    assert len(a) == 1 and len(b) == 1, (a, b)
    assert a[0]["form"] == job["form"] == b[0]["form"] and a[0]["ragged"] == str(5 * job["ch"]) and "ragged" not in b[0]
    for field in ("L", "M", "k", "small", "nt", "lds", "grid"):
        assert a[0][field] == b[0][field], (field, a[0], b[0])
    y, yeq, table = res["y_" + name], res["yeq_" + name], res["table_" + name]
    assert np.array_equal(_bits(y), _bits(yeq)), "%d elements differ" % int(np.count_nonzero(_bits(y) != _bits(yeq)))
    payload = np.zeros(y.shape, bool)
    for _, _, y0, n_out in table:
        payload[y0:y0 + n_out * job["ch"]] = True
    assert np.all(y[~payload] == SENTINEL["f32"]) and not np.any(y[payload] == SENTINEL["f32"])


def test_an_int16_table_at_an_odd_offset_is_refused_by_name(run_env):
    res = run_env("default")
    assert "FFT engine (integer samples) unavailable for this ragged job" in str(res["err_refusal_i16_odd"])
    assert np.all(res["y_refusal_i16_odd"] == SENTINEL["i16"]), "a refused job wrote"
    assert [f for f in _lines(res["log_refusal_i16_odd"]) if f.get("form") != "none"] == []


# ---- interpolated-phase plans under KERNEL_AUTO: the two-stage form -----------------------------------------------------------
def _admitted(row):
    return min(int(row[1]), int(row[3])) >= 8192


def _two_stage_lines(log, up, admitted_cols, short):
    """exactly one kernel=poly line with ragged=<admitted columns>, one FFT line with the same, one interp* line with
    ragged=<short non-empty clips>, in the direction's order"""
    lines = _lines(log)
    kinds = ["fft" if "form" in f else "poly" if f.get("kernel") in ("poly", "poly2") else "interp" if str(f.get("kernel", "")).startswith("interp") else "?"
             for f in lines]
    assert kinds == (["fft", "poly"] if up else ["poly", "fft"]) + ["interp"], "a constant number of launches: %r" % str(log)
    poly, fft, interp = lines[kinds.index("poly")], lines[kinds.index("fft")], lines[2]
    assert poly["kernel"] == "poly" and poly["ragged"] == str(admitted_cols) == fft["ragged"], (poly, fft)
    assert fft["form"] == "strided2_st" and fft["window"] == "0", fft
    assert interp["ragged"] == str(short), interp
    return poly


@pytest.mark.parametrize("key", TS_JOBS, ids=_ids(TS_JOBS))
def test_two_stage_is_a_constant_number_of_launches(key, run_env):
    job = JOBS[key]
    res = run_env(key[0])
    table = res["table_" + job["name"]]
    admitted = [r for r in table if _admitted(r)]
    short = [r for r in table if r[3] > 0 and not _admitted(r)]
    assert len(admitted) == 6 and len(short) == 2 and len(table) == 9, "the probe's table: six admitted clips, two short ones, one empty"
    poly = _two_stage_lines(res["log_" + job["name"]], job["case"][1] > job["case"][0], len(admitted) * job["ch"], len(short))
    u, m = (int(v) for v in res["geom_" + job["name"]][:2])
    assert 256 * int(poly["R"]) == u, "the table was made for the launcher's own R"
    outs = [int(v) for v in table[:, 3]]
    assert outs[1:7] == [m * u, m * u - 1, (m + 5) * u + 77, m * u + 1, (m + 2) * u + 3, 0] and outs[7] == 100
    assert int(poly["width"]) == {"f32": 4, "f64": 8}[job["dtype"]] and poly["il"] == "0" and poly["split"] == "0", poly


@pytest.mark.parametrize("key", TS_JOBS, ids=_ids(TS_JOBS))
def test_two_stage_columns_match_the_oracle_and_memory_is_kept(key, run_env, oracle):
    """windows of 3000 outputs at the head, the tail and one interior tile edge of every admitted column against the oracle's
    float64 direct form; short clips bit-equal to the clip alone on the exact engine; the sentinels"""
    job = JOBS[key]
    res = run_env(key[0])
    got = _clips(key, res)
    table, u = res["table_" + job["name"]], int(res["geom_" + job["name"]][0])
    pl = oracle.plan(*job["case"])
    tol, worst = TOL[job["dtype"]], 0.
    flat, pos = res["short_" + job["name"]], 0
    for c, (x, y) in enumerate(got):
        if table[c][3] == 0:
            continue
        if not _admitted(table[c]):
            want = flat[pos:pos + y.size].reshape(y.shape)
            pos += y.size
            assert np.array_equal(_bits(y), _bits(want)), "%s clip %d of %d frames" % (key, c, len(y))
            continue
        n_out = y.shape[0]
        edge = (n_out // (2 * u)) * u
        for ch in range(job["ch"]):
            for k0 in (0, n_out - 3000, edge - 1500):
                ref = oracle.resample_channel(pl, np.ascontiguousarray(x[:, ch]).astype(np.float64), "ref", k0=k0, n_out=3000)
                err = _rms(y[k0:k0 + 3000, ch].astype(np.float64) - ref) / max(_rms(ref), 0.05)
                worst = max(worst, err)
                assert err <= tol, "%s clip %d channel %d window at %d: %.3g" % (key, c, ch, k0, err)
    assert pos == flat.size and pos > 0
    print("ragged strided two-stage %s: worst relative RMS %.3g (bar %.0e)" % (key[1], worst, tol))


def test_resample_ragged_on_stereo_clips(run_env, oracle):
    """dist.resample_ragged(plan, stereo clips) forward under defaults: three launches; admitted clips in the two-stage class of
    the oracle, short clips bit-equal to the clip alone on the exact engine"""
    res = run_env("default")
    job = JOBS[("default", "py_ragged")]
    _two_stage_lines(res["log_py_ragged"], False, 2 * 2, 2)
    pl = oracle.plan(*job["case"])
    x, y, ex, xp, yp = res["x_py_ragged"], res["y_py_ragged"], res["exact_py_ragged"], 0, 0
    assert y.dtype == np.float32 and y.shape == ex.shape
    for n, n_out in zip(job["lengths"], (int(v) for v in res["nout_py_ragged"])):
        xc, got, alone = x[xp:xp + 2 * n].reshape(n, 2), y[yp:yp + 2 * n_out].reshape(n_out, 2), ex[yp:yp + 2 * n_out].reshape(n_out, 2)
        if min(n, n_out) >= 8192:
            for ch in range(2):
                for k0 in (0, n_out - 3000):
                    ref = oracle.resample_channel(pl, np.ascontiguousarray(xc[:, ch]).astype(np.float64), "ref", k0=k0, n_out=3000)
                    assert _rms(got[k0:k0 + 3000, ch].astype(np.float64) - ref) <= 1e-6 * max(_rms(ref), 0.05), (n, ch, k0)
            assert not np.array_equal(got, alone), "an admitted clip is the two-stage form's, not the exact engine's"
        else:
            assert np.array_equal(_bits(got), _bits(alone)), n
        xp, yp = xp + 2 * n, yp + 2 * n_out
    assert yp == len(y)


def test_resample_batch_stereo_host_corpus_by_name(run_env, oracle):
    """dist.resample_batch(stereo float32 host clips, kernel=KERNEL_FFT) on 48000 -> 44100: one FFT launch per block of the
    staging ring, every clip within the engine's bar"""
    res = run_env("default")
    job = JOBS[("default", "py_batch")]
    blocks = [int(b) for b in res["blocks_py_batch"]]
    assert len(blocks) >= 3
    lines = _lines(res["log_py_batch"])
    assert [f.get("form") for f in lines] == ["strided2_cp"] * len(blocks), lines
    assert [int(f["ragged"]) for f in lines] == [2 * b for b in blocks]
    x, y, xp, yp = res["x_py_batch"], res["y_py_batch"], 0, 0
    for n, n_out in zip(job["lengths"], (int(v) for v in res["nout_py_batch"])):
        _check_against_ref(oracle, job["case"], x[xp:xp + 2 * n].reshape(n, 2), y[yp:yp + 2 * n_out].reshape(n_out, 2), 1e-6, "clip of %d frames" % n)
        ref_len = len(oracle.resample(np.zeros(n), *job["case"], mode="ref"))
        assert n_out == ref_len, n
        xp, yp = xp + 2 * n, yp + 2 * n_out
    assert yp == len(y)
