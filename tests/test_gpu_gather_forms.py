"""GPU: every launch form of the exact-bank half of launch_gather (csrc/kernels.hip) against the oracle.

An exact-bank plan (48k <-> 44.1k, 44.1k -> 16k and every other small ratio) that is not served by a period tile goes, per
launch: to k_gather_wave from 4096 outputs on, where T >= 32 and wave_geom fits 64 KiB of LDS; else to k_chain (mode 0) below
4096 outputs where chain_geom fits 150 KiB — 8 outputs per workgroup up to 512 outputs, 32 above, halved while LDS is short;
else to lane-per-output k_gather.  Constant-rate device streams run k_chain_multi (one launch appends the chunk, moves a full
ring and computes), variable-rate streams k_chain mode 2 / k_interp_wave / k_interp.  The debug-switch build writes one line
per launch (HIPSOXR_DEBUG_LAUNCH_LOG), so a case here names the form its launch must show and the test reads it from the
log — the rules are not restated.  One child process per environment (tests/_gather_forms_probe.py) runs that
environment's jobs into guarded, NaN- / sentinel-filled buffers; everything is compared here.

Per job: the log shows the stated form — a case is resized, never its assertion changed, if a later launch rule moves it; 8
guard frames either side of every clip untouched and every payload element written; the whole payload equal to the oracle bit
for bit (oracle.resample_channel in the canonical order of the type's engine over the whole signal, then oracle.quantize for
integers: dither keyed by (seed, channel, output index)).  There is no tolerance in this file.  Column 0 of every job is a
prefix of ONE structured signal — two tones and a staircase, scaled to the type — every other column is noise of its own:
jobs of one plan and type see the same input, so whatever form served them, the outputs whose windows lie inside the shorter
input have the same bits (test_cross_form_identity).

Streams: the reference is the oracle on the whole signal, cut at the frame counts the calls returned, and those counts are
the integer model's of tests/test_gpu_stream_schedule.py (variable rate: tests/vr_sim.py).

What the plans reach (numbers from oracle/design.py; tests/test_design_independent.py holds the product to it):
  A 48000 -> 44100 VHQ  147 / 160 / 296    H = 148.  Chain: blocks plus a 20-tap tail (f32), a 4-tap tail (f64).  Wave: full = 9,
                                            last step 4 taps
  B 44100 -> 16000 VHQ  160 / 441 / 736    wave: full = 23, no short step, first look-ahead loop; chain: 16-tap tail
  C 48000 -> 44100 HQ   147 / 160 / 216    wave: full = 6 (< 8), last step 12 taps
  D 48000 -> 44100 LQ   147 / 160 / 48     H = 24 < 32: chain tail only; wave: full = 1, last step 8 taps
  E 48000 -> 44100 QQ   147 / 160 / 8      T < 32: the right half starts at i < 0; no wave form, >= 4096 outputs run k_gather
  F 44100 -> 12000 VHQ  40 / 147 / 976     two staging trips (T > 768); span ~1002 at NO = 8, ~1090 at NO = 32: either side of
                                            store_span's 4 x 256
  G 192000 -> 8000 VHQ  1 / 24 / 6376      L = 1, nine trips; NO falls to 4 (f32) and 2 (f64, i32: 153 536 of 153 600 bytes)
  H 384000 -> 8000 VHQ  1 / 48 / 12752     f32: NO = 2; f64: neither chain_geom nor wave_geom fits, k_gather at every length
Not reached: the L >= 2^31 division branch of chain_body (a bank is L x T coefficients: no exact bank has such an L); the
resident form, k_wave_dot, the ragged forms, the tiles, both FFT engines and the 2^30-output split have files of their own or
are out of this file's scope."""
import functools
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from test_gpu_stream_schedule import BIG, Model
from vr_sim import VrSim

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DBG_LIB = os.path.join(os.path.dirname(HERE), "python-soxr_amd", "_variants", "dbg", "libhipsoxr.so")
GUARD, POISON = 8, 12345
SENT = {"i16": -12345, "i32": -123456789}
DTYPE = {"f32": np.float32, "f64": np.float64, "i16": np.int16, "i32": np.int32}
WIDTH = {"f32": 4, "f64": 8, "i16": 4, "i32": 8}            # the engine's precision
SCALE = {"f32": 1.0, "f64": 1.0, "i16": 8000.0, "i32": 2.0 ** 28}
LOUD = {"i16": 5.0, "i32": 16.0}

A = (48000, 44100, "VHQ")
B = (44100, 16000, "VHQ")
C = (48000, 44100, "HQ")
D = (48000, 44100, "LQ")
E = (48000, 44100, "QQ")
F = (44100, 12000, "VHQ")
G = (192000, 8000, "VHQ")
H = (384000, 8000, "VHQ")
PLAN_SHAPE = {A: (147, 160, 296), B: (160, 441, 736), C: (147, 160, 216), D: (147, 160, 48), E: (147, 160, 8),
              F: (40, 147, 976), G: (1, 24, 6376), H: (1, 48, 12752)}   # case -> (L, M, taps); all exact banks
VR_CASE = B                                                              # variable rate: P = 128

ENVS = {
    "default": {},
    "lane": {"HIPSOXR_NO_CHAIN": "1", "HIPSOXR_NO_GATHER_WAVE": "1"},
    "no32": {"HIPSOXR_DEBUG_CHAIN_NO": "32"},
    "nowords": {"HIPSOXR_NO_DONE_WORDS": "1"},
    "noring": {"HIPSOXR_NO_HOST_RING": "1"},
    "nowave_vr": {"HIPSOXR_NO_INTERP_WAVE": "1", "HIPSOXR_NO_INTERP_TILE": "1"},
}
TIMEOUT = {"default": 300, "lane": 120, "no32": 120, "nowords": 120, "noring": 120, "nowave_vr": 120}


def J(env, case, nf, kind, expect, clips=1, ch=1, layout="inter", dither=False, seed=0, loud=False, counter=False, kernel="gather"):
    return dict(env=env, case=case, nf=nf, kind=kind, expect=expect, clips=clips, ch=ch, layout=layout, dither=dither, seed=seed,
                loud=loud, counter=counter, kernel=kernel)


CHAIN8, CHAIN32 = dict(kernel="chain", mode=0, NO=8, cw=0), dict(kernel="chain", mode=0, NO=32, cw=0)
WAVE = dict(kernel="gather_wave", cw=0)
LANE0, LANE1 = dict(kernel="gather", ch_fast=0), dict(kernel="gather", ch_fast=1)
# (c) NO halved by chain_geom's LDS loop; NO, span_cap and lds as the launch log of an MI355X run showed them
G_F32 = dict(kernel="chain", mode=0, NO=4, span_cap=6484, lds=128080, cw=0)
G_F64 = dict(kernel="chain", mode=0, NO=2, span_cap=6432, lds=153536, cw=0)
H_F32 = dict(kernel="chain", mode=0, NO=2, span_cap=12856, lds=153504, cw=0)

JOBS = {
    # (a) k_chain mode 0, NO = 8: 1, 8, 9 outputs and 512, the last length of NO = 8; every type; layouts; clips
    "a_1": J("default", A, 1, "f32", CHAIN8),
    "a_8": J("default", A, 8, "f32", CHAIN8),
    "a_9": J("default", A, 9, "f32", CHAIN8),
    "a_512": J("default", A, 512, "f32", CHAIN8),
    "a_9_i16": J("default", A, 9, "i16", CHAIN8, dither=True, seed=3),
    "a_512_3ch_i16": J("default", A, 512, "i16", CHAIN8, ch=3, dither=True, seed=3),
    "a_100_f64": J("default", A, 100, "f64", CHAIN8),
    "a_100_i32_loud": J("default", A, 100, "i32", CHAIN8, loud=True, counter=True),
    "a_100_3ch_planar": J("default", A, 100, "f32", CHAIN8, ch=3, layout="planar"),
    "a_100_3ch_view": J("default", A, 100, "f32", CHAIN8, ch=3, layout="view"),
    "a_100_3clips": J("default", A, 100, "f32", CHAIN8, clips=3, ch=2),
    "a_D_f32": J("default", D, 100, "f32", CHAIN8),
    "a_D_f64": J("default", D, 100, "f64", CHAIN8),
    "a_E_f32": J("default", E, 100, "f32", CHAIN8),
    "a_E_f64": J("default", E, 100, "f64", CHAIN8),
    "a_F_512": J("default", F, 512, "f32", CHAIN8),
    # (b) NO = 32: the first and the last length; plan F: a staged span beyond 1024 samples
    "b_513": J("default", A, 513, "f32", CHAIN32),
    "b_4095": J("default", A, 4095, "f32", CHAIN32),
    "b_F_513": J("default", F, 513, "f32", CHAIN32),
    "b_F_512_no32": J("no32", F, 512, "f32", CHAIN32),
    # (c) NO reduced by LDS; two channels once, so that blockIdx.y and a short NO meet
    "c_G_300_f32": J("default", G, 300, "f32", G_F32),
    "c_G_300_f64_2ch": J("default", G, 300, "f64", G_F64, ch=2),
    "c_G_300_i32": J("default", G, 300, "i32", G_F64),
    "c_G_600_f32": J("default", G, 600, "f32", G_F32),
    "c_H_100_f32": J("default", H, 100, "f32", H_F32),
    # (d) k_gather_wave: last workgroups of 32, 1 and 31 outputs in all four types; the other plans
    **{"d_%d_%s" % (nf, kind): J("default", A, nf, kind, WAVE, dither=kind == "i16", seed=5 if kind == "i16" else 0)
       for nf in (4096, 4097, 4127) for kind in DTYPE},
    "d_B_f32": J("default", B, 4100, "f32", WAVE),
    "d_B_f64": J("default", B, 4100, "f64", WAVE),
    "d_C_f32": J("default", C, 4100, "f32", WAVE),
    "d_C_f64": J("default", C, 4100, "f64", WAVE),
    "d_D_f32": J("default", D, 4100, "f32", WAVE),
    "d_D_f64": J("default", D, 4100, "f64", WAVE),
    "d_C_3ch_i16": J("default", C, 4100, "i16", WAVE, ch=3, dither=True, seed=5),
    "d_C_3ch_i16_planar": J("default", C, 4100, "i16", WAVE, ch=3, layout="planar", dither=True, seed=5),
    "d_G_f32": J("default", G, 4100, "f32", WAVE),
    "d_G_f64": J("default", G, 4100, "f64", WAVE),
    "d_H_f32": J("default", H, 4100, "f32", WAVE),
    # (e) k_gather: T < 32 at 4096 outputs and more; the fall-through of both LDS forms; by switch
    "e_E_mono": J("default", E, 4100, "f32", LANE0),
    "e_E_3ch": J("default", E, 4100, "f32", LANE1, ch=3),
    "e_E_3ch_planar": J("default", E, 4100, "f32", LANE0, ch=3, layout="planar"),
    "e_H_100_f64": J("default", H, 100, "f64", LANE0),
    "e_H_4100_f64": J("default", H, 4100, "f64", LANE0),
    "e_lane_9": J("lane", A, 9, "f32", LANE0),
    "e_lane_512": J("lane", A, 512, "f32", LANE0),
    "e_lane_4097": J("lane", A, 4097, "f32", LANE0),
    "e_lane_4097_i16": J("lane", A, 4097, "i16", LANE0, dither=True, seed=5),
    "e_lane_4097_i32": J("lane", A, 4097, "i32", LANE0),
    # (f) one wide job, [40, 65536] interleaved int16 under KERNEL_EXACT: folded over channel ranges (test_wide_job_is_folded)
    "f_wide_i16": J("default", D, None, "i16", dict(kernel="chain", mode=0, NO=8), ch=65536, dither=True, seed=11, kernel="exact"),
}
WIDE_FRAMES = 40

# (g) host ResampleStream on plan B: name -> (environment, channels, type, chunks); the probe adds the flush
SMALL, LARGE = [441, 441, 7, 0, 4410, 441], [20000, 20000, 20000]
HOST = {"g_%s_%dch_%s" % (env, ch, kind): (env, ch, kind, SMALL) for env in ("default", "nowords", "noring") for ch in (1, 2) for kind in ("f32", "i16")}
HOST.update({"g_large_%dch_%s" % (ch, kind): ("default", ch, kind, LARGE) for ch in (1, 2) for kind in ("f32", "i16")})

# (h) TensorStream (k_chain_multi): name -> (case, channels, type, chunks [frames, None, how]).  A first chunk shorter than T/2
# emits nothing yet is appended; a chunk of fewer frames than T behind a longer one: its staged spans straddle the chunk / ring
# seam; equal chunks until the ring moves; one call directly behind the move; the last call ends the stream.
TS = {
    "h_A_f32": (A, 1, "f32", [[100, None, "once"], [441, None, "once"], [200, None, "once"], [441, None, "until_move"], [441, None, "once"], [300, None, "last"]]),
    "h_A_i16": (A, 2, "i16", [[100, None, "once"], [441, None, "once"], [200, None, "once"], [441, None, "until_move"], [441, None, "once"], [300, None, "last"]]),
    "h_F_f32": (F, 1, "f32", [[300, None, "once"], [1470, None, "once"], [500, None, "once"], [1470, None, "until_move"], [1470, None, "once"], [700, None, "last"]]),
    "h_F_i16": (F, 2, "i16", [[300, None, "once"], [1470, None, "once"], [500, None, "once"], [1470, None, "until_move"], [1470, None, "once"], [700, None, "last"]]),
}
MAX_MOVE = 24   # the ring of a device stream holds its history plus sixteen small chunks (at least 1024 frames) at the most

# (i) TensorStreamGroup: five streams on plan A, stereo int16, distinct seeds, de-phased by prefixes fed alone
GROUP = dict(case=A, ch=2, kind="i16", seeds=[11, 12, 13, 14, 15], prefix=[0, 53, 106, 159, 212], calls=6, frames=441, flush=2)

# (j) variable rate on 44100 -> 16000 VHQ: name -> (environment, channels, type, chunks [frames, change after it, how], the form).
# The first chunk runs at the creation ratio, the largest the stream admits (chain_geom sizes the span from it); the second
# inside a slew; the last after a jump.
VR = {
    "j_chain_f32": ("default", 1, "f32", [[441, (44100, 20000, 400), "once"], [441, None, "once"], [441, (44100, 17000, 0), "once"], [441, None, "once"]],
                    dict(kernel="chain", mode=2, NO=8)),
    "j_chain_i16": ("default", 2, "i16", [[441, (44100, 20000, 400), "once"], [441, None, "once"], [441, (44100, 17000, 0), "once"], [441, None, "once"]],
                    dict(kernel="chain", mode=2, NO=8)),
    "j_wave_f32": ("default", 1, "f32", [[4410, (44100, 20000, 4000), "once"], [4410, None, "once"], [4410, (44100, 17000, 0), "once"], [4410, None, "once"]],
                   dict(kernel="interp_wave")),
    "j_wave_i16": ("default", 2, "i16", [[4410, (44100, 20000, 4000), "once"], [4410, None, "once"], [4410, (44100, 17000, 0), "once"], [4410, None, "once"]],
                   dict(kernel="interp_wave")),
    "j_lane_f32": ("nowave_vr", 1, "f32", [[20000, (44100, 20000, 20000), "once"], [20000, (44100, 17000, 0), "once"], [20000, None, "once"]], dict(kernel="interp")),
    "j_lane_i16": ("nowave_vr", 2, "i16", [[20000, (44100, 20000, 20000), "once"], [20000, (44100, 17000, 0), "once"], [20000, None, "once"]], dict(kernel="interp")),
}


def _wide_columns(job):
    """the columns of a wide job that are compared: both ends and both sides of column 65535, in every clip"""
    ch = job["ch"]
    return [(b, c) for b in range(job["clips"]) for c in sorted({0, 1, ch // 2 - 1, ch - 2, ch - 1})]


@functools.lru_cache(maxsize=None)
def _plan(case):
    from soxr_amd import device as dev
    return dev.Plan(*case)


def _in_len(plan, n_out):
    """an input length whose output length is n_out"""
    n = n_out * plan.M // plan.L
    while plan.out_len(n) < n_out:
        n += 1
    while plan.out_len(n) > n_out:
        n -= 1
    assert plan.out_len(n) == n_out
    return n


@functools.lru_cache(maxsize=None)
def _structured(n):
    """two tones and a staircase (steps at 3, 150, 2000, 30011, 70001): a discontinuity inside a staged span"""
    t = np.arange(n, dtype=np.float64)
    x = 0.4 * np.sin(2 * np.pi * 997.0 / 48000 * t) + 0.3 * np.sin(2 * np.pi * 12345.6 / 48000 * t + 0.5)
    for at in (3, 150, 2000, 30011, 70001):
        x[at:] += 0.04
    x.setflags(write=False)
    return x


def _signal(rng, kind, clips, frames, ch, loud=False):
    """[clips, frames, ch]: column 0 the structured signal, the others noise, scaled to the type"""
    scale = SCALE[kind] * (LOUD[kind] if loud else 1.0)   # (loud: peaks of 0.74 x 16 x 2^28, beyond int32: the input saturates, the output overshoots it)
    x = rng.standard_normal((clips, frames, ch)) * 0.25
    x[0, :, 0] = _structured(1 << 18)[:frames]
    x = x * scale
    if kind in SENT:
        lim = np.iinfo(DTYPE[kind])
        x = np.clip(np.rint(x), lim.min, lim.max)
    return x.astype(DTYPE[kind])


def _frames(job):
    return WIDE_FRAMES if job["nf"] is None else _in_len(_plan(job["case"]), job["nf"])


def _ts_frames(chunks):
    return sum(n * (MAX_MOVE if how == "until_move" else 1) for n, _, how in chunks)


@functools.lru_cache(maxsize=None)
def _inputs():
    """name -> x for every job ([clips, frames, channels]), stream ([frames, channels]) and the group ([streams, frames, channels]), seeded"""
    rng = np.random.default_rng(7171)
    out = {}
    for name, job in JOBS.items():
        out[name] = _signal(rng, job["kind"], job["clips"], _frames(job), job["ch"], job["loud"])
    for name, (env, ch, kind, chunks) in HOST.items():   # (one signal per script, channel count and type: the same in every environment)
        out[name] = out[name.replace("_" + env + "_", "_default_")] if env != "default" else _signal(rng, kind, 1, sum(chunks), ch)[0]
    for name, (_, ch, kind, chunks) in TS.items():
        out[name] = _signal(rng, kind, 1, _ts_frames(chunks), ch)[0]
    for name, (_, ch, kind, chunks, _) in VR.items():
        out[name] = _signal(rng, kind, 1, _ts_frames(chunks), ch)[0]
    g = GROUP
    out["i_group"] = _signal(rng, g["kind"], len(g["prefix"]), max(g["prefix"]) + g["calls"] * g["frames"], g["ch"])
    return out


_ABNORMAL = ""


@functools.lru_cache(maxsize=None)
def _results(env):
    """The probe's results for one environment: one child process."""
    import tempfile
    assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
    tmp = tempfile.mkdtemp(prefix="gather_forms_" + env + "_")
    x, meta, arrays = _inputs(), [], {}

    def add(name, entry):
        meta.append(dict(entry, name=name))
        arrays["x_" + name] = x[name]

    # (a new stream takes a finished one's ring from the process's pool, whatever its capacity: the streams that wait for a ring to
    #  fill run first, in front of the host streams whose 20 000-frame chunks leave rings of 2^17 frames behind)
    if env == "default":
        for name, (case, _, _, chunks) in TS.items():
            add(name, dict(stream=dict(case=list(case), vr=False, dither=True, seed=21), chunks=chunks, max_move=MAX_MOVE))
        add("i_group", dict(group=dict(GROUP, case=list(GROUP["case"]))))
    for name, job in JOBS.items():
        if job["env"] == env:
            add(name, dict(case=list(job["case"]), kernel=job["kernel"], layout=job["layout"], dither=job["dither"], seed=job["seed"], counter=job["counter"]))
    for name, (senv, _, _, chunks) in HOST.items():
        if senv == env:
            add(name, dict(host=dict(case=list(B), seed=0), chunks=chunks))
    for name, (senv, _, _, chunks, _) in VR.items():
        if senv == env:
            add(name, dict(stream=dict(case=list(VR_CASE), vr=True, dither=True, seed=0), chunks=chunks, max_move=0))
    jobs_npz, res_npz = os.path.join(tmp, "jobs.npz"), os.path.join(tmp, "results.npz")
    np.savez(jobs_npz, meta=np.array(json.dumps(meta)), **arrays)
    child_env = {key: v for key, v in os.environ.items() if not key.startswith("HIPSOXR_")}
    child_env.update(ENVS[env])
    child_env.update({"HIPSOXR_LIBRARY": DBG_LIB, "HIPSOXR_DEBUG_LAUNCH_LOG": os.path.join(tmp, "launch.log")})
    global _ABNORMAL
    assert not _ABNORMAL, "nothing more is started on the GPU: " + _ABNORMAL
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "_gather_forms_probe.py"), jobs_npz, res_npz], env=child_env, capture_output=True,
                           text=True, timeout=TIMEOUT[env])
    except subprocess.TimeoutExpired:
        _ABNORMAL = "the child of environment %r ran into its time limit" % env
        raise
    if r.returncode != 0:  # (a child that faulted, aborted or raised: the other environments' children are not started after it)
        _ABNORMAL = "the child of environment %r ended with status %d" % (env, r.returncode)
    assert r.returncode == 0, r.stderr[-2000:]
    res = dict(np.load(res_npz))
    for f in (jobs_npz, res_npz, os.path.join(tmp, "launch.log")):
        os.remove(f)
    os.rmdir(tmp)
    return res


def _parse(line):
    """one launch line -> {field: value}; grid=XxYxZ becomes gx, gy, gz"""
    f = dict(tok.split("=", 1) for tok in line.split())
    out = {k: (v if k in ("kernel", "io") else int(v)) for k, v in f.items() if k != "grid"}
    out["gx"], out["gy"], out["gz"] = (int(v) for v in f["grid"].split("x"))
    return out


def _lines(res, key):
    return [ln for ln in str(res["log_" + key]).splitlines() if ln.strip()]


def _oracle_column(oracle, case, kind, x, channel, dither, seed):
    """-> (the column's expected outputs over the whole signal x, its clip count)"""
    real = np.float32 if WIDTH[kind] == 4 else np.float64
    v = oracle.resample_channel(oracle.plan(*case), x.astype(real), "port_f32" if WIDTH[kind] == 4 else "port_f64")
    if kind in SENT:
        return oracle.quantize(v, DTYPE[kind], channel=channel, k0=0, dither=dither, seed=seed)
    return v, 0


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, "%s: %d outputs differ from the oracle, the first at %d" % (what, bad.size, bad[0])


def _check_common(f, case, kind, cols):
    plan = _plan(case)
    assert (f["width"], f["io"]) == (WIDTH[kind], kind), f
    assert (f["L"], f["M"], f["T"], f["P"]) == (plan.L, plan.M, plan.taps, 0), f
    if f["kernel"] == "chain":
        assert f["block"] == 256 and f["gx"] == -(-f["nf"] // f["NO"]) and f["gy"] == cols and f["lds"] <= 150 * 1024, f
    elif f["kernel"] == "gather_wave":
        assert f["block"] == 256 and f["gx"] == -(-f["nf"] // 32) and f["gy"] == cols and f["lds"] <= 64 * 1024 and f["span_cap"] >= plan.taps + 31 * plan.M // plan.L, f


def _check_launch(log, job, name):
    """the common fields of a job's one launch line, then the form the case names"""
    assert log and log.count("\n") == 0, "one launch per job: %r" % log
    f = _parse(log)
    plan, cols = _plan(job["case"]), job["clips"] * job["ch"]
    _check_common(f, job["case"], job["kind"], cols)
    assert (f["vr"], f["done"], f["k0"], f["in_abs0"], f["cols"]) == (0, 0, 0, 0, cols), f
    assert f["nf"] == (plan.out_len(WIDE_FRAMES) if job["nf"] is None else job["nf"]), f
    assert {k: f.get(k) for k in job["expect"]} == job["expect"], (name, f)
    if f["kernel"] == "gather":
        assert f["block"] == 256 and f["lds"] == 0
        assert (f["gx"], f["gy"]) == ((-(-f["nf"] * job["ch"] // 256), job["clips"]) if f["ch_fast"] else (-(-f["nf"] // 256), cols)), f
    return f


def _payload(name, job, res):
    """guards checked -> the payload [clips, n_out, channels]"""
    x = _inputs()[name]
    clips, frames, ch = x.shape
    n_out = _plan(job["case"]).out_len(frames)
    buf = res["y_" + name]
    side = 1 if job["layout"] == "view" else 0
    assert buf.shape == (clips, n_out + 2 * GUARD, ch + 2 * side) and buf.dtype == x.dtype
    assert np.all(buf[:, :GUARD] == POISON) and np.all(buf[:, -GUARD:] == POISON), "guard frames were written"
    if side:
        assert np.all(buf[:, :, 0] == POISON) and np.all(buf[:, :, -1] == POISON), "the channels beside the view were written"
    y = buf[:, GUARD:-GUARD, side:side + ch]
    if job["kind"] in SENT:
        assert not np.any(y == SENT[job["kind"]]), "a payload element was not written"   # (no case's oracle result holds the sentinel: asserted with the parity)
    else:
        assert not np.isnan(y).any(), "a payload element was not written"
    return y


@pytest.mark.parametrize("case", list(PLAN_SHAPE))
def test_plans_are_exact_banks(case):
    plan = _plan(case)
    assert (plan.L, plan.M, plan.taps) == PLAN_SHAPE[case] and plan.phases == 0
    vr = _plan(VR_CASE + (True,))
    assert (vr.taps, vr.phases) == (736, 128)


@pytest.mark.parametrize("name", [n for n in JOBS if n != "f_wide_i16"])
def test_form_guards_and_parity(oracle, name):
    job = JOBS[name]
    res = _results(job["env"])
    log = str(res["log_" + name])
    print(name, "launch:", log)
    _check_launch(log, job, name)
    _job_parity(oracle, name, job, res)


def _job_parity(oracle, name, job, res):
    y = _payload(name, job, res)
    x = _inputs()[name]
    total_clips = 0
    columns = _wide_columns(job) if job["nf"] is None else [(b, c) for b in range(job["clips"]) for c in range(job["ch"])]
    for b, c in columns:
        want, n_clipped = _oracle_column(oracle, job["case"], job["kind"], x[b, :, c], c, job["dither"], job["seed"])
        total_clips += n_clipped
        if job["kind"] in SENT:
            assert not np.any(want == SENT[job["kind"]]), "the sentinel is a value of this case: choose another"
        _same(y[b, :, c], want, "%s clip %d channel %d" % (name, b, c))
    if job["counter"]:
        print(name, "clip counter:", int(res["clips_" + name]), "oracle:", total_clips)
        assert int(res["clips_" + name]) == total_clips
        assert (total_clips > 0) == job["loud"]


def test_wide_job_is_folded(oracle):
    """(f) [40, 65536] interleaved int16 with dither on plan D under KERNEL_EXACT: launch_job folds it over channel ranges — two
    launches, of 65535 columns and of one — and the second launch's dither channel is the column's own index (t_ch_base): the
    columns at both ends and either side of 65535 against the oracle."""
    name = "f_wide_i16"
    job, res = JOBS[name], _results("default")
    lines = _lines(res, name)
    print(name, "launches:", " | ".join(lines))
    assert len(lines) == 2, lines
    f = [_parse(ln) for ln in lines]
    assert [g["cols"] for g in f] == [65535, 1]
    for g in f:
        _check_common(g, job["case"], job["kind"], g["cols"])
        assert {k: g.get(k) for k in job["expect"]} == job["expect"] and (g["nf"], g["k0"], g["done"]) == (_plan(D).out_len(WIDE_FRAMES), 0, 0), g
    _job_parity(oracle, name, job, res)


def test_cross_form_identity():
    """Jobs of one plan, type, dither and seed on one column: the outputs whose windows lie inside the shorter input have the
    same bits as the longest job's, whichever form served them — plan A float32 through k_chain (both geometries),
    k_gather_wave and k_gather."""
    groups = {}
    for name, job in JOBS.items():
        if (job["clips"], job["ch"], job["loud"]) == (1, 1, False) and job["nf"] is not None:
            groups.setdefault((job["case"], job["kind"], job["dither"], job["seed"]), []).append(name)
    forms = {}
    for key, names in groups.items():
        if len(names) < 2:
            continue
        plan = _plan(key[0])
        longest = max(names, key=lambda n: JOBS[n]["nf"])
        ref = _payload(longest, JOBS[longest], _results(JOBS[longest]["env"]))[0, :, 0]
        for name in names:
            job = JOBS[name]
            res = _results(job["env"])
            f = _parse(str(res["log_" + name]))
            forms.setdefault(key, set()).add((f["kernel"], f.get("NO")))
            y = _payload(name, job, res)[0, :, 0]
            assert np.array_equal(_inputs()[name][0, :, 0], _inputs()[longest][0, :_frames(job), 0])
            # output k reads input frames below floor(k M / L) + T/2 + 1
            inside = int(((_frames(job) - plan.taps // 2 - 2) * plan.L) // plan.M)
            n = max(0, min(len(y), inside))
            assert n >= len(y) - (plan.taps // 2 + 2) * plan.L // plan.M - 2
            assert np.array_equal(_bits(y[:n]), _bits(ref[:n])), name
    assert forms[(A, "f32", False, 0)] == {("chain", 8), ("chain", 32), ("gather_wave", None), ("gather", None)}
    assert forms[(G, "f32", False, 0)] == {("chain", 4), ("gather_wave", None)}
    assert forms[(H, "f64", False, 0)] == {("gather", None)} and forms[(F, "f32", False, 0)] == {("chain", 8), ("chain", 32)}


def _model(case):
    """tests/test_gpu_stream_schedule.py's integer model of a constant-rate stream, on the plan's handle (the model asks a
    stream for its plan: a plan stands in for the stream)"""
    from soxr_amd import _native as n
    plan = _plan(case)
    shim = types.SimpleNamespace(PlanInfo=n.PlanInfo, check=n.check,
                                 lib=types.SimpleNamespace(hipsoxr_stream_plan=lambda h: h, hipsoxr_plan_info=n.lib.hipsoxr_plan_info,
                                                           hipsoxr_plan_out_len=n.lib.hipsoxr_plan_out_len))
    return Model(shim, plan.handle)


def _stream_reference(oracle, case, kind, x, dither, seed):
    """[n_out, channels]: the oracle over the whole signal x [frames, channels]"""
    return np.stack([_oracle_column(oracle, case, kind, x[:, c], c, dither, seed)[0] for c in range(x.shape[1])], axis=1)


def _as2(y, ch):
    return y.reshape(-1, ch)


def _host_stream_check(oracle, name):
    """(g) soxr_amd.ResampleStream on plan B: every call returns the model's count and the oracle's bits; the launches are
    k_chain mode 0 — NO = 8, then 32 for the 4410-frame chunk — with completion words claimed where the launch has at most 64
    workgroups and never under HIPSOXR_NO_DONE_WORDS; 20 000-frame chunks take k_gather_wave.  From the second launch on the
    job starts at a later output (k0), and once the ring has dropped frames at a later input (in_abs0).  -> the launches"""
    env, ch, kind, chunks = HOST[name]
    res, x = _results(env), _inputs()[name]
    plan = _plan(B)
    fed = [int(v) for v in res["n_" + name]]
    assert fed == chunks + [0]
    want = _stream_reference(oracle, B, kind, x, True, 0)
    model, at, launches = _model(B), 0, []
    for i, n in enumerate(fed):
        last = i == len(fed) - 1
        due = model.call(n, BIG) + (model.call(None, BIG) if last else 0)
        y = _as2(res["y_%s_%d" % (name, i)], ch)
        lines = _lines(res, "%s_%d" % (name, i))
        print(name, "call", i, "(%d frames in, %d out):" % (n, len(y)), " | ".join(lines))
        assert len(y) == due, "call %d: %d frames returned, %d due" % (i, len(y), due)
        _same(y, want[at:at + due], "%s call %d" % (name, i))
        assert len(lines) == (1 if due else 0) or last
        k = at
        for ln in lines:
            f = _parse(ln)
            _check_common(f, B, kind, ch)
            assert (f["vr"], f["done"], f["k0"], f["cols"]) == (0, 0, k, ch), f
            # the ring holds the frames the launch's first output needs: floor(k M / L) - (T/2 - 1) and later ones
            assert 0 <= f["in_abs0"] <= max(0, k * plan.M // plan.L - (plan.taps // 2 - 1)), f
            if chunks == LARGE and not last:
                assert f["kernel"] == "gather_wave", f
            else:
                assert (f["kernel"], f["mode"], f["NO"]) == ("chain", 0, 8 if f["nf"] <= 512 else 32), f
            assert f["cw"] == (1 if env != "nowords" and f["gx"] * f["gy"] <= 64 else 0), f
            k += f["nf"]
            launches.append(f)
        assert k == at + due
        at += due
    assert at == len(want) == model.handed
    assert [f["k0"] > 0 for f in launches] == [False] + [True] * (len(launches) - 1)
    if chunks == SMALL:
        assert {f["NO"] for f in launches} == {8, 32} and (env == "nowords") == (not any(f["cw"] for f in launches))
    return launches


@pytest.mark.parametrize("name", list(HOST))
def test_host_stream(oracle, name):
    _host_stream_check(oracle, name)


def test_host_stream_reads_a_ring_that_dropped_frames(oracle):
    """(g) in_abs0: a ring drops frames when the next chunk does not fit, and a stream may inherit a larger ring from the pool —
    so not every stream's launches start at a later input frame, but the first stream of each process does, from its 4410-frame
    chunk on."""
    for env in ("default", "nowords", "noring"):
        launches = _host_stream_check(oracle, "g_%s_1ch_f32" % env)
        assert [f["in_abs0"] > 0 for f in launches] == [False, False, False, True, True, True], env


@pytest.mark.parametrize("ch,kind", [(1, "f32"), (2, "f32"), (1, "i16"), (2, "i16")])
def test_host_stream_switches_change_no_bit(ch, kind):
    """(g) the same signal and script without a switch, under HIPSOXR_NO_DONE_WORDS and under HIPSOXR_NO_HOST_RING: the same
    bits, call by call."""
    base = "g_default_%dch_%s" % (ch, kind)
    for env in ("nowords", "noring"):
        name = "g_%s_%dch_%s" % (env, ch, kind)
        assert np.array_equal(_inputs()[name], _inputs()[base])
        for i in range(len(SMALL) + 1):
            a, b = _results("default")["y_%s_%d" % (base, i)], _results(env)["y_%s_%d" % (name, i)]
            assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (env, i)


@pytest.mark.parametrize("name", list(TS))
def test_tensor_stream(oracle, name):
    """(h) device.TensorStream: every call is ONE launch of k_chain_multi (items=1) — the first emits nothing yet appends its
    chunk (empty=1), a short chunk behind a longer one has its spans across the chunk / ring seam, equal chunks until the ring
    moves (moving=1), one call directly behind the move — then the flush on k_chain.  Counts by the model, bits by the oracle."""
    case, ch, kind, chunks = TS[name]
    res, x = _results("default"), _inputs()[name]
    plan = _plan(case)
    fed = [int(v) for v in res["n_" + name]]
    n_move = len(fed) - (len(chunks) - 1)
    assert 1 <= n_move <= MAX_MOVE
    expect_fed = [c[0] for c in chunks[:3]] + [chunks[3][0]] * n_move + [c[0] for c in chunks[4:]]
    assert fed == expect_fed
    assert fed[0] < plan.taps // 2 and fed[2] < plan.taps < fed[1]
    x = x[:sum(fed)]
    want = _stream_reference(oracle, case, kind, x, True, 21)
    model, at = _model(case), 0
    for i, n in enumerate(fed):
        last = i == len(fed) - 1
        first = model.call(n, BIG)                              # what the chunk makes due: the k_chain_multi launch's
        due = first + (model.call(None, BIG) if last else 0)    # ... and what the end of input adds
        y = _as2(res["y_%s_%d" % (name, i)], ch)
        lines = _lines(res, "%s_%d" % (name, i))
        print(name, "call", i, "(%d frames in, %d out):" % (n, len(y)), " | ".join(lines))
        assert len(y) == due, "call %d: %d frames returned, %d due" % (i, len(y), due)
        _same(y, want[at:at + due], "%s call %d" % (name, i))
        f = _parse(lines[0])
        assert (f["kernel"], f["width"], f["io"], f["L"], f["M"], f["T"], f["P"]) == ("chain_multi", WIDTH[kind], kind, plan.L, plan.M, plan.taps, 0), f
        assert (f["items"], f["nch"], f["mode"], f["block"], f["NO"], f["gy"]) == (1, ch, 0, 256, 8, ch) and f["lds"] <= 150 * 1024, f
        assert f["max_out"] == first and f["gx"] == max(1, -(-first // 8)) and f["empty"] == (1 if first == 0 else 0), f
        assert f["moving"] == (1 if i == 3 + n_move - 1 else 0), (i, f)
        if i == 0:
            assert (first, due) == (0, 0) and len(lines) == 1
        if not last:
            assert len(lines) == 1
        else:  # the flush: what the end of input adds, on k_chain from the stream's output count on
            k = at + first
            assert len(lines) >= 2
            for ln in lines[1:]:
                g = _parse(ln)
                _check_common(g, case, kind, ch)
                assert (g["kernel"], g["mode"], g["k0"], g["cols"]) == ("chain", 0, k, ch) and g["in_abs0"] > 0, g
                k += g["nf"]
            assert k == at + due
        at += due
    assert at == len(want) == plan.out_len(len(x))


def test_tensor_stream_group(oracle):
    """(i) device.TensorStreamGroup: five stereo int16 streams with seeds of their own, de-phased by prefixes fed alone; six
    group calls are six launches of k_chain_multi with items=5; one member is ended alone.  Every stream against the oracle on
    its OWN signal."""
    g, res, x = GROUP, _results("default"), _inputs()["i_group"]
    n, ch, kind, frames = len(g["prefix"]), g["ch"], g["kind"], g["frames"]
    models, at = [_model(g["case"]) for _ in range(n)], [0] * n
    wants = []
    for i, pre in enumerate(g["prefix"]):
        total = pre + g["calls"] * frames
        wants.append(_stream_reference(oracle, g["case"], kind, x[i, :total], True, g["seeds"][i]))
        if pre:
            due = models[i].call(pre, BIG)
            y = _as2(res["y_i_group_pre%d" % i], ch)
            lines = _lines(res, "i_group_pre%d" % i)
            print("i_group stream", i, "prefix:", " | ".join(lines))
            f = _parse(lines[0])
            assert len(lines) == 1 and (f["kernel"], f["items"], f["max_out"], f["empty"]) == ("chain_multi", 1, due, 1 if due == 0 else 0), f
            assert len(y) == due
            _same(y, wants[i][:due], "stream %d prefix" % i)
            at[i] = due
    assert [a > 0 for a in at] == [False, False, False, True, True]
    for c in range(g["calls"]):
        lines = _lines(res, "i_group_%d" % c)
        print("i_group call", c, ":", " | ".join(lines))
        f = _parse(lines[0])
        y, counts = res["y_i_group_%d" % c], res["counts_i_group_%d" % c]
        dues = [models[i].call(frames, BIG) for i in range(n)]
        assert [int(v) for v in counts] == dues
        assert len(lines) == 1 and (f["kernel"], f["io"], f["items"], f["nch"], f["gy"], f["max_out"]) == ("chain_multi", kind, n, ch, n * ch, max(dues)), f
        assert 0 <= f["moving"] <= n   # (whose rings are full depends on the rings the pool handed out)
        assert f["empty"] == sum(d == 0 for d in dues) and f["NO"] == 8 and f["gx"] == -(-max(dues) // 8)
        for i in range(n):
            _same(_as2(y[i], ch)[:dues[i]], wants[i][at[i]:at[i] + dues[i]], "stream %d call %d" % (i, c))
            at[i] += dues[i]
    assert len(set(at)) > 1, "the streams are at different outputs"
    i = g["flush"]
    due = models[i].call(0, BIG) + models[i].call(None, BIG)
    y = _as2(res["y_i_group_flush"], ch)
    lines = _lines(res, "i_group_flush")
    print("i_group flush of stream", i, ":", " | ".join(lines))
    assert len(y) == due and len(lines) >= 1 and all(_parse(ln)["kernel"] == "chain" for ln in lines) and _parse(lines[0])["k0"] == at[i]
    _same(y, wants[i][at[i]:at[i] + due], "stream %d flush" % i)
    assert at[i] + due == len(wants[i])


@pytest.mark.parametrize("name", list(VR))
def test_variable_rate_below_the_tile(oracle, name):
    """(j) device.TensorStream(vr=True) on 44100 -> 16000 VHQ against tests/vr_sim.py, every chunk bit for bit: k_chain mode 2
    at 441-frame chunks, k_interp_wave at 4410-frame chunks, k_interp under the switches at 20 000-frame chunks — the first
    chunk at the creation ratio, one inside a slew, one after a jump."""
    env, ch, kind, chunks, expect = VR[name]
    res, x = _results(env), _inputs()[name]
    sims = [VrSim(oracle, VR_CASE[0], VR_CASE[1], VR_CASE[2], DTYPE[kind]) for _ in range(ch)]
    at, k, in_slew, after_jump = 0, 0, 0, 0
    for i, (n, change, _) in enumerate(chunks):
        lines = _lines(res, "%s_%d" % (name, i))
        print(name, "chunk", i, "launches:", " | ".join(lines))
        y = _as2(res["y_%s_%d" % (name, i)], ch)
        slewing = bool(sims[0].n_slew) and sims[0].k_done < sims[0].k_s + sims[0].n_slew
        for c in range(ch):
            want = sims[c].feed(x[at:at + n, c], last=False, channel=c)
            assert len(want) == len(y), "chunk %d: %d frames returned, %d due" % (i, len(y), len(want))
            _same(np.ascontiguousarray(y[:, c]), want, "%s chunk %d channel %d" % (name, i, c))
        assert 1 <= len(lines) <= 2   # (a call that crosses the end of a slew makes a second launch)
        for ln in lines:
            f = _parse(ln)
            assert {key: f.get(key) for key in expect} == expect, f
            assert (f["vr"], f["io"], f["width"], f["T"], f["P"], f["cols"], f["k0"]) == (1, kind, WIDTH[kind], 736, 128, ch, k), f
            k += f["nf"]
        assert k == sims[0].k_done
        in_slew += slewing and sims[0].k_done <= sims[0].k_s + sims[0].n_slew and len(lines) == 1
        after_jump += i > 0 and chunks[i - 1][1] is not None and chunks[i - 1][1][2] == 0
        at += n
        if change:
            for s in sims:
                s.set_io_ratio(change[0] / change[1], change[2])
    assert in_slew >= 1 and after_jump >= 1, "one chunk inside a slew and one after a jump"


def test_every_form_ran():
    """Every form of sections (a) to (j) appears in some launch line: (kernel, I/O type, mode or variable rate)."""
    seen = set()
    for env in ENVS:
        for key, v in _results(env).items():
            if key.startswith("log_"):
                for line in str(v).splitlines():
                    if line.strip():
                        f = _parse(line)
                        seen.add((f["kernel"], f["io"], f.get("mode", f.get("vr"))))
    for want in [("chain", io, 0) for io in DTYPE] + [("gather_wave", io, 0) for io in DTYPE] + [("gather", io, 0) for io in DTYPE] \
            + [("chain_multi", io, 0) for io in ("f32", "i16")] \
            + [(kernel, io, m) for io in ("f32", "i16") for kernel, m in (("chain", 2), ("interp_wave", 1), ("interp", 1))]:
        assert want in seen, want
