"""GPU: every launch form of the interpolated-phase forward kernels (csrc/kernels.hip, launch_gather) against the oracle.

launch_gather decides, per launch of an interpolated-phase plan: k_chain (mode 1; variable rate: 2) for fewer than 4096
outputs — above 512 only where k_interp_wave cannot take them; k_interp_wave; k_interp_tile where the cost model of
interp_tile_form puts it ahead — one output per lane (pair=0), neighbouring channels of an even channel count (pair=1) or
the column's two halves h periods of L outputs apart (pair=2), float pairs with the span staged twice (twin=1); and
lane-per-output k_interp where neither fits.  The debug-switch build writes one line per launch (HIPSOXR_DEBUG_LAUNCH_LOG),
so a case here names the form its launch must show and the test reads it from the log — the rules are not restated.  One
child process per environment (tests/_interp_forms_probe.py: the default one and four switch sets) runs that environment's
jobs into guarded, NaN- / sentinel-filled buffers; everything is compared here.

Per job: the log shows the stated form — a case is resized, never its assertion changed, if a later launch rule moves it;
8 guard frames either side of every clip untouched and every payload element written; the whole payload equal to the oracle
bit for bit (oracle.resample_channel in the canonical order of the type's engine over the whole signal, then
oracle.quantize for integers: dither keyed by (seed, channel, output index)).  Column 0 of every job is a prefix of ONE
structured signal — two tones and a staircase, scaled to the type — every other column is noise of its own: jobs of one
plan and type see the same input, so whatever form served them, the outputs whose windows lie inside the shorter input
have the same bits (test_cross_form_identity).

The sizes come from interp_tile_form's constants and were pinned from the launch log on an MI355X:
  * 48000 -> 44101 HQ (T 216, P 32) in workgroups of KO = 26 x 32 = 832 outputs: one workgroup costs the model
    832 x 216 x 6.3e-5 us = 11.32 us, k_interp_wave 216e-6 us per output, so the tile form starts at 52 417 outputs of a mono
    column (C_FIRST); 64 KO = 53 248 is the length around which the last workgroup has 1, 832 and 831 outputs;
  * halves: h = ceil(nf / 2L), n1 = h L, taken iff n1 < nf and 10 (nf - n1) >= 7 n1: h = 1 from 74 972 to 88 202 outputs
    (m2_n = n1 there), neither at 74 971 nor at 88 203; without a switch from 335 873 outputs (h = 4), where pairing saves
    a layer of 256 workgroups;
  * variable rate (44100 -> 16000 VHQ, T 736, P 128): a workgroup costs the model KO x 736 x 2.9e-4 us (x 1.4 twin, x 1.7
    pair), lane-per-output k_interp 2.5e-6 x 736 us per output and column.  A 96 000-frame chunk of 4 channels (34 830
    outputs) stays on k_interp under HIPSOXR_NO_INTERP_WAVE — 256 us against 880 us for one layer of twin workgroups of
    2816 outputs — so the chunks here are the smallest that reach the tile form under the switches: 114 330 outputs (4
    channels, twin), 164 071 (4 channels, one copy), 128 683 (3 channels).  In the default environment, against
    k_interp_wave's 1e-6 x 736 us, the form starts at 335 873 outputs of 4 channels (a chunk of 925 750 frames: 119
    workgroups of 2816 outputs a column pair, 238 in one layer); 3 channels never reach it: one output per lane costs a
    layer of 3328 x 736 x 2.9e-4 us = 710 us per 256 workgroups, the wave kernel 628 us for the same outputs."""
import functools
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
GUARD, POISON = 8, 12345
SENT = {"i16": -12345, "i32": -123456789}
DTYPE = {"f32": np.float32, "f64": np.float64, "i16": np.int16, "i32": np.int32}
WIDTH = {"f32": 4, "f64": 8, "i16": 4, "i32": 8}            # the engine's precision
SCALE = {"f32": 1.0, "f64": 1.0, "i16": 8000.0, "i32": 2.0 ** 28}

MAIN = (48000, 44101, "HQ")        # T 216, P 32; L = 44101 puts the halves seam at output 44101
VHQ = (48000, 44101, "VHQ")        # P 128
QQ = (600011, 700001, "QQ")        # P 256 (the cap of the first-wave scan in k_interp_tile), T 8: k_interp_wave has one step
LONG = (95999, 8001, "HQ")         # 12 input samples per output: the span sizing
VR_CASE = (44100, 16000, "VHQ")
PLAN_SHAPE = {MAIN: (216, 32), VHQ: (296, 128), QQ: (8, 256), LONG: (2336, 32)}  # case -> (taps, phases)

ENVS = {
    "default": {},
    "pair": {"HIPSOXR_DEBUG_INTERP_PAIR_ALWAYS": "1", "HIPSOXR_NO_CHAIN": "1"},
    "nowave": {"HIPSOXR_DEBUG_INTERP_PAIR_ALWAYS": "1", "HIPSOXR_NO_INTERP_WAVE": "1"},
    "notwin": {"HIPSOXR_DEBUG_INTERP_PAIR_ALWAYS": "1", "HIPSOXR_NO_INTERP_WAVE": "1", "HIPSOXR_DEBUG_INTERP_NO_TWIN": "1"},
    "lane": {"HIPSOXR_NO_INTERP_WAVE": "1", "HIPSOXR_NO_INTERP_TILE": "1"},
}
TIMEOUT = {"default": 300, "pair": 240, "nowave": 300, "notwin": 300, "lane": 120}

KO = 832                 # 26 outputs per interval x 32 intervals: what the log shows on MAIN below two layers of workgroups
C_FIRST = 52417          # 832 x 216 x 6.3e-5 us = 216e-6 us x 52416
H1_FIRST, H1_LAST = 74972, 88202   # 10 (nf - L) >= 7 L  ...  nf <= 2 L
H_DEFAULT = 335873       # the first mono length at which pairing the halves saves a layer of workgroups (h = 4)


def J(env, case, nf, kind, expect, clips=1, ch=1, layout="inter", dither=False, seed=0, loud=False, counter=False):
    return dict(env=env, case=case, nf=nf, kind=kind, expect=expect, clips=clips, ch=ch, layout=layout, dither=dither, seed=seed,
                loud=loud, counter=counter)


CHAIN = dict(kernel="chain", mode=1, NO=8)
WAVE = dict(kernel="interp_wave")
TILE0 = dict(kernel="interp_tile", pair=0, twin=0, h=0)
PAIR_T, PAIR_1 = dict(kernel="interp_tile", pair=1, twin=1, h=0), dict(kernel="interp_tile", pair=1, twin=0, h=0)
HALF_T, HALF_1 = dict(kernel="interp_tile", pair=2, twin=1, h=1), dict(kernel="interp_tile", pair=2, twin=0, h=1)
LANE = dict(kernel="interp")

JOBS = {
    # (a) k_chain mode 1: 1, 8, 9 outputs and 512, the last length of NO = 8
    "a_1": J("default", MAIN, 1, "f32", CHAIN),
    "a_8_3ch": J("default", MAIN, 8, "f32", CHAIN, ch=3),
    "a_9_i16": J("default", MAIN, 9, "i16", CHAIN, dither=True, seed=3),
    "a_512": J("default", MAIN, 512, "f32", CHAIN),
    "a_512_3ch_i16": J("default", MAIN, 512, "i16", CHAIN, ch=3, dither=True, seed=3),
    # (b) k_interp_wave: the first length past the chain, the last below the tile rule's 4096 (no multiple of 32: the quads
    # past the end), one output without the chain, every type, three channels in both layouts
    "b_513": J("default", MAIN, 513, "f32", WAVE),
    "b_4095_f32": J("default", MAIN, 4095, "f32", WAVE),
    "b_4095_f64": J("default", MAIN, 4095, "f64", WAVE),
    "b_4095_i16": J("default", MAIN, 4095, "i16", WAVE, dither=True, seed=5),
    "b_4095_i32": J("default", MAIN, 4095, "i32", WAVE),
    "b_1000_3ch": J("default", MAIN, 1000, "f32", WAVE, ch=3),
    "b_1000_3ch_planar": J("default", MAIN, 1000, "i16", WAVE, ch=3, layout="planar", dither=True, seed=5),
    "b_1_nochain": J("pair", MAIN, 1, "f32", WAVE),
    "b_52416": J("default", MAIN, C_FIRST - 1, "f32", WAVE),     # one output short of the tile form
    # (c) k_interp_tile, one output per lane: the first length, and last workgroups of 831, 832 and 1 outputs
    "c_first_f32": J("default", MAIN, C_FIRST, "f32", dict(TILE0, KO=KO)),
    "c_first_f64": J("default", MAIN, C_FIRST, "f64", dict(TILE0, KO=KO)),
    "c_64ko_m1": J("default", MAIN, 64 * KO - 1, "f32", dict(TILE0, KO=KO, gx=64)),
    "c_64ko": J("default", MAIN, 64 * KO, "f32", dict(TILE0, KO=KO, gx=64)),
    "c_64ko_p1_f32": J("default", MAIN, 64 * KO + 1, "f32", dict(TILE0, KO=KO, gx=65)),
    "c_64ko_p1_f64": J("default", MAIN, 64 * KO + 1, "f64", dict(TILE0, KO=KO, gx=65)),
    # (d) channel pairs.  Twin (float engine), PAIR_ALWAYS: the tile form from 36 692 outputs of a stereo clip, 18 346 of
    # four channels, 12 231 of three stereo clips (1.4 x 11.32 us against 216e-6 us per output and column)
    "d_2ch": J("pair", MAIN, 37000, "f32", PAIR_T, ch=2),
    "d_4ch": J("pair", MAIN, 18500, "f32", PAIR_T, ch=4),
    "d_2ch_planar": J("pair", MAIN, 37000, "f32", PAIR_T, ch=2, layout="planar"),
    "d_3clips": J("pair", MAIN, 12500, "f32", PAIR_T, clips=3, ch=2),
    "d_view": J("pair", MAIN, 37000, "f32", PAIR_T, ch=2, layout="view"),
    "d_i16": J("pair", MAIN, 37000, "i16", PAIR_T, ch=2, dither=True, seed=7),
    "d_i16_loud": J("pair", MAIN, 37000, "i16", PAIR_T, ch=2, dither=True, seed=7, loud=True, counter=True),
    # ... float64 / int32 never twin (1.7 x 11.32 us: from 44 554 outputs)
    "d_f64": J("pair", MAIN, 45000, "f64", PAIR_1, ch=2),
    "d_i32": J("pair", MAIN, 45000, "i32", PAIR_1, ch=2, counter=True),
    # ... one copy of the span (NO_TWIN; against k_interp's 2.5e-6 us per output x tap: from 17 822 / 8911 outputs)
    "dn_2ch": J("notwin", MAIN, 18000, "f32", PAIR_1, ch=2),
    "dn_4ch": J("notwin", MAIN, 9000, "f32", PAIR_1, ch=4),
    "dn_i16": J("notwin", MAIN, 18000, "i16", PAIR_1, ch=2, dither=True, seed=7),
    "dn_planar": J("notwin", MAIN, 18000, "f32", PAIR_1, ch=2, layout="planar"),
    # (e) the column's two halves: h = 1 from 74 972 to 88 202 outputs, another form one output either side
    "e_74971": J("pair", MAIN, H1_FIRST - 1, "f32", TILE0),
    "e_first": J("pair", MAIN, H1_FIRST, "f32", dict(HALF_T, nf_t=44101, m2_n=H1_FIRST - 44101)),
    "e_last": J("pair", MAIN, H1_LAST, "f32", dict(HALF_T, nf_t=44101, m2_n=44101)),
    "e_88203": J("pair", MAIN, H1_LAST + 1, "f32", TILE0),
    "e_3ch": J("pair", MAIN, H1_FIRST, "f32", dict(HALF_T, nf_t=44101), ch=3),
    "e_i16": J("pair", MAIN, 80000, "i16", dict(HALF_T, nf_t=44101), dither=True, seed=9),
    "en_first": J("notwin", MAIN, H1_FIRST, "f32", dict(HALF_1, nf_t=44101)),
    "en_3ch_last": J("notwin", MAIN, H1_LAST, "f32", dict(HALF_1, nf_t=44101, m2_n=44101), ch=3),
    "en_i16": J("notwin", MAIN, 80000, "i16", dict(HALF_1, nf_t=44101), dither=True, seed=9),
    "en_f64": J("notwin", MAIN, H1_FIRST, "f64", dict(HALF_1, nf_t=44101)),
    "en_i32": J("notwin", MAIN, 80000, "i32", dict(HALF_1, nf_t=44101)),
    "e_default_m1": J("default", MAIN, H_DEFAULT - 1, "f32", TILE0),
    "e_default": J("default", MAIN, H_DEFAULT, "f32", dict(kernel="interp_tile", pair=2, twin=1, h=4, nf_t=4 * 44101, KO=KO)),
    # (f) lane per output: by switch, and where 65 536 columns of channel-fast data leave no other kernel
    "f_3ch_f32": J("lane", MAIN, 5000, "f32", dict(LANE, ch_fast=1), ch=3),
    "f_3ch_i32": J("lane", MAIN, 5000, "i32", dict(LANE, ch_fast=1), ch=3),
    "f_chain32": J("lane", MAIN, 4095, "f32", dict(kernel="chain", mode=1, NO=32)),   # (the chain's other geometry)
    "f_wide": J("default", MAIN, None, "f32", dict(LANE, ch_fast=1, gy=1), ch=65536),             # [40, 65536]
    "f_wide_i16": J("default", MAIN, None, "i16", dict(LANE, ch_fast=1, gy=1), ch=65536, dither=True, seed=11),
    "f_wide_3clips": J("default", MAIN, None, "f32", dict(LANE, ch_fast=1, gy=3), clips=3, ch=40000),
    # the other plans: P 128; P 256 with T 8; a step of 12 input samples per output
    "vhq_wave": J("default", VHQ, 5000, "f32", WAVE),
    "vhq_tile": J("nowave", VHQ, 60000, "f32", dict(PAIR_T, KO=26 * 128), ch=2),
    "qq_wave": J("default", QQ, 5000, "f32", WAVE),
    "qq_tile": J("nowave", QQ, 120000, "f32", dict(PAIR_T, KO=26 * 256), ch=2),
    "long_wave": J("default", LONG, 1000, "f32", WAVE),
    "long_tile": J("nowave", LONG, 21500, "f32", dict(TILE0, KO=KO)),
}
WIDE_FRAMES = 40


def _wide_columns(job):
    """the columns of a wide job that are compared: both ends and both sides of column 65535, in every clip"""
    ch = job["ch"]
    return [(b, c) for b in range(job["clips"]) for c in sorted({0, 1, ch // 2 - 1, ch - 2, ch - 1})]
SHARED = ["a_1", "a_512", "b_513", "b_4095_f32", "b_1_nochain", "b_52416", "c_first_f32", "c_64ko_m1", "c_64ko", "c_64ko_p1_f32", "f_chain32"]

# name -> (environment, channels, type, chunks [(frames, ratio change after it)], what each chunk's first launch shows)
VR_TILE = dict(kernel="interp_tile", vr=1)
STREAMS = {
    # (g) variable rate; the second chunk runs inside a slew: a step increment and a clock origin
    "g_4ch_f32": ("nowave", 4, "f32", [(330000, (44100, 20000, 400000)), (330000, None)],
                  [dict(VR_TILE, pair=1, twin=1, k0=0), dict(VR_TILE, pair=1, twin=1)]),
    "g_4ch_i16": ("notwin", 4, "i16", [(470000, None)], [dict(VR_TILE, pair=1, twin=0)]),
    "g_3ch_f32": ("nowave", 3, "f32", [(370000, None)], [dict(VR_TILE, pair=0, twin=0)]),
}
# (h) constant rate, two chunks of the halves form each: the second launch starts at a non-zero output and ring origin
# (the device ring holds four chunks of the first call's size — 2^19 frames after 95 000 — and is compacted when the next
#  chunk does not fit: the second chunk is longer than what is left of it)
H_STREAM = ("pair", [95000, 440000])


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
    """two tones and a staircase (steps at 3, 150, 2000, 30011, 70001, 250007): a discontinuity inside a staged span"""
    t = np.arange(n, dtype=np.float64)
    x = 0.4 * np.sin(2 * np.pi * 997.0 / 48000 * t) + 0.3 * np.sin(2 * np.pi * 12345.6 / 48000 * t + 0.5)
    for at in (3, 150, 2000, 30011, 70001, 250007):
        x[at:] += 0.04
    x.setflags(write=False)
    return x


def _signal(rng, kind, clips, frames, ch, loud=False):
    """[clips, frames, ch]: column 0 the structured signal, the others noise, scaled to the type"""
    scale = SCALE[kind] * (5.0 if loud else 1.0)   # (loud: peaks of 0.94 x 40 000, beyond int16)
    x = rng.standard_normal((clips, frames, ch)) * 0.25
    x[0, :, 0] = _structured(1 << 20)[:frames]
    x = x * scale
    if kind in SENT:
        lim = np.iinfo(DTYPE[kind])
        x = np.clip(np.rint(x), lim.min, lim.max)
    return x.astype(DTYPE[kind])


def _frames(job):
    return WIDE_FRAMES if job["nf"] is None else _in_len(_plan(job["case"]), job["nf"])


@functools.lru_cache(maxsize=None)
def _inputs():
    """name -> x [clips, frames, channels] for every job and stream, seeded"""
    rng = np.random.default_rng(6161)
    out = {}
    for name, job in JOBS.items():
        out[name] = _signal(rng, job["kind"], job["clips"], _frames(job), job["ch"], job["loud"])
    for name, (_, ch, kind, chunks, _) in STREAMS.items():
        out[name] = _signal(rng, kind, 1, sum(n for n, _ in chunks), ch)
    out["h_stream"] = _signal(rng, "f32", 1, sum(H_STREAM[1]), 1)
    return out


_ABNORMAL = ""


@functools.lru_cache(maxsize=None)
def _results(env):
    """The probe's results for one environment: one child process."""
    import tempfile
    assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
    tmp = tempfile.mkdtemp(prefix="interp_forms_" + env + "_")
    x, meta, arrays = _inputs(), [], {}
    for name, job in JOBS.items():
        if job["env"] == env:
            meta.append(dict(name=name, case=list(job["case"]), layout=job["layout"], dither=job["dither"], seed=job["seed"], counter=job["counter"]))
            arrays["x_" + name] = x[name]
    for name, (senv, _, kind, chunks, _) in STREAMS.items():
        if senv == env:
            meta.append(dict(name=name, stream=dict(case=list(VR_CASE), vr=True, dither=True, seed=0, flush=False), chunks=[[n, c] for n, c in chunks]))
            arrays["x_" + name] = x[name]
    if H_STREAM[0] == env:
        meta.append(dict(name="h_stream", stream=dict(case=list(MAIN), vr=False, dither=False, seed=0, flush=False), chunks=[[n, None] for n in H_STREAM[1]]))
        arrays["x_h_stream"] = x["h_stream"]
    jobs_npz, res_npz = os.path.join(tmp, "jobs.npz"), os.path.join(tmp, "results.npz")
    np.savez(jobs_npz, meta=np.array(json.dumps(meta)), **arrays)
    child_env = {key: v for key, v in os.environ.items() if not key.startswith("HIPSOXR_")}
    child_env.update(ENVS[env])
    child_env.update({"HIPSOXR_LIBRARY": DBG_LIB, "HIPSOXR_DEBUG_LAUNCH_LOG": os.path.join(tmp, "launch.log")})
    global _ABNORMAL
    assert not _ABNORMAL, "nothing more is started on the GPU: " + _ABNORMAL
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "_interp_forms_probe.py"), jobs_npz, res_npz], env=child_env, capture_output=True,
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


def _oracle_column(oracle, case, kind, x, channel, dither, seed):
    """-> (the column's expected outputs, its clip count)"""
    real = np.float32 if WIDTH[kind] == 4 else np.float64
    v = oracle.resample_channel(oracle.plan(*case), x.astype(real), "port_f32" if WIDTH[kind] == 4 else "port_f64")
    if kind in SENT:
        return oracle.quantize(v, DTYPE[kind], channel=channel, k0=0, dither=dither, seed=seed)
    return v, 0


def _bits(a):
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _check_launch(log, job, name):
    """the common fields of a job's one launch line, then the form the case names"""
    assert log and log.count("\n") == 0, "one launch per job: %r" % log
    f = _parse(log)
    kind, plan = job["kind"], _plan(job["case"])
    assert (f["width"], f["io"], f["vr"]) == (WIDTH[kind], kind, 0), f
    assert (f["L"], f["M"], f["T"], f["P"]) == (plan.L, plan.M, plan.taps, plan.phases), f
    assert (f["done"], f["k0"], f["in_abs0"], f["cols"]) == (0, 0, 0, job["clips"] * job["ch"]), f
    assert f["nf"] == (plan.out_len(WIDE_FRAMES) if job["nf"] is None else job["nf"]), f
    assert {k: f.get(k) for k in job["expect"]} == job["expect"], (name, f)
    if f["kernel"] == "interp_tile":
        assert f["block"] == 1024 and f["gx"] == -(-f["nf_t"] // f["KO"]) and f["gy"] == f["cols"] // (2 if f["pair"] == 1 else 1) and f["lds"] <= 160 * 1024
        assert f["KO"] % f["P"] == 0 and 15 <= f["KO"] // f["P"] <= 64
        if f["pair"] == 2:
            assert f["nf_t"] == f["h"] * f["L"] and f["m2_n"] == f["nf"] - f["nf_t"] and 0 < f["m2_n"] <= f["nf_t"]
        if WIDTH[kind] == 8:
            assert f["twin"] == 0, "float64 / int32 pairs never stage the span twice"
    elif f["kernel"] == "interp_wave":
        assert f["block"] == 256 and f["gx"] == -(-f["nf"] // 32) and f["gy"] == f["cols"]
    elif f["kernel"] == "chain":
        assert f["block"] == 256 and f["gx"] == -(-f["nf"] // f["NO"]) and f["gy"] == f["cols"]
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
    if job["kind"] not in SENT:
        assert not np.isnan(y).any(), "a payload element was not written"
    return y


@pytest.mark.parametrize("case", list(PLAN_SHAPE))
def test_plans_are_interpolated(case):
    plan = _plan(case)
    assert (plan.taps, plan.phases) == PLAN_SHAPE[case]
    vr = _plan(VR_CASE + (True,))
    assert (vr.taps, vr.phases) == (736, 128)


@pytest.mark.parametrize("name", list(JOBS))
def test_form_guards_and_parity(oracle, name):
    job = JOBS[name]
    res = _results(job["env"])
    log = str(res["log_" + name])
    print(name, "launch:", log)
    f = _check_launch(log, job, name)
    y = _payload(name, job, res)
    x = _inputs()[name]
    total_clips = 0
    columns = _wide_columns(job) if job["nf"] is None else [(b, c) for b in range(job["clips"]) for c in range(job["ch"])]
    for b, c in columns:
        want, n_clipped = _oracle_column(oracle, job["case"], job["kind"], x[b, :, c], c, job["dither"], job["seed"])
        total_clips += n_clipped
        got = y[b, :, c]
        assert got.shape == want.shape
        if f["kernel"] == "interp_tile" and f["pair"] == 2:   # by name: the 432 outputs around the seam k = h L
            seam = slice(f["nf_t"] - 216, f["nf_t"] + 216)
            assert np.array_equal(_bits(got[seam]), _bits(want[seam])), "clip %d channel %d: outputs around the halves seam %d differ" % (b, c, f["nf_t"])
        if name.startswith("b_4095"):                         # by name: zero extension at both ends
            assert np.array_equal(_bits(got[:216]), _bits(want[:216])), "the first 216 outputs differ"
            assert np.array_equal(_bits(got[-216:]), _bits(want[-216:])), "the last 216 outputs differ"
        bad = np.flatnonzero(_bits(got) != _bits(want))
        assert bad.size == 0, "clip %d channel %d: %d outputs differ from the oracle, the first at %d" % (b, c, bad.size, bad[0])
    if job["counter"]:
        print(name, "clip counter:", int(res["clips_" + name]), "oracle:", total_clips)
        assert int(res["clips_" + name]) == total_clips
        assert (total_clips > 0) == job["loud"]


def test_wide_job_runs_lane_per_output():
    """(f) the [40, 65536] interleaved float32 job in the default environment: ONE launch of kernel=interp on channel-fast data.
    launch_job folds jobs of more than 65535 columns into channel ranges, which used to hand this one to k_chain in two
    launches (65535 + 1 columns, 1252 us); a short constant-rate job on channel-fast data now stays whole and launch_gather
    gives it lane-per-output k_interp (253 us, the same bits).  test_form_guards_and_parity[f_wide*] compares the columns
    either side of 65535 and at both ends with the oracle — int16: the dither channel is the column's own index."""
    res = _results("default")
    lines = str(res["log_f_wide"]).splitlines()
    print("f_wide launches:", " | ".join(lines))
    assert len(lines) == 1, "one launch: %r" % lines
    f = _parse(lines[0])
    assert (f["kernel"], f["ch_fast"], f["cols"]) == ("interp", 1, 65536), f


def test_cross_form_identity():
    """One column, float32, 48000 -> 44101 HQ, through k_chain (both geometries), k_interp_wave and k_interp_tile: the outputs
    whose windows lie inside the shorter input have the same bits."""
    plan = _plan(MAIN)
    longest = "c_64ko_p1_f32"
    ref = _payload(longest, JOBS[longest], _results(JOBS[longest]["env"]))[0, :, 0]
    kernels = set()
    for name in SHARED:
        job = JOBS[name]
        assert (job["case"], job["kind"], job["ch"]) == (MAIN, "f32", 1)
        res = _results(job["env"])
        f = _parse(str(res["log_" + name]))
        kernels.add((f["kernel"], f.get("NO")))
        y = _payload(name, job, res)[0, :, 0]
        assert np.array_equal(_inputs()[name][0, :, 0], _inputs()[longest][0, :_frames(job), 0])
        # output k reads input frames below floor(k M / L) + T/2 + 1
        inside = int(((_frames(job) - plan.taps // 2 - 2) * plan.L) // plan.M)
        n = max(0, min(len(y), inside))
        assert n > len(y) - 220 * plan.L // plan.M - 2
        assert np.array_equal(_bits(y[:n]), _bits(ref[:n])), name
    assert kernels == {("chain", 8), ("chain", 32), ("interp_wave", None), ("interp_tile", None)}


def test_every_form_and_instance_ran():
    """Every (kernel, I/O type, variable rate, pair, twin) instance this file is about appears in some launch line."""
    seen = set()
    for env in ENVS:
        for key, v in _results(env).items():
            if key.startswith("log_"):
                for line in str(v).splitlines():
                    f = _parse(line)
                    seen.add((f["kernel"], f["io"], f["vr"], f.get("pair"), f.get("twin")))
    for want in [("chain", "f32", 0, None, None), ("chain", "i16", 0, None, None), ("interp", "f32", 0, None, None), ("interp", "i32", 0, None, None)] \
            + [("interp_wave", io, 0, None, None) for io in DTYPE] \
            + [("interp_tile", io, 0, 0, 0) for io in ("f32", "f64")] \
            + [("interp_tile", io, 0, pair, 0) for io in DTYPE for pair in (1, 2)] \
            + [("interp_tile", io, 0, pair, 1) for io in ("f32", "i16") for pair in (1, 2)] \
            + [("interp_tile", "f32", 1, 1, 1), ("interp_tile", "i16", 1, 1, 0), ("interp_tile", "f32", 1, 0, 0)]:
        assert want in seen, want


@pytest.mark.parametrize("name", list(STREAMS))
def test_variable_rate_tile(oracle, name):
    """(g) device.TensorStream(vr=True) against tests/vr_sim.py, as tests/test_gpu_vr.py: every chunk bit for bit."""
    env, ch, kind, chunks, expect = STREAMS[name]
    res, x = _results(env), _inputs()[name][0]
    sims = [VrSim(oracle, VR_CASE[0], VR_CASE[1], VR_CASE[2], DTYPE[kind]) for _ in range(ch)]
    at = 0
    for i, (n, change) in enumerate(chunks):
        lines = str(res["log_%s_%d" % (name, i)]).splitlines()
        print(name, "chunk", i, "launches:", " | ".join(lines))
        f = _parse(lines[0])
        assert len(lines) == 1 and {k: f.get(k) for k in expect[i]} == expect[i], f
        assert (f["io"], f["T"], f["P"], f["cols"]) == (kind, 736, 128, ch)
        if i:
            assert f["k0"] > 0, "the second chunk starts at a later output"
        y = res["y_%s_%d" % (name, i)].reshape(-1, ch)
        assert f["nf"] == len(y)
        for c in range(ch):
            want = sims[c].feed(x[at:at + n, c], last=False, channel=c)
            assert len(want) == len(y)
            bad = np.flatnonzero(_bits(np.ascontiguousarray(y[:, c])) != _bits(want))
            assert bad.size == 0, "chunk %d channel %d: %d outputs differ from the oracle, the first at %d" % (i, c, bad.size, bad[0])
        at += n
        if change:
            for s in sims:
                s.set_io_ratio(change[0] / change[1], change[2])
            assert sims[0].delta != 0 and len(chunks) > i + 1


def test_constant_rate_stream_second_chunk(oracle):
    """(h) a constant-rate device stream fed two chunks of the halves form each: the second launch has p0, d0 and in_abs0
    != 0, and its outputs are the matching slice of the one-shot oracle result."""
    res, x = _results(H_STREAM[0]), _inputs()["h_stream"][0, :, 0]
    want = oracle.resample_channel(oracle.plan(*MAIN), x, "port_f32")
    at = 0
    for i in range(len(H_STREAM[1])):
        lines = str(res["log_h_stream_%d" % i]).splitlines()
        print("h_stream chunk", i, "launches:", " | ".join(lines))
        f = _parse(lines[0])
        assert len(lines) == 1 and (f["kernel"], f["pair"], f["twin"], f["vr"]) == ("interp_tile", 2, 1, 0), f
        y = res["y_h_stream_%d" % i]
        assert f["nf"] == len(y) and f["k0"] == at and f["nf_t"] == f["h"] * f["L"] and f["h"] == -(-f["nf"] // (2 * f["L"])) == (1, 5)[i]
        if i:
            assert f["k0"] * f["M"] % f["L"] != 0 and f["k0"] * f["M"] // f["L"] > 0 and f["in_abs0"] > 0, f   # p0, d0, in_abs0
        bad = np.flatnonzero(_bits(y) != _bits(want[at:at + len(y)]))
        assert bad.size == 0, "chunk %d: %d outputs differ from the one-shot oracle, the first at %d" % (i, bad.size, bad[0])
        seam = slice(f["nf_t"] - 216, f["nf_t"] + 216)
        assert np.array_equal(_bits(y[seam]), _bits(want[at:at + len(y)][seam]))
        at += len(y)
