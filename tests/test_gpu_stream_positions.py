"""GPU: the kernels and the host code that take their positions from a STREAM HANDLE's counters (n_in_total, k_done, in_base,
the variable-rate clock), at positions up to 2^50.

tests/test_gpu_window_positions.py holds every kernel hipsoxr_run_device reaches with window fields to the oracle there; the
kernels below have no such entry — k_chain_multi (one item and many), the variable-rate forms (k_chain mode 2, k_interp,
k_interp_wave, k_interp_tile with the Q64.64 clock), k_chain_resident (48-bit mailbox words), the frequency-domain stream
window — nor has the host code between the counters and them (first_needed, stream_keep, stream_item_prepare / commit, the
host ring, deferred output, delay()).  No test can run a stream for 2^31 frames; the debug-switch build exports
hipsoxr_debug_stream_seek (csrc/engine.cpp debug_stream_seek), which moves a FRESH stream's counters to (in_frames,
out_frames): a time translation.  A constant-rate stream moved by whole periods is the fresh stream moved — the same counts
per call, the same phases, zeros in front of in_frames where the fresh one reads zeros in front of 0, the same frequency-domain
blocks relative to its ring (tests/c/stream_rules_check.cpp holds that in integers); a variable-rate stream takes any integer pair.

A case is one stream configuration fed a fixed sequence of chunks, then the end of input.  tests/_stream_seek_probe.py runs it
on a fresh handle and on the handle seeked to each position class, every run twice, in child processes on the debug-switch
build, one after another: `rules`, `lane` (HIPSOXR_NO_INTERP_WAVE: lane-per-output k_interp and the variable-rate k_interp_tile)
and `resident` (on its own).  Position classes, as the seek: (a) the outputs cross 2^31 inside a call, not at its first output;
(b) 2^32 likewise (the dither key passes 2^32 inside a launch); (c) the INPUT indices straddle 2^32, the outputs do not;
(d) just above 2^40; (e) just below 2^48 (everything a resident message carries still fits); (f) just above 2^50.  The
L = 4800037 plan's period is longer than any run here, so no whole number of periods puts a run across a given index: it is
run at (d)-(f), where k_done M lies beyond 2^63 at (e) and (f), and the 48000 -> 44101.5 plan (L = 29401) carries the
interpolated-phase paths through all six.

Compared here, tolerance zero:
  1  every call of a seeked run returns the fresh run's count, the counts are the model's, the total is the plan's length;
  2  GUARD frames of poison either side of each call's result, and everything behind it, untouched; every element written;
  3  floats and int32: the seeked run's bytes are the fresh run's, the frequency-domain stream's included; each run's repeat
     has the same bytes call by call;
  4  exact-engine streams: the fresh run is the oracle in port mode, the seeked run the oracle AT ITS POSITION (128-bit
     locate, tests/test_window_oracle.py; variable rate: tests/vr_sim.py with the translated clock);
  5  dithered int16: the seeked result differs from the fresh one and equals oracle.quantize keyed at out_frames + k of the
     float column (exact engine: the oracle's; frequency-domain stream: the float32 stream's own output on the same cut);
     num_clips() is the oracle's count in every run, and greater than zero on the loud cases;
  6  delay() after every call: the seeked handle's value equals the fresh handle's as doubles;
  7  each stream of a group (eight handles at eight positions, one launch per call) equals the same handle run alone;
  8  after clear() a seeked handle reproduces the fresh run; a seek of a fed handle, a seek off the period grid and a
     position from 2^62 on are refused by name; the product library does not export the symbol.
The launch log names the path of every run: the set of (kernel, mode, engine width) seen equals EXPECTED exactly, each at
every class and in the fresh run, and the gather family's lines carry the seek's k0 and in_abs0.

Found with this file and fixed (profiles/NOTES_stream_positions.md): delay() formed n_in_total L / M - k_done in doubles on
the counters themselves — off in its last bits from 2^31 on (62.81179141998291 for 62.811791383219955 at class a) and by up to
0.2 frames at 2^50; a resident stream beyond 2^48 launched and retired an instance in every call before it fell back.
delay() counts from the signal's start, which for a seeked handle is its seek: check 6 holds the handle's bookkeeping (pending
deferred frames, the clock after a slew), the arithmetic at large counts is held by tests/c/stream_rules_check.cpp."""
import ctypes
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _stream_seek_probe as sp  # noqa: E402
from vr_sim import ONE, VrSim, q64  # noqa: E402

PKG = os.path.join(os.path.dirname(HERE), "python-soxr_amd")
DBG_LIB = os.path.join(PKG, "_variants", "dbg", "libhipsoxr.so")
PRODUCT_LIB = os.path.join(PKG, "soxr_amd", "libhipsoxr.so")
NPDT = {"float32": np.float32, "float64": np.float64, "int16": np.int16, "int32": np.int32}
WIDTH = {"float32": 4, "float64": 8, "int16": 4, "int32": 8}
POS = sp.POSITIONS

G = (44100, 16000, "VHQ")       # L 160, M 441, T 736
P = (48000, 44100, "VHQ")       # L 147, M 160, T 296
A = (48000, 44101.5, "HQ")      # L 29401, M 32000: interpolated phases, a period short enough to straddle an index
B = (44100, 48000.37, "HQ")     # L 4800037, M 4410000: k_done M beyond 2^63 at (e) and (f)
V = (44100, 16000, "HQ")        # variable rate: the largest io ratio
V2 = (48000, 32000, "HQ")       # ... for the tile form's long call
ENVS = {"rules": {}, "lane": {"HIPSOXR_NO_INTERP_WAVE": "1"}, "resident": {}}
SEED = 0x5EED1234
SMALL = [441] * 20              # stream_item_prepare leaves room for sixteen chunks in a ring of 8192 frames: the 19th call moves it
MIXED = [441, 300] * 10
LONG = [441] * 56               # 24 696 frames: the L = 29401 / M = 32000 plan meets 2^32 23 296 input frames (10 414 outputs) into a period


def S(env, surface, rates, dtype, chunks, ch=1, classes=POS, vr=False, engine="exact", events=None, loud=False, expect=(), **kw):
    return dict(env=env, surface=surface, rates=list(rates), dtype=dtype, chunks=list(chunks), ch=ch, classes=list(classes), vr=vr, engine=engine,
                events={str(k): list(v) for k, v in (events or {}).items()}, dither=dtype == "int16", seed=SEED if dtype == "int16" else 0, loud=loud,
                expect=set(expect), **kw)


def K(kernel, dtype, mode=None):
    """a path as the launch log names it"""
    return (kernel if mode is None else "%s mode=%d" % (kernel, mode), WIDTH[dtype])


def _tensor(rates, dtype, chunks, mode, **kw):  # k_chain_multi with one item; the flush is a job of k_chain
    return S("rules", "tensor", rates, dtype, chunks, expect=[K("chain_multi", dtype, mode), K("chain", dtype, mode)], **kw)


CONST = {0: V[:2] + (0,)}
CASES = {
    # ---- k_chain_multi, one item (TensorStream, small calls) ----
    "cm0_f32": _tensor(G, "float32", SMALL, 0, ring_move=True), "cm0_f64": _tensor(P, "float64", MIXED, 0),
    "cm0_i16": _tensor(G, "int16", SMALL, 0, loud=True, ring_move=True), "cm0_i32": _tensor(P, "int32", MIXED, 0),
    "cm0_f32_stereo": _tensor(P, "float32", SMALL, 0, ch=2, ring_move=True),
    "cm1_f32": _tensor(A, "float32", LONG, 1), "cm1_f64": _tensor(A, "float64", LONG, 1), "cm1_i16": _tensor(A, "int16", LONG, 1, loud=True),
    "cm1b_f32": _tensor(B, "float32", SMALL, 1, classes=POS[3:]), "cm1b_f64": _tensor(B, "float64", SMALL, 1, classes=POS[3:]),
    "cm1b_i16": _tensor(B, "int16", SMALL, 1, classes=POS[3:], loud=True),
    # ---- k_chain_multi, eight items: one unseeked, one per class, a second (b) ----
    "grp_f32": S("rules", "group", G, "float32", SMALL, ring_move=True, expect=[K("chain_multi", "float32", 0)]),
    "grp_i16": S("rules", "group", G, "int16", SMALL, loud=True, ring_move=True, expect=[K("chain_multi", "int16", 0)]),
    # ---- variable rate: k_chain mode 2 (up to 512 outputs), k_interp_wave (from 513), a slew that begins in one call and ends in a later one ----
    "vr_chain_f32": S("rules", "tensor", V, "float32", [441] * 10, vr=True, events=CONST, expect=[K("chain", "float32", 2)]),
    "vr_chain_f64": S("rules", "tensor", V, "float64", [441] * 10, vr=True, events=CONST, expect=[K("chain", "float64", 2)]),
    "vr_chain_slew_i16": S("rules", "tensor", V, "int16", [441] * 10, vr=True, events={0: V[:2] + (0,), 3: (44100, 22050, 500)}, loud=True, slew=True,
                           expect=[K("chain", "int16", 2)]),
    "vr_wave_f64": S("rules", "tensor", V, "float64", [2000] * 4, vr=True, events=CONST, expect=[K("chain", "float64", 2), K("interp_wave", "float64")]),
    "vr_wave_slew_f32": S("rules", "tensor", V, "float32", [2000] * 5, vr=True, events={0: V[:2] + (0,), 1: (44100, 30000, 1500)}, slew=True,
                          expect=[K("chain", "float32", 2), K("interp_wave", "float32")]),
    "vr_wave_i16": S("rules", "tensor", V, "int16", [2000] * 4, vr=True, events=CONST, loud=True, expect=[K("chain", "int16", 2), K("interp_wave", "int16")]),
    # ---- lane-per-output k_interp (from 4096 outputs without k_interp_wave), k_interp_tile (from ~112 000: interp_tile_form's cost model) ----
    "vr_interp_f32": S("lane", "tensor", V, "float32", [14000] * 3, vr=True, events=CONST, expect=[K("interp", "float32"), K("chain", "float32", 2)]),
    "vr_interp_i16": S("lane", "tensor", V, "int16", [14000] * 3, vr=True, events=CONST, loud=True, expect=[K("interp", "int16"), K("chain", "int16", 2)]),
    "vr_interp_f64": S("lane", "tensor", V, "float64", [14000] * 3, vr=True, events=CONST, expect=[K("interp", "float64"), K("chain", "float64", 2)]),
    "vr_tile_f32": S("lane", "tensor", V2, "float32", [200000, 3000, 200000], vr=True, events={0: V2[:2] + (0,)},
                     expect=[K("interp_tile", "float32"), K("chain", "float32", 2)]),
    "vr_tile_f64": S("lane", "tensor", V2, "float64", [200000, 3000, 200000], vr=True, events={0: V2[:2] + (0,)},
                     expect=[K("interp_tile", "float64"), K("chain", "float64", 2)]),
    "vr_tile_i16": S("lane", "tensor", V2, "int16", [200000, 3000, 200000], vr=True, events={0: V2[:2] + (0,)}, loud=True,
                     expect=[K("interp_tile", "int16"), K("chain", "int16", 2)]),
    # ---- k_chain_resident (host ResampleStream(resident=True), 441-frame calls); at (f) the mailbox cannot carry the message ----
    "res0_f32": S("resident", "host", G, "float32", [441] * 12, resident=True, seek_first=True, expect=[K("chain_resident", "float32", 0), K("chain", "float32", 0)]),
    "res0_i16": S("resident", "host", G, "int16", [441] * 12, resident=True, loud=True, expect=[K("chain_resident", "int16", 0), K("chain", "int16", 0)]),
    "res1_f32": S("resident", "host", A, "float32", LONG, resident=True, expect=[K("chain_resident", "float32", 1), K("chain", "float32", 1)]),
    "res1b_f32": S("resident", "host", B, "float32", [441] * 12, resident=True, classes=POS[3:], expect=[K("chain_resident", "float32", 1), K("chain", "float32", 1)]),
    "res2_f32": S("resident", "host", V, "float32", [441] * 10, vr=True, resident=True, events={0: V[:2] + (0,), 3: (44100, 22050, 500)}, slew=True,
                  expect=[K("chain_resident", "float32", 2), K("chain", "float32", 2)]),
    "res2_i16": S("resident", "host", V, "int16", [441] * 10, vr=True, resident=True, seek_first=True, events=CONST, loud=True,
                  expect=[K("chain_resident", "int16", 2), K("chain", "int16", 2)]),
    # ---- the frequency-domain stream window: pair2 (mono), strided2_cp (interleaved stereo); three chunks of unequal size ----
    "fft_f32": S("rules", "tensor", P, "float32", [30000, 7000, 48001], engine="fft", expect=[("fft pair2 f32", 4)]),
    "fft_f64": S("rules", "tensor", P, "float64", [30000, 7000, 48001], engine="fft", expect=[("fft pair2 f64", 8)]),
    "fft_i16": S("rules", "tensor", P, "int16", [30000, 7000, 48001], engine="fft", loud=True, float_twin="fft_f32_of_i16", expect=[("fft pair2 i16", 4)]),
    "fft_f32_of_i16": S("rules", "tensor", P, "float32", [30000, 7000, 48001], engine="fft", loud=True, sig_from="int16", sig_of="fft_i16", expect=[("fft pair2 f32", 4)]),
    "fft_i32": S("rules", "tensor", P, "int32", [30000, 7000, 48001], engine="fft", expect=[("fft pair2 i32", 8)]),
    "fft_g_f32": S("rules", "tensor", G, "float32", [44100, 5000, 61000], engine="fft", expect=[("fft pair2 f32", 4)]),
    "fft_st_f32": S("rules", "tensor", G, "float32", [44100, 5000, 61000], ch=2, engine="fft", expect=[("fft strided2_cp f32", 4)]),
    "fft_st_i16": S("rules", "tensor", G, "int16", [44100, 5000, 61000], ch=2, engine="fft", loud=True, float_twin="fft_st_f32_of_i16", expect=[("fft strided2_cp i16", 4)]),
    "fft_st_f32_of_i16": S("rules", "tensor", G, "float32", [44100, 5000, 61000], ch=2, engine="fft", loud=True, sig_from="int16", sig_of="fft_st_i16",
                           expect=[("fft strided2_cp f32", 4)]),
    # ---- host paths on the counters: the host ring, deferred output, a call large enough to move the ring to the device ----
    "host_i16": S("rules", "host", G, "int16", [441] * 12, loud=True, seek_first=True, expect=[K("chain", "int16", 0)]),
    "host_def_i16": S("rules", "host", G, "int16", [441] * 12, loud=True, deferred=True, expect=[K("chain", "int16", 0)]),
    "host_big_f32": S("rules", "host", G, "float32", [441, 441, 20000, 441], expect=[K("chain", "float32", 0), ("gather_wave", 4)]),
}
for _i, (_name, _c) in enumerate(CASES.items()):
    _c["name"], _c["sig_seed"] = _name, 9000 + 10 * _i
for _c in CASES.values():
    if _c.get("sig_of"):
        _c["sig_seed"] = CASES[_c["sig_of"]]["sig_seed"]
EXPECTED = set().union(*[c["expect"] for c in CASES.values()])


# ---- geometry, counts, seeks: Python integers ----------------------------------------------------------------------------------
class SeekSim(VrSim):
    """tests/vr_sim.py with the clock moved to (in0, out0): input frame 0 of the signal is absolute frame in0, the first output
    is out0 — what debug_stream_seek does to a fresh variable-rate stream.  compute=False: counts alone."""
    _plans = {}

    def __init__(self, oracle, rates, dtype, in0=0, out0=0, seed=0):
        key = tuple(rates)
        if key not in SeekSim._plans:
            SeekSim._plans[key] = oracle.VrPlan(*rates)
        self.o, self.vp = oracle, SeekSim._plans[key]
        self.H, self.dtype, self.eng = self.vp.T // 2, np.dtype(dtype), oracle.engine_of(dtype)
        self.in0, self.seed = in0, seed
        self.k_s = self.k_done = out0
        self.n_slew = self.delta = 0
        self.t_s = in0 * ONE
        self.s0 = self.s1 = q64(float(rates[0]) / float(rates[1]))
        self.x = np.zeros(0, np.float64)

    def _limit(self, ended):
        n_in = self.in0 + len(self.x)
        if ended:
            ok = lambda k: self.pos(k) + (self.step(k) // 2 if self.step(k) >= 0 else -((-self.step(k)) // 2)) <= n_in * ONE  # noqa: E731
        else:
            ok = lambda k: (self.pos(k) >> 64) + self.H <= n_in - 1  # noqa: E731
        k = self.k_done
        if not ok(k):
            return k
        lo, span = k, 1
        while ok(lo + span):
            lo, span = lo + span, span * 2
        hi = lo + span
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if ok(mid) else (lo, mid)
        return hi

    def call(self, chunk, last, compute=True):
        """one call of the stream: everything due, one position law per stretch -> (count, frames or None)"""
        self.x = np.concatenate([self.x, np.asarray(chunk, np.float64)])
        k_end, k0, outs = self._limit(last), self.k_done, []
        while self.k_done < k_end:
            slew_end = self.k_s + self.n_slew
            slewing = self.n_slew and self.k_done < slew_end
            stop = min(k_end, slew_end) if slewing else k_end
            if compute:
                v = self.o.vr_run(self.vp, self.x, "port_" + self.eng, stop - self.k_done, self.pos(self.k_done), self.step(self.k_done), self.delta if slewing else 0,
                                  in_abs0=self.in0)
                outs.append(self.o.quantize(v, self.dtype, channel=0, k0=self.k_done, dither=True, seed=self.seed))
            self.k_done = stop
        return k_end - k0, outs


def _geometry(oracle, case):
    if case["vr"]:
        return None
    pl = oracle.plan(*case["rates"])
    return pl.L, pl.M, pl.T


def _vr_run(oracle, case, seek, x=None):
    """the model of a variable-rate run -> (frames per call with the flush last, frames or None, clips)"""
    sim = SeekSim(oracle, case["rates"], NPDT[case["dtype"]], *(seek or (0, 0)), seed=case["seed"])
    counts, parts, clips, pos = [], [], 0, 0
    for i, c in enumerate(case["chunks"] + [0]):
        if str(i) in case["events"]:
            ev = case["events"][str(i)]
            sim.set_io_ratio(float(ev[0]) / float(ev[1]), ev[2])
        chunk = np.zeros(c) if x is None else x[pos:pos + c, 0]
        n, outs = sim.call(chunk, i == len(case["chunks"]), compute=x is not None)
        pos += c
        counts.append(n)
        parts += [o[0] for o in outs]
        clips += sum(o[1] for o in outs)
    return counts, (np.concatenate(parts)[:, None] if parts else None), clips


_counts_cache = {}


def _counts(oracle, case):
    """frames per call of the case's run (the flush last), whatever the position"""
    if case["name"] not in _counts_cache:
        g = _geometry(oracle, case)
        _counts_cache[case["name"]] = _vr_run(oracle, case, None)[0] if g is None else sp.call_counts(*g, case["chunks"])
    return _counts_cache[case["name"]]


def _seek(oracle, case, cls):
    """-> (in_frames, out_frames) of class cls"""
    counts, n_in = _counts(oracle, case), sum(case["chunks"])
    if case["vr"]:
        return sp.clock_pair(counts, n_in, cls)
    L, M, _ = _geometry(oracle, case)
    q = sp.periods(L, M, counts, n_in, cls)
    assert q is not None, (case["name"], cls)
    return q * M, q * L


def _second_b(oracle, case):
    """another whole number of periods of class (b)"""
    (L, M, _), counts, n_in = _geometry(oracle, case), _counts(oracle, case), sum(case["chunks"])
    q = sp.periods(L, M, counts, n_in, "b_out_2p32")
    for dq in (-3, 3, -5, 5, -1, 1):
        if sp.class_holds((q + dq) * M, (q + dq) * L, counts, n_in, "b_out_2p32"):
            return (q + dq) * M, (q + dq) * L
    raise AssertionError("no second position of class (b)")


GROUP_RUNS = ["fresh"] + list(POS) + ["b_second"]


def _seeks(oracle, case):
    """run -> seek of a case (a group: the list of its eight streams' seeks)"""
    if case["surface"] == "group":
        return [None] + [list(_seek(oracle, case, cls)) for cls in POS] + [list(_second_b(oracle, case))]
    runs = [("fresh", None)] + [(cls, list(_seek(oracle, case, cls))) for cls in case["classes"]]
    # seek_first: the handle's first chunk ever follows a seek (the probe makes the runs in this order) — where the ring lives is
    # decided there (engine.cpp stream_unfed), and only a ring in host memory gets the resident kernel
    return dict(runs[1:] + runs[:1] if case.get("seek_first") else runs)


def _job(oracle, case):
    """the case as the probe reads it"""
    job = {k: v for k, v in case.items() if k not in ("expect", "classes")}
    job["seeks"], job["cap"] = _seeks(oracle, case), max(_counts(oracle, case)) + 64
    if case["loud"]:  # white noise whose resampled copy has an RMS of about 13000 LSB: about one output in a hundred saturates
        g = _geometry(oracle, case)
        job["loud"] = int(13000 / min(1.0, (g[0] / g[1]) if g else case["rates"][1] / case["rates"][0]) ** 0.5)  # (the filter keeps min(1, L / M) of its power)
    else:
        job["loud"] = 0
    if case["surface"] == "group":
        job["seed"] = [(SEED + 7919 * i) & 0xFFFFFFFF if case["dither"] else 0 for i in range(len(job["seeks"]))]
    return job


# ---- no GPU ----------------------------------------------------------------------------------------------------------------------
def test_positions_are_what_they_are_called(oracle):
    """every run sits in the class it is called; a constant-rate seek is whole periods; the first call leaves k_done off a
    period boundary; (e) and (f) of the L = 4800037 plan need the 128-bit product; (e) fits a resident message"""
    for case in CASES.values():
        counts, n_in, g = _counts(oracle, case), sum(case["chunks"]), _geometry(oracle, case)
        assert counts[0] > 0, case["name"]
        runs = _seeks(oracle, case)
        pairs = zip(GROUP_RUNS, runs) if case["surface"] == "group" else runs.items()
        for run, seek in pairs:
            if seek is None:
                continue
            cls = "b_out_2p32" if run == "b_second" else run
            in0, out0 = seek
            assert sp.class_holds(in0, out0, counts, n_in, cls), (case["name"], run, seek)
            assert max(in0 + n_in, out0 + sum(counts)) < 2 ** 62
            if g:
                L, M, _ = g
                assert in0 * L == out0 * M and (out0 + counts[0]) % L != 0, (case["name"], run)
                if tuple(case["rates"]) == B and cls in POS[4:]:
                    assert out0 * M > 2 ** 63
                if cls == "e_2p48":  # in_abs0, out_k0 + n and d0 = floor(out_k0 M / L) below the mailbox's 2^48
                    assert in0 + n_in < 2 ** 48 and out0 + sum(counts) < 2 ** 48 and (out0 + sum(counts)) * M // L < 2 ** 48
        if case["surface"] == "group":
            assert len({None if s is None else tuple(s) for s in runs}) == 8, "eight different positions"
    # the period of the L = 4800037 plan is longer than any run: no whole number of periods crosses 2^31, 2^32 in it
    case = CASES["cm1b_f32"]
    assert all(sp.periods(*_geometry(oracle, case)[:2], _counts(oracle, case), sum(case["chunks"]), cls) is None for cls in POS[:3])
    # every path of the issue's table is expected somewhere, and at every class
    for key in EXPECTED:
        classes = set().union(*[set(c["classes"]) for c in CASES.values() if key in c["expect"]])
        assert classes == set(POS) or key[0].startswith("chain_resident"), (key, classes)


def test_the_seek_is_exported_by_the_debug_build_alone():
    """nm -D: the debug-switch library defines hipsoxr_debug_stream_seek, the product does not (tests/test_cabi.py holds its
    export list to the header's); ctypes answers AttributeError for the symbol on the product library"""
    assert os.path.exists(DBG_LIB) and os.path.exists(PRODUCT_LIB), "build.sh makes the debug-switch build beside the product"
    sym = lambda path: set(re.findall(r" T (hipsoxr_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)))  # noqa: E731
    dbg, product = sym(DBG_LIB), sym(PRODUCT_LIB)
    assert dbg - product == {"hipsoxr_debug_stream_seek"} and product <= dbg
    with open(os.path.join(os.path.dirname(HERE), "include", "hipsoxr.h")) as f:
        assert "hipsoxr_debug_stream_seek" not in f.read()
    with pytest.raises(AttributeError):
        ctypes.CDLL(PRODUCT_LIB).hipsoxr_debug_stream_seek


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def results(oracle, tmp_path_factory):
    """environment -> the probe's results: one child process per environment, one after another; a child that ends on a
    signal or its time limit ends the run"""
    assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
    tmp = tmp_path_factory.mktemp("stream_positions")
    out = {}
    for tag, extra in ENVS.items():
        jobs = [_job(oracle, c) for c in CASES.values() if c["env"] == tag]
        if tag == "rules":
            L, M, _ = _geometry(oracle, CASES["cm0_f32"])
            jobs.append(dict(_job(oracle, CASES["cm0_f32"]), name="refusals", surface="refusals", q=2 ** 40 // L, LM=[L, M]))
        with open(tmp / (tag + ".json"), "w") as f:
            json.dump(jobs, f)
        env = {key: v for key, v in os.environ.items() if not key.startswith("HIPSOXR_")}
        env.update({"HIPSOXR_LIBRARY": DBG_LIB, "HIPSOXR_DEBUG_LAUNCH_LOG": str(tmp / (tag + ".log"))})
        env.update(extra)
        p = subprocess.Popen([sys.executable, os.path.join(HERE, "_stream_seek_probe.py"), str(tmp / (tag + ".json")), str(tmp / (tag + ".npz"))], env=env,
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        try:
            _, err = p.communicate(timeout=300)
        finally:
            if p.poll() is None:
                p.kill()
        assert p.returncode == 0, (tag, p.returncode, err[-3000:])  # (raises: no further child is started)
        out[tag] = np.load(tmp / (tag + ".npz"))
    return out


def _lines(log):
    out = []
    for line in str(log).splitlines():
        f = dict(tok.split("=", 1) for tok in line.split())
        out.append({k: (int(v) if re.fullmatch(r"-?\d+", v) else v) for k, v in f.items()})
    return out


def _key(f):
    if "form" in f:
        return ("fft %s %s" % (f["form"], f["kind"]), 8 if f["kind"] in ("f64", "i32") else 4)
    k = f["kernel"]
    return (k + (" mode=%d" % f["mode"] if k.startswith("chain") else ""), f["width"])


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _per_call(y, counts):
    edges = np.cumsum([0] + list(counts))
    return [y[a:b] for a, b in zip(edges[:-1], edges[1:])]


def _runs(case):
    """(key in the results, run name, class or None) of every run of a case"""
    if case["surface"] == "group":
        return [("%s_%s%d" % (case["name"], kind, i), run, None if run == "fresh" else "b_out_2p32" if run == "b_second" else run)
                for kind in "gs" for i, run in enumerate(GROUP_RUNS)]
    return [(case["name"] + "_fresh", "fresh", None)] + [("%s_%s" % (case["name"], cls), cls, cls) for cls in case["classes"]]


@pytest.mark.gpu
def test_every_listed_path_served_every_position_class(oracle, results):
    """the (kernel, mode, engine width) of the launch logs are EXPECTED, exactly; each was seen in a fresh run and at every
    class (a)-(f) — k_chain_resident at (a)-(e): at (f) the log must not name it; the gather family's lines carry the seek"""
    seen = {}
    for case in CASES.values():
        res, seeks = results[case["env"]], _seeks(oracle, case)
        for key, run, cls in _runs(case):
            if case["surface"] == "group" and key.split("_")[-1][0] == "s":
                continue  # (the streams alone: cm0's path)
            lines = _lines(res["log_" + key])
            assert lines, (key, "no launch was logged")
            kinds = {_key(f) for f in lines}
            assert kinds <= case["expect"], (key, kinds - case["expect"])
            for k in kinds:
                seen.setdefault(k, set()).add(cls)
            seek = (seeks[GROUP_RUNS.index(run)] if case["surface"] == "group" else seeks[run]) or (0, 0)
            if "k0" in lines[0]:  # the run's first launch: the seek's own numbers
                assert (lines[0]["in_abs0"], lines[0]["k0"]) == tuple(seek), (key, lines[0], seek)
            if case["surface"] != "group" and not case.get("resident"):  # (a resident instance that idled out is launched again: not one line per call)
                fresh = _lines(res["log_" + case["name"] + "_fresh"])
                assert [_key(f) for f in lines] == [_key(f) for f in fresh], (key, "another sequence of launches than the fresh run's")
                # (the ring's base is the seek's in_frames plus what was retired so far — which depends on the capacity the handle's
                #  ring had when the run began, not on the position: inside the frames fed, no more is asked of it)
                assert all(f["k0"] - seek[1] == g["k0"] and f["nf"] == g["nf"] and 0 <= f["in_abs0"] - seek[0] <= sum(case["chunks"])
                           for f, g in zip(lines, fresh) if "k0" in f), (key, [(f["k0"], f["in_abs0"]) for f in lines if "k0" in f], seek)
            if case["surface"] == "group":
                assert all(f["items"] == 8 for f in lines) and len(lines) == len(case["chunks"]), (key, "one launch of eight items per call")
            if case.get("ring_move"):
                assert any(f.get("moving") for f in lines[1:] if f["kernel"] == "chain_multi"), (key, "no call moved the ring")
            if case.get("resident"):
                named = any(f["kernel"] == "chain_resident" for f in lines)
                assert named == (cls != "f_2p50"), (key, "resident instance launched" if named else "no resident instance")
            if cls == "f_2p50":
                print(key, "|", str(res["log_" + key]).splitlines()[min(1, len(lines) - 1)])
    assert set(seen) == EXPECTED, (sorted(set(seen) - EXPECTED), sorted(EXPECTED - set(seen)))
    for k, classes in seen.items():
        want = {None} | set(POS[:5] if k[0].startswith("chain_resident") else POS)
        assert classes == want, (k, classes)


def _oracle_run(oracle, case, seek, x, seed):
    """the exact engine's result of a whole run at its position -> (frames [n, ch], clips)"""
    in0, out0 = seek or (0, 0)
    if case["vr"]:
        _, y, clips = _vr_run(oracle, dict(case, seed=seed), seek, x)
        return y, clips
    pl, dt = oracle.plan(*case["rates"]), NPDT[case["dtype"]]
    eng = oracle.engine_of(dt)
    real = np.float32 if eng == "f32" else np.float64
    n_out = pl.out_len(len(x))
    want, clips = np.empty((n_out, case["ch"]), dt), 0
    for c in range(case["ch"]):
        y = oracle.resample_channel(pl, np.ascontiguousarray(x[:, c]).astype(real), "port_" + eng, k0=out0, n_out=n_out, in_abs0=in0)
        want[:, c], n = oracle.quantize(y, dt, channel=c, k0=out0, dither=case["dither"], seed=seed)
        clips += n
    return want, clips


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_seeked_streams_equal_the_oracle_and_the_fresh_stream(oracle, results, name):
    case = CASES[name]
    res, job = results[case["env"]], None
    job = _job(oracle, case)
    counts, dt, ch, group = _counts(oracle, case), NPDT[case["dtype"]], case["ch"], case["surface"] == "group"
    exact, differed, clipped = case["engine"] == "exact", 0, 0
    model = [c for c in counts if c] if not case.get("deferred") else None  # (the probe records the flush's calls that returned frames)
    for key, run, cls in _runs(case):
        stream = int(key.rsplit("_", 1)[1][1:]) if group else 0
        alone = group and key.rsplit("_", 1)[1][0] == "s"
        seek = job["seeks"][stream] if group else job["seeks"][run]
        fresh_key = key.rsplit("_", 1)[0] + "_" + key.rsplit("_", 1)[1][0] + "0" if group else name + "_fresh"  # (group: its unseeked stream)
        y, n = res["y_" + key], [int(v) for v in res["n_" + key]]
        y = y.reshape(-1, ch)
        print(key, "counts", n[:4], "... total", sum(n), "delay", list(res["d_" + key][:3]), "clips", int(res["c_" + key]))
        # 1 counts
        n_live = [c for c in n if c]
        if model is not None:
            assert n_live == model, (key, n, counts)
        assert n == [int(v) for v in res["n_" + fresh_key]] and sum(n) == sum(counts) == len(y), (key, n)
        # 2 sentinels
        assert bool(res["g_" + key]), "a frame outside a call's result was written: " + key
        assert y.dtype == dt
        if dt in (np.float32, np.float64):
            assert not (y == sp.POISON).any() and np.isfinite(y).all(), "a payload element was not written: " + key
        elif dt == np.int32:  # (samples of RMS 2^28: none equals the poison by right; int16 payloads are held to the oracle below, element by element)
            assert not (y == sp.POISON).any(), "a payload element was not written: " + key
        # 6 delay() after every call
        assert res["d_" + key].tobytes() == res["d_" + fresh_key].tobytes(), (key, list(res["d_" + key]), list(res["d_" + fresh_key]))
        if alone:  # 7 the stream of the group against the same handle alone
            g = key.replace("_s%d" % stream, "_g%d" % stream)
            assert y.tobytes() == res["y_" + g].tobytes() and int(res["c_" + key]) == int(res["c_" + g]), (key, "differs from the grouped run")
            continue
        # 3 the repeat, call by call
        assert [str(h) for h in res["hr_" + key]] == [_sha(p) for p in _per_call(y, n)] and [int(v) for v in res["nr_" + key]] == n, (key, "the repeat differs")
        assert bool(res["gr_" + key]) and res["dr_" + key].tobytes() == res["d_" + key].tobytes() and int(res["cr_" + key]) == int(res["c_" + key]), key
        fresh = res["y_" + fresh_key].reshape(-1, ch)
        if not case["dither"] and not group:
            assert y.tobytes() == fresh.tobytes(), "moving the stream to %r changed bits of the result: %s" % (seek, key)
        # 4, 5 the oracle at the run's position
        x = sp.signal(job, stream)
        seed = job["seed"][stream] if group else job["seed"]
        if exact:
            want, n_clips = _oracle_run(oracle, case, seek, x, seed)
        else:
            want = n_clips = None
            if case.get("float_twin"):  # the float32 stream's own output on the same cut, through the output stage keyed at out_frames + k
                twin = results[case["env"]]["y_%s_%s" % (case["float_twin"], run)].reshape(-1, ch)
                want, n_clips = np.empty_like(y), 0
                for c in range(ch):
                    want[:, c], k = oracle.quantize(np.ascontiguousarray(twin[:, c]), dt, channel=c, k0=(seek or (0, 0))[1], dither=True, seed=seed)
                    n_clips += k
        if want is not None:
            bad = np.argwhere(y != want)
            assert y.shape == want.shape and bad.size == 0, "%s: %d elements differ from the oracle at %r, first at %r: %r against %r" % (
                key, len(bad), seek, tuple(bad[0]), y[tuple(bad[0])], want[tuple(bad[0])])
            assert y.tobytes() == want.tobytes(), key
            if dt in (np.int16, np.int32):
                assert int(res["c_" + key]) == n_clips, (key, int(res["c_" + key]), n_clips)
                clipped += n_clips
        if case["dither"] and seek is not None and not group:
            assert y.tobytes() != fresh.tobytes(), "a dithered result equals the fresh stream's: the key ignores the position: " + key
            differed += 1
    if case["loud"] and dt == np.int16 and (exact or case.get("float_twin")):
        assert 0 < clipped < sum(counts) * ch * len(_runs(case)) // 10, clipped
    if not group:
        # 8 after clear() the handle is a fresh stream again
        fresh = res["y_" + name + "_fresh"].reshape(-1, ch)
        assert [str(h) for h in res["hc_" + name]] == [_sha(p) for p in _per_call(fresh, [int(v) for v in res["n_" + name + "_fresh"]])], name
        if case["dither"]:
            assert differed == len(case["classes"])
    if case["vr"] and not case.get("slew"):  # a constant ratio: the plan's own length rule
        from soxr_amd import device as dev
        ev = case["events"]["0"]
        assert dev.Plan(*case["rates"], vr=True).vr_out_len(sum(case["chunks"]), float(ev[0]) / float(ev[1])) == sum(counts)


@pytest.mark.gpu
def test_the_seek_refuses_by_name(results):
    ans = json.loads(str(results["rules"]["refusals"]))
    assert ans["fresh_whole"] is None and ans["cleared"] is None, ans
    assert "whole periods" in ans["off_period"] and "whole periods" in ans["off_period_out"], ans
    assert "not at zero" in ans["fed"] and "not at zero" in ans["twice"] and "has ended" in ans["ended"], ans
    assert "out of range" in ans["range"] and ans["null"] == "null argument", ans
