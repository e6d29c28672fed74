"""GPU: window jobs of the exact engine at stream positions up to 2^50, every kernel hipsoxr_run_device reaches with window
fields, against the oracle at the job's own position and against the same job moved down by whole periods.

The contract (include/hipsoxr.h): in_abs0 places in[0] on an absolute input index, out_k0 names the first output, the signal
is zero outside [in_abs0, in_abs0 + in_frames).  A stream carries positions beyond 2^31 after half a day and beyond 2^32 after
a day; the position arithmetic is spread over the kernels below and their launchers, and a 32-bit cast on the wrong side of
one subtraction would pass every other test of the suite.  A job here is Plan.run on a short signal placed at in_abs0, asking
for outputs [k0, k0 + n_out), k0 = q L + r with r no multiple of L:

  positions    (a) the outputs straddle 2^31; (b) the outputs straddle 2^32 (the dither key and every k - out_k0 cross inside
               the launch); (c) the INPUT indices straddle 2^32 while the outputs do not; (d), (e), (f) k0 just above 2^40,
               2^47, 2^50 — on the L = 4800037 plan k0 M is 2^62.07 at (d) and beyond 2^63 at (e) and (f)
               (make_gather_args' 128-bit product);
  placements   with n0 the first tap of output k0 (a multiple of 4 here): in_abs0 = n0 exactly; n0 - 5 (spare history, an odd
               base: the tile kernels stage sample by sample); n0 + 3 (the first outputs read zeros in front of the window);
               in_frames two short of what the last output reads (zeros behind);
  kernels      chain mode 0 with NO = 8 and NO = 32, gather_wave, lane-per-output gather, tile, tile_mfma (float32 and
               float64 engines), tile_mfma_p, tile_mfma64_p, chain mode 1, interp, interp_wave, interp_tile — at the smallest
               shapes that reach them (the tables of test_gpu_gather_forms.py, test_gpu_tile_forms.py and
               test_gpu_interp_forms.py); a tile job is 2.5 slabs long, so one slab is interior and two are not.  One form of
               each: position arithmetic is per kernel, not per split or halves form;
  types        float32 and float64 on every kernel (the two planar kernels have one engine each); int16 with dither, a
               non-zero seed, a clip counter and a level at which a few samples saturate on one float32-engine kernel of
               each family; int32 on one float64-engine kernel of each family; one stereo interleaved case per family.

Every (variant, position, placement) is one job; the probe (tests/_window_probe.py) runs it twice — at its position and
moved down by q periods, (k0 - q L, in_abs0 - q M) — in two child processes for the whole file: the rules as they are, and
HIPSOXR_NO_CHAIN + HIPSOXR_NO_GATHER_WAVE + HIPSOXR_NO_INTERP_WAVE for the lane-per-output kernels and the smallest
k_interp_tile job.  Compared here, tolerance zero (a result is a pure function of absolute positions):

  * the launch log: the stated kernel served both runs, and the gather family's lines carry the k0 and in_abs0 passed;
  * GUARD frames of poison either side untouched, every payload element written;
  * the payload equals the oracle in port mode AT THE JOB'S POSITION (128-bit locate), through oracle.quantize for integers
    (dither keyed by the absolute output index), bit for bit, and the clip count equals the oracle's;
  * the moved job has the same bytes (SHA-256) — float types and int32; the dithered int16 result DIFFERS from its moved
    twin, and the twin equals the oracle's output stage keyed at the twin's position.

Every kernel of the list is reachable with window fields: launch_typed / launch_gather (csrc/kernels.hip) read nothing of the
window when they pick a form, and no launcher refuses or reroutes one.  Not reachable through a job at all — their positions
come from a stream handle's counters, which no product entry point sets: k_chain_multi, the variable-rate kernels (mode 2),
k_chain_resident, launch_fft_window.  tests/test_gpu_stream_positions.py holds those, through the debug-switch build's seek
(profiles/NOTES_stream_positions.md)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _window_probe as wp  # noqa: E402

DBG_LIB = os.path.join(os.path.dirname(HERE), "python-soxr_amd", "_variants", "dbg", "libhipsoxr.so")
GATHER, TILE_VALU, EXACT = 1, 3, 6
NPDT = {"float32": np.float32, "float64": np.float64, "int16": np.int16, "int32": np.int32}
IO = {"float32": "f32", "float64": "f64", "int16": "i16", "int32": "i32"}
WIDTH = {"float32": 4, "float64": 8, "int16": 4, "int32": 8}

PLANAR = (48000, 44100, "VHQ")     # L 147, M 160, T 296: planes (k_tile_mfma_p, k_tile_mfma64_p); k_tile stages 16-byte rows
GENERAL = (44100, 16000, "VHQ")    # L 160, M 441, T 736: k_tile_mfma; k_tile stages rows of an odd length
INTERP_A = (48000, 44101.5, "HQ")  # L 29401, M 32000, 32 phase intervals
INTERP_B = (44100, 48000.37, "HQ") # L 4800037, M 4410000: k0 M passes 2^63 in classes (e) and (f)
ENVS = {"rules": {}, "lane": {"HIPSOXR_NO_CHAIN": "1", "HIPSOXR_NO_GATHER_WAVE": "1", "HIPSOXR_NO_INTERP_WAVE": "1"}}

# kernel -> (the log's fields that name it, plan, selector, outputs per job, environment).  Sizes: k_chain serves fewer than 4096
# outputs, 8 per workgroup up to 512; k_gather_wave 4096 and more under HIPSOXR_KERNEL_GATHER; the lane kernels three
# workgroups of 256; a tile job 2.5 slabs of the form its size gets (k_tile: 64 periods of 147, float64 on GENERAL 32 of 160;
# k_tile_mfma small form: 16 of 160; k_tile_mfma_p: 64 or 32 of 147; k_tile_mfma64_p: 16 or 32 of 147), each above the tile
# family's threshold (4096 outputs, 16 periods); k_interp_wave from 513 outputs; k_interp_tile against lane-per-output
# k_interp from 25.2 x 960 outputs (interp_tile_form: 6.3e-5 x KO against 2.5e-6 us per output and tap, KO <= 30 x 32)
KERNELS = {
    "chain8": (dict(kernel="chain", mode=0, NO=8), GENERAL, EXACT, 300, "rules"),
    "chain32": (dict(kernel="chain", mode=0, NO=32), PLANAR, EXACT, 1501, "rules"),
    "gather_wave": (dict(kernel="gather_wave"), PLANAR, GATHER, 4501, "rules"),
    "gather": (dict(kernel="gather"), GENERAL, GATHER, 701, "lane"),
    "tile": (dict(kernel="tile"), PLANAR, TILE_VALU, 23531, "rules"),
    "tile_general": (dict(kernel="tile"), GENERAL, TILE_VALU, 12811, "rules"),
    "tile_mfma": (dict(kernel="tile_mfma"), GENERAL, EXACT, 6403, "rules"),
    "tile_mfma_p": (dict(kernel="tile_mfma_p"), PLANAR, EXACT, 23531, "rules"),
    "tile_mfma64_p": (dict(kernel="tile_mfma64_p"), PLANAR, EXACT, 11771, "rules"),
    "chain_interp": (dict(kernel="chain", mode=1, NO=8), INTERP_B, EXACT, 300, "rules"),
    "interp": (dict(kernel="interp"), INTERP_A, EXACT, 701, "lane"),
    "interp_wave": (dict(kernel="interp_wave"), INTERP_B, EXACT, 1501, "rules"),
    "interp_tile": (dict(kernel="interp_tile"), INTERP_A, EXACT, 26001, "lane"),
}


def V(kernel, dtype, ch=1, **kw):
    return dict(kernel=kernel, dtype=dtype, ch=ch, dither=kw.get("dither", False), dither_seed=kw.get("seed", 0), loud=kw.get("loud", False),
                counter=kw.get("counter", False))


I16 = dict(dither=True, seed=0x5EED1234, loud=True, counter=True)
VARIANTS = {
    # float32 and float64 on every kernel
    "chain8_f32": V("chain8", "float32"), "chain8_f64": V("chain8", "float64"),
    "chain32_f32": V("chain32", "float32"), "chain32_f64": V("chain32", "float64"),
    "gather_wave_f32": V("gather_wave", "float32"), "gather_wave_f64": V("gather_wave", "float64"),
    "gather_f32": V("gather", "float32"), "gather_f64": V("gather", "float64"),
    "tile_f32": V("tile", "float32"), "tile_f64": V("tile_general", "float64"),
    "tile_mfma_f32": V("tile_mfma", "float32"), "tile_mfma_f64": V("tile_mfma", "float64"),
    "tile_mfma_p_f32": V("tile_mfma_p", "float32"), "tile_mfma64_p_f64": V("tile_mfma64_p", "float64"),
    "chain_interp_f32": V("chain_interp", "float32"), "chain_interp_f64": V("chain_interp", "float64"),
    "interp_f32": V("interp", "float32"), "interp_f64": V("interp", "float64"),
    "interp_wave_f32": V("interp_wave", "float32"), "interp_wave_f64": V("interp_wave", "float64"),
    "interp_tile_f32": V("interp_tile", "float32"), "interp_tile_f64": V("interp_tile", "float64"),
    # int16, dithered, on a float32-engine kernel of each family
    "chain8_i16": V("chain8", "int16", **I16), "gather_wave_i16": V("gather_wave", "int16", **I16),
    "tile_mfma_p_i16": V("tile_mfma_p", "int16", **I16), "tile_mfma_i16": V("tile_mfma", "int16", **I16),
    "interp_wave_i16": V("interp_wave", "int16", **I16),
    # int32 on a float64-engine kernel of each family
    "chain32_i32": V("chain32", "int32", counter=True), "gather_wave_i32": V("gather_wave", "int32", counter=True),
    "tile_mfma64_p_i32": V("tile_mfma64_p", "int32", counter=True), "tile_mfma_i32": V("tile_mfma", "int32", counter=True),
    "interp_wave_i32": V("interp_wave", "int32", counter=True),
    # stereo, interleaved: one per family
    "chain8_f32_stereo": V("chain8", "float32", 2), "gather_wave_f64_stereo": V("gather_wave", "float64", 2),
    "tile_mfma_p_i16_stereo": V("tile_mfma_p", "int16", 2, **I16), "tile_mfma_f32_stereo": V("tile_mfma", "float32", 2),
    "interp_wave_f32_stereo": V("interp_wave", "float32", 2), "interp_tile_i16_stereo": V("interp_tile", "int16", 2, **I16),
}
# what the launch logs must show, no more and no less: (the fields that name a kernel, the engine's width)
EXPECTED_KERNELS = {(k, w) for k in ("chain mode=0 NO=8", "chain mode=0 NO=32", "gather_wave", "gather", "tile", "tile_mfma", "chain mode=1 NO=8", "interp",
                                     "interp_wave", "interp_tile") for w in (4, 8)} | {("tile_mfma_p", 4), ("tile_mfma64_p", 8)}


def _jobs(oracle, vname):
    """the 24 jobs of a variant: every position class at every placement"""
    v = VARIANTS[vname]
    _, case, selector, n_out, _ = KERNELS[v["kernel"]]
    pl = oracle.plan(*case)
    # a loud job: white noise whose resampled copy has an RMS of about 13000 LSB (the filter keeps min(1, L / M) of its power), so
    # that about one output in a hundred lies beyond 2.5 sigma = full scale
    loud = int(13000 / min(1.0, pl.L / pl.M) ** 0.5) if v["loud"] else 0
    jobs = []
    for ci, cls in enumerate(wp.POSITIONS):
        k0, q = wp.position(pl.L, pl.M, pl.T, n_out, cls)
        for pi, how in enumerate(wp.PLACEMENTS):
            in_abs0, n_in, lead = wp.placement(pl.L, pl.M, pl.T, k0, n_out, how)
            jobs.append(dict(name="%s-%s-%s" % (vname, cls, how), variant=vname, cls=cls, how=how, case=list(case), dtype=v["dtype"], ch=v["ch"],
                             seed=7000 + 100 * sorted(VARIANTS).index(vname) + 10 * ci + pi, kernel=selector, k0=k0, n_out=n_out, in_abs0=in_abs0,
                             n_in=n_in, lead=lead, total=wp.span(pl.L, pl.M, pl.T, k0, n_out) + 5, q=q, loud=loud, dither=v["dither"],
                             dither_seed=v["dither_seed"], counter=v["counter"]))
    return jobs


@pytest.fixture(scope="module")
def results(oracle, tmp_path_factory):
    """environment -> the probe's results: one child process per environment, side by side"""
    assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
    tmp = tmp_path_factory.mktemp("window_positions")
    procs = {}
    for tag, extra in ENVS.items():
        jobs = [j for vname in VARIANTS if KERNELS[VARIANTS[vname]["kernel"]][4] == tag for j in _jobs(oracle, vname)]
        with open(tmp / (tag + ".json"), "w") as f:
            json.dump(jobs, f)
        env = {key: v for key, v in os.environ.items() if not key.startswith("HIPSOXR_")}
        env.update({"HIPSOXR_LIBRARY": DBG_LIB, "HIPSOXR_DEBUG_LAUNCH_LOG": str(tmp / (tag + ".log"))})
        env.update(extra)
        procs[tag] = subprocess.Popen([sys.executable, os.path.join(HERE, "_window_probe.py"), str(tmp / (tag + ".json")), str(tmp / (tag + ".npz"))], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    out = {}
    for tag, p in procs.items():
        try:
            _, err = p.communicate(timeout=300)
        finally:
            if p.poll() is None:
                p.kill()
        assert p.returncode == 0, (tag, err[-2000:])
        out[tag] = np.load(tmp / (tag + ".npz"))
    return out


def _line(log):
    """the one launch line of a run -> {field: value}"""
    lines = str(log).splitlines()
    assert len(lines) == 1, "one launch per run: %r" % str(log)
    f = dict(tok.split("=", 1) for tok in lines[0].split())
    return {k: (v if k in ("kernel", "io", "grid") else int(v)) for k, v in f.items()}


def _kernel_key(f):
    return f["kernel"] + (" mode=%d NO=%d" % (f["mode"], f["NO"]) if f["kernel"] == "chain" else "")


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_positions_are_what_they_are_called(oracle):
    """every job sits in its position class, its first output has a phase other than 0, its moved twin stays at non-negative
    input indices, and classes (e) and (f) of the L = 4800037 plan need the 128-bit product"""
    for vname in VARIANTS:
        for j in _jobs(oracle, vname):
            pl = oracle.plan(*j["case"])
            assert wp.class_holds(pl.L, pl.M, pl.T, j["k0"], j["n_out"], j["cls"]), j["name"]
            assert j["k0"] % pl.L != 0 and j["k0"] * pl.M % pl.L != 0 and wp.first_tap(pl.L, pl.M, pl.T, j["k0"]) % 4 == 0
            assert j["in_abs0"] - j["q"] * pl.M >= 0 and 0 < j["k0"] - j["q"] * pl.L < 4 * pl.L + 2 * pl.T * pl.L // pl.M
            assert j["in_abs0"] % 4 == {"exact": 0, "history5": 3, "late3": 3, "short2": 0}[j["how"]]
            if tuple(j["case"]) == INTERP_B and j["cls"] in wp.POSITIONS[3:]:  # (d): 2^62.07, the last a 64-bit product holds
                assert j["k0"] * pl.M > 2 ** (62 if j["cls"] == "d_2p40" else 63)
            if j["cls"] == "e_2p47":
                assert j["k0"] + j["n_out"] < 2 ** 48


def test_every_listed_kernel_served_every_position_class(oracle, results):
    """the (kernel, engine width) pairs of the launch logs are the list, exactly, and each was seen at every class (a)-(f)"""
    seen = {}
    for vname, v in VARIANTS.items():
        res = results[KERNELS[v["kernel"]][4]]
        for j in _jobs(oracle, vname):
            for tag in ("log_", "logs_"):
                f = _line(res[tag + j["name"]])
                seen.setdefault((_kernel_key(f), f["width"]), set()).add(j["cls"])
    assert set(seen) == EXPECTED_KERNELS, (sorted(set(seen) - EXPECTED_KERNELS), sorted(EXPECTED_KERNELS - set(seen)))
    assert all(classes == set(wp.POSITIONS) for classes in seen.values()), seen


@pytest.mark.parametrize("vname", list(VARIANTS))
def test_window_jobs_equal_the_oracle_and_their_moved_twins(oracle, results, vname):
    v = VARIANTS[vname]
    expect, case, _, n_out, env = KERNELS[v["kernel"]]
    res, pl, dtype, ch = results[env], oracle.plan(*case), v["dtype"], v["ch"]
    eng = oracle.engine_of(NPDT[dtype])
    real = np.float32 if eng == "f32" else np.float64
    differed = clipped = 0
    for j in _jobs(oracle, vname):
        name, k0, q = j["name"], j["k0"], j["q"]
        if j["how"] == "history5":
            print(name, "|", str(res["log_" + name]))
        # the launch log: this kernel, at these positions, both runs
        for tag, shift in (("log_", 0), ("logs_", q)):
            f = _line(res[tag + name])
            assert {k: f[k] for k in expect} == expect and f["width"] == WIDTH[dtype] and f["io"] == IO[dtype] and (f["L"], f["M"]) == (pl.L, pl.M), (name, f)
            if "k0" in f:  # (the gather family's lines)
                assert (f["k0"], f["in_abs0"], f["nf"], f["done"]) == (k0 - shift * pl.L, j["in_abs0"] - shift * pl.M, n_out, 0), (name, f)
        # guards and payload
        buf = res["y_" + name]
        assert buf.shape == (n_out + 2 * wp.GUARD, ch) and buf.dtype == NPDT[dtype]
        assert (buf[:wp.GUARD] == wp.POISON).all() and (buf[wp.GUARD + n_out:] == wp.POISON).all(), "a guard frame was written: " + name
        got = buf[wp.GUARD:wp.GUARD + n_out]
        assert bool(res["gs_" + name]), "the moved twin wrote a guard frame: " + name
        assert str(res["h_" + name]) == _sha(got)
        # the oracle at the job's own position; its output stage keyed at the job's and at the twin's
        x = wp.make_signal(dtype, j["total"], ch, j["seed"], j["loud"])[j["lead"]:j["lead"] + j["n_in"]]
        want, twin, n_clipped, n_clipped_twin = np.empty_like(got), np.empty_like(got), 0, 0
        for c in range(ch):
            y = oracle.resample_channel(pl, np.ascontiguousarray(x[:, c]).astype(real), "port_" + eng, k0=k0, n_out=n_out, in_abs0=j["in_abs0"])
            want[:, c], n = oracle.quantize(y, NPDT[dtype], channel=c, k0=k0, dither=j["dither"], seed=j["dither_seed"])
            twin[:, c], nt = oracle.quantize(y, NPDT[dtype], channel=c, k0=k0 - q * pl.L, dither=j["dither"], seed=j["dither_seed"])
            n_clipped, n_clipped_twin = n_clipped + n, n_clipped_twin + nt
        # (an int16 sample may equal the sentinel by right: an element counts as unwritten where the oracle says otherwise)
        unwritten = np.isnan(got) if got.dtype.kind == "f" else (got == wp.INT_SENT[dtype]) & (want != wp.INT_SENT[dtype])
        assert not unwritten.any(), "a payload element was not written: %s, first at %r" % (name, np.argwhere(unwritten)[0])
        bad = np.argwhere(got != want)
        assert bad.size == 0, "%s: %d elements differ from the oracle at k0 = %d, first at %r: %r against %r" % (
            name, len(bad), k0, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
        assert got.tobytes() == want.tobytes(), name  # (the sign of a zero too)
        # the same job moved down by q periods
        if j["dither"]:
            assert str(res["hs_" + name]) == _sha(twin), "the moved twin is not the oracle's output stage keyed at k0 - q L: " + name
            differed += str(res["hs_" + name]) != str(res["h_" + name])
        else:
            assert str(res["hs_" + name]) == str(res["h_" + name]), "moving the job by %d periods changed bits of the result: %s" % (q, name)
        if j["counter"]:
            assert list(res["clips_" + name]) == [n_clipped, n_clipped_twin], (name, list(res["clips_" + name]), n_clipped, n_clipped_twin)
            clipped += n_clipped
    if v["loud"]:  # over the variant's jobs: a few samples saturated, not most
        assert 0 < clipped < len(wp.POSITIONS) * len(wp.PLACEMENTS) * n_out * ch // 10, clipped
    if v["dither"]:
        assert differed == len(wp.POSITIONS) * len(wp.PLACEMENTS), "a dithered result equals its moved twin: the key ignores the position"
