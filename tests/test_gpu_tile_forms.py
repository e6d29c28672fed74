"""GPU: every launch form of the exact engine's tile kernels (csrc/kernels.hip, launch_tile) against the oracle.

launch_tile decides (csrc/tile_rules.h): the slab size of the planar kernels (float32: 64 or 32 periods, float64: 32 or 16) and
their unit split, as XCD-aware 1-D ids or on grid.z; the small form (16-period slabs, half-chains on two waves), the mid form
(16-period slabs) and the plan's own slab of the general-period kernel; the waves of a workgroup; the row-tile split over
grid.z.  The debug-switch build writes one line per tile launch (HIPSOXR_DEBUG_LAUNCH_LOG), so a case here names the fields its
launch must show and the test reads them from the log — the rules are not restated.  The switches are read once per process,
so the jobs run in three child processes (tests/_tile_forms_probe.py), started together: every case under the rules as they
are; every case again under the REFERENCE form (the plan's own slab, no half-chains, no row-tile split, 32-period float64
slabs, plain grid.z); and the XCD case under HIPSOXR_NO_XCD_SPLIT alone.

Per case: the log line's fields; windows of 256 outputs at the first and last outputs, across a slab boundary and at three
random places against the oracle's canonical-order port (port_f32 / port_f64, integer types through the oracle's output
stage), bit for bit, every channel; the whole result against the reference form's, bit for bit (SHA-256 of its bytes).  Each
case has a small size at which the rules give its form — found with the header's functions in a scratch program; where a form
holds from the 4096-output threshold of the tile family on, a size of several slabs with a partial last one.  A case is
resized, never its assertion changed, if a later launch rule moves it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _tile_forms_probe import make_input  # noqa: E402

DBG_LIB = os.path.join(os.path.dirname(HERE), "python-soxr_amd", "_variants", "dbg", "libhipsoxr.so")
EXACT, TILE_VALU = 6, 3
W = 256
TILE_KERNELS = ("tile", "tile_mfma", "tile_mfma_p", "tile_mfma64_p")
NPDT = {"float32": np.float32, "float64": np.float64, "int16": np.int16, "int32": np.int32}
IO = {"float32": "f32", "float64": "f64", "int16": "i16", "int32": "i32"}

PLANAR = (48000, 44100, "VHQ")   # Lc 147, Mc 160, 10 row tiles: k_tile_mfma_p (float32 engine), k_tile_mfma64_p (float64 engine)
GENERAL = (44100, 16000, "VHQ")  # Lc 160, Mc 441: no planes, k_tile_mfma; a float32 slab is 64 periods, a float64 one 32
WIDE = (32000, 44100, "VHQ")     # Lc 441, 28 row tiles: more than a workgroup has waves
REFERENCE_ENV = {"HIPSOXR_DEBUG_SLAB64": "1", "HIPSOXR_DEBUG_NO_HALVES": "1", "HIPSOXR_NO_TILE_SPLIT": "1", "HIPSOXR_DEBUG_MFMA64_PB": "32", "HIPSOXR_NO_XCD_SPLIT": "1"}

# name -> (plan, dtype, frames, channels, selector, {log field: value}, {log field of the reference form's line: value}, extras)
FORMS = {
    # float32 planar kernel: slabs of 64 periods over all columns decide (planes_form).  32 split: from the family's threshold on
    # (60000 frames: 12 slabs of 32, the last partial); 64 split: from 47 slabs of 64 (2 x 215041 frames: 2 x 22 slabs is the first
    # stereo size); 32 whole: from 2 x 107 slabs of 64; 64 whole: from 2 x 253 (the 512-slab rule of the comment)
    "p32_split": (PLANAR, "float32", 60000, 1, EXACT, dict(kernel="tile_mfma_p", pb=32, split=3, xz=3, gz=1, nw=4), dict(pb=64, split=5, xz=0, gz=5), {}),
    "p64_split": (PLANAR, "float32", 215041, 2, EXACT, dict(kernel="tile_mfma_p", pb=64, split=5, xz=5, gz=1), dict(pb=64, xz=0, gz=5), {}),
    "p32_whole": (PLANAR, "float32", 1090561, 2, EXACT, dict(kernel="tile_mfma_p", pb=32, split=1, xz=0, gz=1), dict(pb=64, split=5), {}),
    "p64_whole": (PLANAR, "float32", 2585601, 2, EXACT, dict(kernel="tile_mfma_p", pb=64, split=1, xz=0, gz=1), dict(pb=64, xz=0), {}),
    # float64 planar kernel (float64 and int32 io): 16-period slabs below 1536 slabs of 32, split below 512 workgroups (2 x 256
    # slabs of 16: 2 x 652801 frames is the first whole one); 32-period slabs from 2 x 768 on, always whole.  32-period slabs
    # WITH a unit split are no form of an equal-length job (1536 slabs are more than 512 workgroups): the reference form's run
    # of the small job shows it, forced by HIPSOXR_DEBUG_MFMA64_PB=32
    "p16_split_f64": (PLANAR, "float64", 60000, 1, EXACT, dict(kernel="tile_mfma64_p", width=8, pb=16, split=3, xz=3, gz=1), dict(pb=32, split=3, xz=0, gz=3), {}),
    "p16_whole_i32": (PLANAR, "int32", 652801, 2, EXACT, dict(kernel="tile_mfma64_p", width=8, pb=16, split=1, xz=0, gz=1), dict(pb=32, split=3, gz=3), {}),
    "p32_whole_f64": (PLANAR, "float64", 3927041, 2, EXACT, dict(kernel="tile_mfma64_p", width=8, pb=32, split=1, xz=0, gz=1), dict(pb=32, split=1), {}),
    # general-period kernel.  Small form (up to 96 slabs of 64 periods): half-chains on two waves; below 128 workgroups the row
    # tiles are split as well (30011 frames: 5 slabs of 16, one row tile = two waves per workgroup, grid.z 10); from 128
    # workgroups on 5 row tiles per workgroup (2 x 296354 frames: 2 x 43 slabs of 16).  Mid form: 16-period slabs, whole row
    # tiles, from 97 slabs of 64 (float32: 2 x 49) resp. 129 (float64: 2 x 65); the plan's own slab where that fills the chip's
    # layers as well (float32: from 193 slabs of 64; float64, slabs of 32: at 2 x 97)
    "g_halves_split_f32": (GENERAL, "float32", 30011, 1, EXACT, dict(kernel="tile_mfma", pb=16, halves=1, nw=2, split=10, gz=10, block=256), dict(pb=64, halves=0, gz=1, nw=10), {}),
    "g_halves_f32": (GENERAL, "float32", 296354, 2, EXACT, dict(kernel="tile_mfma", pb=16, halves=1, nw=10, split=2, gz=2, block=640), dict(pb=64, halves=0, gz=1), {}),
    "g_mid_f32": (GENERAL, "float32", 1354754, 2, EXACT, dict(kernel="tile_mfma", pb=16, halves=0, nw=10, split=1, gz=1), dict(pb=64, halves=0), {}),
    "g_own_f32": (GENERAL, "float32", 2709506, 2, EXACT, dict(kernel="tile_mfma", pb=64, halves=0, nw=10, split=1, gz=1), dict(pb=64, halves=0), {}),
    "g_halves_split_f64": (GENERAL, "float64", 30011, 1, EXACT, dict(kernel="tile_mfma", width=8, pb=16, halves=1, nw=2, split=10, gz=10), dict(pb=32, halves=0, gz=1), {}),
    "g_halves_f64": (GENERAL, "float64", 296354, 2, EXACT, dict(kernel="tile_mfma", width=8, pb=16, halves=1, nw=10, split=2, gz=2), dict(pb=32, halves=0, gz=1), {}),
    "g_mid_f64": (GENERAL, "float64", 1806338, 2, EXACT, dict(kernel="tile_mfma", width=8, pb=16, halves=0, split=1, gz=1), dict(pb=32, halves=0), {}),
    "g_own_f64": (GENERAL, "float64", 1354754, 2, EXACT, dict(kernel="tile_mfma", width=8, pb=32, halves=0, split=1, gz=1), dict(pb=32, halves=0), {}),
    # k_tile by selector: aligned (Mc 160) and unaligned (Mc 441) staging, 28 row tiles on 14 waves, whole from 128 workgroups
    # on (8 columns x 16 slabs of 64); below that the row tiles of a slab go to grid.z workgroups (20000 frames: 2 slabs)
    "valu_aligned": (PLANAR, "float32", 153601, 8, TILE_VALU, dict(kernel="tile", pb=64, n_rt=10, nw=10, split=1, gz=1, block=640), dict(gz=1), {}),
    "valu_unaligned": (GENERAL, "float32", 423362, 8, TILE_VALU, dict(kernel="tile", pb=64, n_rt=10, nw=10, split=1, gz=1), dict(gz=1), {}),
    "valu_unaligned_i32": (GENERAL, "int32", 211682, 8, TILE_VALU, dict(kernel="tile", width=8, pb=32, nw=10, split=1, gz=1), dict(gz=1), {}),
    "valu_28_row_tiles": (WIDE, "float32", 307201, 8, TILE_VALU, dict(kernel="tile", pb=64, n_rt=28, nw=14, split=1, gz=1, block=896), dict(gz=1), {}),
    "valu_split": (PLANAR, "float32", 20000, 1, TILE_VALU, dict(kernel="tile", pb=64, nw=1, split=10, gz=10, block=256), dict(nw=10, split=1, gz=1, block=640), {}),
    # a window job through Plan.run: outputs [100000, 183750) — the first period is 680, inside a slab of the whole signal
    "window_k0": (PLANAR, "float32", 200000, 1, EXACT, dict(kernel="tile_mfma_p", pb=32, split=3, xz=3, gx=72), dict(pb=64), dict(k0=100000)),
    # int16 with dither on a planar and a general-period form
    "p32_split_i16_dither": (PLANAR, "int16", 60000, 1, EXACT, dict(kernel="tile_mfma_p", io="i16", pb=32, split=3, xz=3), dict(pb=64), dict(dither=True, dither_seed=11)),
    "g_halves_i16_dither": (GENERAL, "int16", 30011, 1, EXACT, dict(kernel="tile_mfma", io="i16", pb=16, halves=1, gz=10), dict(pb=64, halves=0), dict(dither=True, dither_seed=12)),
}
XCD_CASE = "p32_split"  # ... and under HIPSOXR_NO_XCD_SPLIT alone: the same slabs and split on grid.z


def _parse(line):
    """one tile launch line -> {field: value}; grid=XxYxZ becomes gx, gy, gz"""
    f = dict(tok.split("=", 1) for tok in line.split())
    out = {k: (v if k in ("kernel", "io") else int(v)) for k, v in f.items() if k != "grid"}
    out["gx"], out["gy"], out["gz"] = (int(v) for v in f["grid"].split("x"))
    return out


def _tile_lines(log):
    """the equal-length tile launches among a job's log lines"""
    return [_parse(ln) for ln in str(log).splitlines() if ln.split(" ", 1)[0][len("kernel="):] in TILE_KERNELS and "ragged=" not in ln]


def _windows(oracle, name):
    """[first output, count] of the windows a case is compared on, relative to its first output: the ends, a slab boundary, three others"""
    case, dtype, frames, ch, _, expect, _, extra = FORMS[name]
    pl = oracle.plan(*case)
    k0 = extra.get("k0", 0)
    n = pl.out_len(frames) - k0
    Lc, slab = pl.L, expect["pb"] * pl.L  # (L >= 16 in these plans: a period is not replicated)
    blocks = ((k0 + n - 1) // Lc - k0 // Lc) // expect["pb"] + 1
    edge = (k0 // Lc) * Lc + max(1, blocks // 2) * slab - k0  # first output of a slab in the middle of the job
    rng = np.random.default_rng(len(name) * 1000 + frames)
    firsts = [0, n - W, edge - W // 2] + [int(v) for v in rng.integers(0, n - W, 3)]
    assert 0 < edge - W // 2 and edge + W // 2 < n, (name, edge, n)
    return [[a, W] for a in firsts]


def _spawn(tmp, tag, names, oracle, env_extra):
    jobs = []
    for i, n in enumerate(names):
        case, dtype, frames, ch, kernel, _, _, extra = FORMS[n]
        jobs.append(dict(name=n, case=list(case), dtype=dtype, frames=frames, ch=ch, seed=400 + list(FORMS).index(n), kernel=kernel, dither=extra.get("dither", False),
                         dither_seed=extra.get("dither_seed", 0), k0=extra.get("k0", 0), windows=_windows(oracle, n) if tag == "rules" else []))
    with open(tmp / (tag + ".json"), "w") as f:
        json.dump(jobs, f)
    env = {key: v for key, v in os.environ.items() if not key.startswith("HIPSOXR_")}
    env.update({"HIPSOXR_LIBRARY": DBG_LIB, "HIPSOXR_DEBUG_LAUNCH_LOG": str(tmp / (tag + ".log"))})
    env.update(env_extra)
    return subprocess.Popen([sys.executable, os.path.join(HERE, "_tile_forms_probe.py"), str(tmp / (tag + ".json")), str(tmp / (tag + ".npz"))], env=env,
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


@pytest.fixture(scope="module")
def results(oracle, tmp_path_factory):
    """tag -> the probe's results: three child processes for the whole file, side by side"""
    assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
    tmp = tmp_path_factory.mktemp("tile_forms")
    procs = {"rules": _spawn(tmp, "rules", list(FORMS), oracle, {}), "reference": _spawn(tmp, "reference", list(FORMS), oracle, REFERENCE_ENV),
             "no_xcd": _spawn(tmp, "no_xcd", [XCD_CASE], oracle, {"HIPSOXR_NO_XCD_SPLIT": "1"})}
    out = {}
    for tag, p in procs.items():
        try:
            _, err = p.communicate(timeout=600)
        finally:
            if p.poll() is None:
                p.kill()
        assert p.returncode == 0, (tag, err[-2000:])
        out[tag] = np.load(tmp / (tag + ".npz"))
    return out


def _one_line(res, name):
    lines = _tile_lines(res["log_" + name])
    assert len(lines) == 1, "one tile launch per job: %r" % str(res["log_" + name])
    return lines[0]


def _check_line(f, case_plan, dtype, ch, n_out, k0=0):
    """what every tile line shows, whatever its form"""
    assert f["kernel"] in TILE_KERNELS and f["io"] == IO[dtype] and f["width"] == (4 if dtype in ("float32", "int16") else 8)
    assert (f["L"], f["M"]) == (case_plan.L, case_plan.M) and f["Lc"] == case_plan.L and f["gy"] == ch
    blocks = ((k0 + n_out - 1) // f["Lc"] - k0 // f["Lc"]) // f["pb"] + 1
    if f["xz"]:
        assert f["xz"] == f["split"] > 1 and f["gz"] == 1 and f["gx"] == -(-blocks // 8) * 8 * f["split"]
    else:
        assert f["gx"] == blocks and f["gz"] == f["split"]
    assert 1 <= f["nw"] <= 16 and f["block"] <= 1024 and f["block"] == (64 * f["nw"] if f["split"] == 1 or f["kernel"] in TILE_KERNELS[2:] else max(256, 64 * f["nw"]))
    assert f["lds"] <= 160 * 1024 and f["halves"] in (0, 1) and (not f["halves"] or f["kernel"] == "tile_mfma")


@pytest.mark.parametrize("name", list(FORMS))
def test_form_oracle_and_reference_form(oracle, results, name):
    case, dtype, frames, ch, _, expect, expect_ref, extra = FORMS[name]
    res, ref = results["rules"], results["reference"]
    pl = oracle.plan(*case)
    k0 = extra.get("k0", 0)
    n_out = pl.out_len(frames) - k0
    assert tuple(res["shape_" + name]) == (n_out, ch) == tuple(ref["shape_" + name])
    f, fr = _one_line(res, name), _one_line(ref, name)
    print(name, "rules:", str(res["log_" + name]), "| reference form:", str(ref["log_" + name]))
    _check_line(f, pl, dtype, ch, n_out, k0)
    _check_line(fr, pl, dtype, ch, n_out, k0)
    assert {k: f[k] for k in expect} == expect, f
    assert fr["kernel"] == f["kernel"] and fr["halves"] == 0 and fr["xz"] == 0 and {k: fr[k] for k in expect_ref} == expect_ref, fr
    # windows against the canonical-order port, every channel
    x = make_input(dtype, frames, ch, 400 + list(FORMS).index(name))
    eng = oracle.engine_of(NPDT[dtype])
    real = np.float32 if eng == "f32" else np.float64
    got = res["w_" + name]
    assert got.shape == (6 * W, ch) and got.dtype == NPDT[dtype]
    for i, (a, n) in enumerate(_windows(oracle, name)):
        for c in range(ch):
            v = oracle.resample_channel(pl, np.ascontiguousarray(x[:, c]).astype(real), "port_" + eng, k0=k0 + a, n_out=n)
            want, _ = oracle.quantize(v, NPDT[dtype], channel=c, k0=k0 + a, dither=extra.get("dither", False), seed=extra.get("dither_seed", 0))
            assert np.array_equal(got[i * W:(i + 1) * W, c], want), (name, a, c)
    # the whole result against the reference form's
    assert str(res["h_" + name]) == str(ref["h_" + name]), "the form changed bits of the result"


def test_unit_split_on_grid_z_without_xcd_ids(oracle, results):
    """the XCD case under HIPSOXR_NO_XCD_SPLIT: the same slab size and split, on grid.z, the same bits"""
    case, dtype, frames, ch, _, expect, _, _ = FORMS[XCD_CASE]
    pl = oracle.plan(*case)
    f, fz = _one_line(results["rules"], XCD_CASE), _one_line(results["no_xcd"], XCD_CASE)
    _check_line(fz, pl, dtype, ch, pl.out_len(frames))
    assert f["xz"] > 1 and fz["xz"] == 0 and fz["gz"] == f["split"] == fz["split"] > 1 and fz["pb"] == f["pb"] and fz["gx"] * 8 >= f["gx"] // f["split"] >= fz["gx"]
    assert str(results["no_xcd"]["h_" + XCD_CASE]) == str(results["rules"]["h_" + XCD_CASE])
