"""GPU: ragged batches on the exact engine — a clip table (hipsoxr_job_t::clip_table) as ONE launch of a kernel's `bool
RAGGED` form (csrc/kernels_tile.h, k_gather; kernels.hip launch_ragged), where the parent ran one launch_job per clip.

All jobs run in ONE child process (tests/_ragged_exact_probe.py) on the debug-switch build, which writes one line per
ragged exact launch.  The probe makes the data (lengths are stated in units of Lc and of pb, which it reads from the launch
log) and returns every buffer as it lay in memory; everything is compared here.

Oracle 1 (bitwise): each clip of a ragged job equals the same clip run alone through device.resample_tensor(...,
kernel=KERNEL_EXACT) — or, for the 65 600-clip job, the clips of one length as one equal-length batch.
Oracle 2 (bitwise): the clips named per job equal oracle.resample(..., mode="port") on the plan's bank.
No tolerance is involved: every exact kernel computes the canonical order.
Launch count: the log holds exactly ONE line per job (the launches of the fold for more than 65535 columns), naming the
kernel and `ragged=<clips>` — the parent writes no line for these jobs, its results would pass.
Memory guard: every buffer is pre-filled with a sentinel; one spare frame lies behind every clip of the output (so between
clips and behind the last) and must keep it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DBG_LIB = os.path.join(os.path.dirname(HERE), "python-soxr_amd", "_variants", "dbg", "libhipsoxr.so")
SENTINEL = {"f32": 12345.0, "f64": 12345.0, "i32": 1234567, "i16": 12345}
NP = {"f32": np.float32, "f64": np.float64, "i32": np.int32, "i16": np.int16}
AUTO, GATHER, TILE_VALU, TILE_MFMA, EXACT = 0, 1, 3, 4, 6
EXACT_KERNELS = ("tile_mfma_p", "tile_mfma64_p", "tile_mfma", "tile", "gather")

TRIPLE = (16000, 48000, "QQ")   # planar, Lc 48 / Mc 16: slabs of at most 3072 outputs
HQ = (48000, 44100, "HQ")       # planar: k_tile_mfma_p (float32 engine), k_tile_mfma64_p (float64 engine)
DOWN = (44100, 16000, "HQ")     # Mc 441, no planes: k_tile_mfma
PRIME = (9973, 12289, "QQ")     # no tile tables: k_gather
INTERP = (48000, 44101, "HQ")   # interpolated-phase plan: still clip by clip

# a clip is [a, b, c, cut, t]: a pb Lc + b Lc + c + t BIG outputs wanted (BIG = max(16 Lc, 4096), AUTO's tile threshold),
# out_frames = that - cut.  {0, 1, Lc-1, pb Lc-1, pb Lc, pb Lc+1, 3 pb Lc+5}, one clip at the threshold, one truncated
# below out_len(in_frames); shuffled, the longest (clip 2) not last
TILE_SET = [[1, 0, 1, 0, 0], [0, 0, 1, 0, 0], [3, 0, 5, 0, 0], [0, 1, -1, 0, 0], [0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [0, 0, 0, 0, 1],
            [1, 0, -1, 0, 0], [0, 2, 3, 7, 0]]
TILE_CHECK = (1, 3, 7, 8)       # oracle 2 on the clips of 1, Lc - 1, pb Lc - 1 outputs and the truncated one
PRIME_SET = [[0, 0, 5000, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, 0], [0, 0, 5001, 3, 0], [0, 0, 700, 0, 0], [0, 0, 255, 0, 0], [0, 0, 257, 0, 0]]
WRAP = 65600

JOBS = {}  # name -> (job for the probe, {log field: value}, clips checked against oracle 2)


def _job(name, case, dtype, ch, clips, kernel=EXACT, expect=None, check=(), **kw):
    j = dict(name=name, case=list(case), dtype=dtype, ch=ch, clips=clips, kernel=kernel, seed=2000 + len(JOBS), solo="clip")
    j.update(kw)
    JOBS[name] = (j, expect or {}, tuple(check))


_PLANAR = {"f32": "tile_mfma_p", "i16": "tile_mfma_p", "f64": "tile_mfma64_p", "i32": "tile_mfma64_p"}
for _case, _tag in ((TRIPLE, "triple"), (HQ, "hq")):
    for _dt in ("f32", "f64"):
        for _ch in (1, 2):
            _job("tile_%s_%s_%d" % (_tag, _dt, _ch), _case, _dt, _ch, TILE_SET, expect=dict(kernel=_PLANAR[_dt], ragged=9),
                 check=TILE_CHECK if _ch == 1 or _tag == "hq" else ())
            _job("gather_%s_%s_%d" % (_tag, _dt, _ch), _case, _dt, _ch, TILE_SET, cap=True, expect=dict(kernel="gather", ragged=9),
                 check=(3, 8) if _ch == 2 else ())
# integers under the default selector (pinned to the canonical order): int16 with dither and a fixed seed
_job("tile_hq_i16_1_dither", HQ, "i16", 1, TILE_SET, kernel=AUTO, dither=True, dither_seed=5, expect=dict(kernel="tile_mfma_p", ragged=9), check=TILE_CHECK)
_job("tile_hq_i16_2", HQ, "i16", 2, TILE_SET, kernel=AUTO, expect=dict(kernel="tile_mfma_p", ragged=9), check=(3,))
_job("tile_hq_i32_1", HQ, "i32", 1, TILE_SET, kernel=AUTO, expect=dict(kernel="tile_mfma64_p", ragged=9), check=(3, 8))
_job("tile_triple_i32_2", TRIPLE, "i32", 2, TILE_SET, kernel=AUTO, expect=dict(kernel="tile_mfma64_p", ragged=9))
_job("gather_hq_i16_2_dither", HQ, "i16", 2, TILE_SET, kernel=AUTO, cap=True, dither=True, dither_seed=9, expect=dict(kernel="gather", ragged=9), check=(7,))
_job("gather_triple_i32_1", TRIPLE, "i32", 1, TILE_SET, kernel=AUTO, cap=True, expect=dict(kernel="gather", ragged=9), check=(3,))
# the general-period MFMA kernel
_job("down_f32_1", DOWN, "f32", 1, TILE_SET, expect=dict(kernel="tile_mfma", ragged=9, Mc=441), check=TILE_CHECK)
_job("down_f32_2", DOWN, "f32", 2, TILE_SET, kernel=TILE_MFMA, expect=dict(kernel="tile_mfma", ragged=9, Mc=441))
_job("down_f64_1", DOWN, "f64", 1, TILE_SET, expect=dict(kernel="tile_mfma", ragged=9, Mc=441), check=(3, 8))
_job("down_i16_2", DOWN, "i16", 2, TILE_SET, kernel=AUTO, dither=True, dither_seed=1, expect=dict(kernel="tile_mfma", ragged=9, Mc=441), check=(1,))
# the VALU tiles, by name
_job("valu_hq_f32_1", HQ, "f32", 1, TILE_SET, kernel=TILE_VALU, expect=dict(kernel="tile", ragged=9), check=(3, 8))
_job("valu_triple_f64_2", TRIPLE, "f64", 2, TILE_SET, kernel=TILE_VALU, expect=dict(kernel="tile", ragged=9))
_job("valu_down_i16_1", DOWN, "i16", 1, TILE_SET, kernel=TILE_VALU, expect=dict(kernel="tile", ragged=9))
# no tile tables
for _dt in ("f32", "f64", "i16"):
    _job("prime_" + _dt, PRIME, _dt, 1, PRIME_SET, kernel=AUTO if _dt == "i16" else EXACT, expect=dict(kernel="gather", ragged=7), check=(1, 3, 4))
_job("prime_split3_f32", PRIME, "f32", 3, PRIME_SET, layout="split", expect=dict(kernel="gather", ragged=7), check=(4,))
_job("gather_by_name_hq_f32_2", HQ, "f32", 2, TILE_SET, kernel=GATHER, pilot=EXACT, expect=dict(kernel="gather", ragged=9))
# layouts
_job("split3_hq_f32", HQ, "f32", 3, TILE_SET, layout="split", expect=dict(kernel="tile_mfma_p", ragged=9), check=(3, 8))
_job("split3_down_f64", DOWN, "f64", 3, TILE_SET, layout="split", expect=dict(kernel="tile_mfma", ragged=9))
_job("strided_hq_f64_2", HQ, "f64", 2, TILE_SET, layout="strided", expect=dict(kernel="tile_mfma64_p", ragged=9), check=(7,))
_job("strided_gather_hq_f32_1", HQ, "f32", 1, TILE_SET, cap=True, layout="strided", expect=dict(kernel="gather", ragged=9))
# clip offsets odd (scalar staging) and a multiple of 4 (16-byte loads): the same clips, the same bits
for _lay in ("odd", "al4"):
    _job("%s_hq_f32_1" % _lay, HQ, "f32", 1, TILE_SET, layout=_lay, seed=77, expect=dict(kernel="tile_mfma_p", ragged=9))
    _job("%s_hq_i16_1" % _lay, HQ, "i16", 1, TILE_SET, kernel=AUTO, layout=_lay, seed=78, expect=dict(kernel="tile_mfma_p", ragged=9))
    _job("%s_valu_hq_f64_1" % _lay, HQ, "f64", 1, TILE_SET, kernel=TILE_VALU, layout=_lay, seed=79, expect=dict(kernel="tile", ragged=9))
# an int16 job driven into clipping: the counter receives the sum of the per-clip counts
_job("counter_tile_hq_i16_2", HQ, "i16", 2, TILE_SET, kernel=AUTO, data="square", counter=True, expect=dict(kernel="tile_mfma_p", ragged=9))
_job("counter_gather_hq_i16_1", HQ, "i16", 1, TILE_SET, kernel=AUTO, cap=True, data="square", counter=True, expect=dict(kernel="gather", ragged=9))
# a caller's device copy of the table against the uploaded one: the same job twice
_job("tabledev_hq_f32_2", HQ, "f32", 2, TILE_SET, seed=JOBS["tile_hq_f32_2"][0]["seed"], table_dev=True, solo="none",
     expect=dict(kernel="tile_mfma_p", ragged=9))
# more columns than gridDim.y holds: 65 600 mono clips of 0 .. 5 input frames
_job("wrap", TRIPLE, "f32", 1, [[0, 0, 3 * (i % 6), 0, 0] for i in range(WRAP)], seed=91, solo="class")
# unchanged: an interpolated-phase plan is served clip by clip; a job the frequency-domain engine takes stays its one launch
_job("interp_f32_2", INTERP, "f32", 2, [[0, 0, 5000, 0, 0], [0, 0, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 9000, 5, 0]])
_job("fft_hq_f32_1", HQ, "f32", 1, [[0, 0, 20000, 0, 0], [0, 0, 1, 0, 0], [0, 0, 30001, 0, 0]], kernel=AUTO, solo="none")
TABLE_JOBS = list(JOBS)

PY_JOBS = [
    dict(kind="py_forward", name="py_forward", case=list(HQ), dtype="f32", ch=2, kernel=EXACT, seed=5, lengths=[5000, 1, 0, 30000, 777]),
    dict(kind="py_grad", name="py_grad", case=list(TRIPLE), seed=6, lengths=[9, 1, 14]),
    dict(kind="py_batch", name="py_batch", case=list(HQ), ch=1, seed=7, lengths=[3000, 12000, 1, 7000, 5, 9000, 20000], block_bytes=30000),
]

_child_failed = []  # a fault, abort or time limit in the child: nothing further is started on the GPU from this file


@pytest.fixture(autouse=True)
def _nothing_after_a_failed_child():
    if _child_failed:
        pytest.fail("the probe process failed (%s): no further GPU work from this file" % _child_failed[0])


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ragged_exact")
    assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
    with open(tmp / "jobs.json", "w") as f:
        json.dump([j for j, _, _ in JOBS.values()] + PY_JOBS, f)
    env = {key: v for key, v in os.environ.items() if not key.startswith("HIPSOXR_")}
    env.update({"HIPSOXR_LIBRARY": DBG_LIB, "HIPSOXR_DEBUG_LAUNCH_LOG": str(tmp / "launch.log")})
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "_ragged_exact_probe.py"), str(tmp / "jobs.json"), str(tmp / "out.npz")],
                           env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _child_failed.append("time limit")
        raise
    if r.returncode != 0:
        _child_failed.append("exit status %d" % r.returncode)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(tmp / "out.npz")


def _lines(log):
    return [dict(tok.split("=", 1) for tok in ln.split()) for ln in str(log).split("\n") if ln.strip()]


def _exact_lines(log):
    """the ragged exact launches among the lines (an equal-length tile launch writes the same line without ragged=)"""
    return [f for f in _lines(log) if f.get("kernel") in EXACT_KERNELS and "ragged" in f]


def _bits(a):
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.itemsize])


def _clips(name, res):
    """memory guard checked; -> [(x [n_in, ch], y [out_frames, ch])] per clip, from the buffers as they lay in memory"""
    job = JOBS[name][0]
    ch, table = job["ch"], res["table_" + name]
    _, _, _, xf, xc, yf, yc = (int(v) for v in res["geom_" + name])
    x, y = res["x_" + name], res["y_" + name]
    assert y.dtype == NP[job["dtype"]]
    written = np.zeros(y.shape, bool)
    out = []
    for x0, n_in, y0, n_out in table:
        xi = x0 + np.arange(n_in)[:, None] * xf + np.arange(ch)[None, :] * xc
        yi = y0 + np.arange(n_out)[:, None] * yf + np.arange(ch)[None, :] * yc
        assert not written[yi].any(), "the test's clips overlap"
        written[yi] = True
        out.append((x[xi], y[yi]))
    spare = y[~written]
    assert spare.size == ch * len(table), "one spare frame behind every clip"
    assert np.all(spare == SENTINEL[job["dtype"]]), "an element between packed clips (or behind the last) was written"
    return out


def _solo(name, res):
    ch, table, flat = JOBS[name][0]["ch"], res["table_" + name], res["solo_" + name]
    out, pos = [], 0
    for n in table[:, 3]:
        out.append(flat[pos:pos + n * ch].reshape(n, ch))
        pos += n * ch
    assert pos == flat.size
    return out


@pytest.mark.parametrize("name", [n for n in TABLE_JOBS if JOBS[n][1]])
def test_one_launch_of_the_expected_kernel(name, results):
    """exactly ONE log line per job: the kernel family, ragged=<clips>, a grid of the longest clip over all columns"""
    job, expect, _ = JOBS[name]
    lines = _lines(results["log_" + name])
    assert len(lines) == 1, "one launch per ragged job: %r" % str(results["log_" + name])
    f = lines[0]
    for key, v in expect.items():
        assert f[key] == str(v), (key, f)
    lc, pb, big = (int(v) for v in results["geom_" + name][:3])
    table = results["table_" + name]
    gx, gy, gz = (int(v) for v in f["grid"].split("x"))
    if f["kernel"] == "gather":
        assert int(table[:, 3].max()) < big or job["kernel"] == GATHER or lc == 0
        ch_fast = job["ch"] > 1 and job.get("layout", "packed") != "split"
        assert (gx, gy) == (-(-int(table[:, 3].max()) * (job["ch"] if ch_fast else 1) // 256), len(table) if ch_fast else len(table) * job["ch"])
    else:
        assert (int(f["Lc"]), int(f["pb"])) == (lc, pb) and int(table[:, 3].max()) >= big
        slabs = -(-(-(-int(table[:, 3].max()) // lc)) // pb)
        split = int(f["split"])
        assert gy == len(table) * job["ch"] and gx * gz in (slabs * split, -(-slabs // 8) * 8 * split)
        # the lengths the job was to have: around the period and the slab, one at AUTO's threshold
        want = sorted(int(v) for v in table[:, 3])
        assert want == sorted([0, 1, lc - 1, pb * lc - 1, pb * lc, pb * lc + 1, 3 * pb * lc + 5, big, 2 * lc + 3 - 7])
        assert int(table[-1, 3]) != want[-1], "the longest clip is not the last"


@pytest.mark.parametrize("name", [n for n in TABLE_JOBS if JOBS[n][0]["solo"] == "clip"])
def test_every_clip_equals_the_clip_run_alone(name, results):
    """bitwise; every element of every clip written, nothing between the clips"""
    got, solo = _clips(name, results), _solo(name, results)
    for c, ((_, y), s) in enumerate(zip(got, solo)):
        assert y.shape == s.shape
        assert np.array_equal(_bits(np.ascontiguousarray(y)), _bits(np.ascontiguousarray(s))), "%s clip %d of %d frames" % (name, c, len(y))


@pytest.mark.parametrize("name", [n for n in TABLE_JOBS if JOBS[n][2]])
def test_named_clips_equal_the_oracle(name, results, oracle):
    """bitwise against the oracle's canonical order on the plan's bank (conversion, dither and all)"""
    job, _, check = JOBS[name]
    got = _clips(name, results)
    for c in check:
        x, y = got[c]
        want = oracle.resample(np.ascontiguousarray(x), *job["case"], mode="port", dither=job.get("dither", False), seed=job.get("dither_seed", 0))
        assert len(want) >= len(y) and len(y) > 0
        assert np.array_equal(_bits(np.ascontiguousarray(y)), _bits(np.ascontiguousarray(want[:len(y)]))), "%s clip %d" % (name, c)


@pytest.mark.parametrize("tag", ["hq_f32_1", "hq_i16_1", "valu_hq_f64_1"])
def test_odd_offsets_give_the_bits_of_aligned_ones(tag, results):
    """a clip whose offset is no multiple of 4 elements takes the scalar staging path: the same clips, the same results"""
    odd, al4 = _clips("odd_" + tag, results), _clips("al4_" + tag, results)
    assert all(int(r[0]) % 2 == 1 for r in results["table_odd_" + tag] if r[1]) and all(int(r[0]) % 4 == 0 for r in results["table_al4_" + tag])
    for (xo, yo), (xa, ya) in zip(odd, al4):
        assert np.array_equal(xo, xa) and np.array_equal(_bits(np.ascontiguousarray(yo)), _bits(np.ascontiguousarray(ya)))


@pytest.mark.parametrize("name", ["counter_tile_hq_i16_2", "counter_gather_hq_i16_1"])
def test_clip_counter_is_the_sum_over_clips(name, results):
    ragged, solo = (int(v) for v in results["count_" + name])
    assert solo > 0, "the test's data does not clip"
    assert ragged == solo


def test_callers_table_gives_the_uploaded_tables_bits(results):
    assert np.array_equal(results["table_tabledev_hq_f32_2"], results["table_tile_hq_f32_2"])
    assert np.array_equal(_bits(results["y_tabledev_hq_f32_2"]), _bits(results["y_tile_hq_f32_2"]))


def test_column_fold(results):
    """65 600 mono clips: the launches of the fold, all k_gather, over ranges that partition the clips"""
    lines = _lines(results["log_wrap"])
    assert [f["kernel"] for f in lines] == ["gather", "gather"]
    assert [int(f["ragged"]) for f in lines] == [65535, WRAP - 65535]
    assert [int(f["grid"].split("x")[1]) for f in lines] == [65535, WRAP - 65535]
    got, solo = _clips("wrap", results), _solo("wrap", results)
    assert sorted(set(len(y) for _, y in got)) == [0, 3, 6, 9, 12, 15]
    assert all(np.array_equal(_bits(np.ascontiguousarray(y)), _bits(np.ascontiguousarray(s))) for (_, y), s in zip(got, solo))


def test_interpolated_phase_plans_are_still_served_clip_by_clip(results):
    assert _exact_lines(results["log_interp_f32_2"]) == []   # (its results: test_every_clip_equals_the_clip_run_alone)
    assert len(_clips("interp_f32_2", results)) == 4


def test_the_frequency_domain_engine_still_takes_its_jobs(results):
    lines = _lines(results["log_fft_hq_f32_1"])
    assert len(lines) == 1 and lines[0].get("form") == "pair2" and "kernel" not in lines[0], lines


def test_resample_ragged_forward_is_one_launch_with_the_per_clip_bits(results):
    lines = _lines(results["log_py_forward"])
    assert len(lines) == 1 and lines[0]["kernel"] == "tile_mfma_p" and lines[0]["ragged"] == "5", lines
    assert np.array_equal(_bits(results["y_py_forward"]), _bits(results["solo_py_forward"]))


def test_resample_ragged_gradcheck_and_double_backward(results):
    assert bool(results["gradcheck_py_grad"])
    lines = _exact_lines(results["log_py_grad"])
    assert len(lines) == 1 and lines[0]["ragged"] == "3", "the double backward is one ragged exact launch: %r" % str(results["log_py_grad"])
    assert np.array_equal(_bits(results["ggw_py_grad"]), _bits(results["ggw_want_py_grad"]))


def test_resample_batch_host_corpus_one_launch_per_block(results, soxr):
    blocks = [int(b) for b in results["blocks_py_batch"]]
    assert len(blocks) >= 3
    lines = _lines(results["log_py_batch"])
    assert [f.get("kernel") in EXACT_KERNELS for f in lines] == [True] * len(blocks), lines
    assert [int(f["ragged"]) for f in lines] == blocks
    job = PY_JOBS[2]
    x, y, xp, yp = results["x_py_batch"], results["y_py_batch"], 0, 0
    assert y.dtype == np.int16
    for n in job["lengths"]:
        want = soxr.resample(x[xp:xp + n], job["case"][0], job["case"][1], job["case"][2]) if n else np.zeros(0, np.int16)
        assert np.array_equal(y[yp:yp + len(want)], want), n
        xp, yp = xp + n, yp + len(want)
    assert yp == len(y)
