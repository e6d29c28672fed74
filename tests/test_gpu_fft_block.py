"""k_fft_block (csrc/fft.hip), the general path of the frequency-domain engine — what HIPSOXR_KERNEL_AUTO gives every
float32 HQ / VHQ job of 2^13 outputs whose ratio is 7-smooth and outside the paired-kernel schedule table — on every
instance of fft_pass<R, SIGN, NB> that run_passes dispatches to, in both directions, by name in the launch log, against
the float64 oracle.  The plan is tests/_block_probe.py's (held to its conditions by tests/test_fft_block_plan.py); three
child processes run it under the debug-switch build: `plain` (no switch but the launch log: the product's own choice, the
small geometry variant), `large` (HIPSOXR_FFT_LARGE_ONLY: the other variant of the ratios where it differs) and `nopair`
(HIPSOXR_FFT_NO_PAIR: tabled ratios on k_fft_block — the same jobs run on the paired kernels in `plain`).

Per job.  LAUNCH LOG: exactly one line, form=block, the case's L, M and kind=f32, and k, hop_out, LDS bytes, n_blocks and
grid (n_blocks x columns) as the Python restatement of fft_geometry says — which ties the restatement, and so the claimed
instance coverage, to what the product chose.  MEMORY: the input is a view inside a NaN-filled tensor (8 frames either
side; beside a channel slice the other channels too), the output a NaN-prefilled view inside a buffer of 12345.0: every
guard intact, no NaN left, two runs the same bytes.  VALUES: every column against oracle.resample(mode="ref"), the
float64 direct form on the oracle's own bank, at the bars of tests/test_gpu_fft.py: relative RMS <= 1e-6, worst point <=
4e-5 x RMS of the column.  The `nopair` results also lie within 1e-6 relative RMS of the paired kernels' on the same job.

Jobs per case: exactly one block's kept run, one output more, and two runs plus a seeded remainder (first, interior,
partial last block; 2^13 outputs and more where the job goes through KERNEL_AUTO); mono and a (2, n, 3) interleaved
batch; on one up- and one down-sampling ratio also a (3, n, 1) planar batch, the channel slice [:, :, 1:3] of five
channels as input and as out=, and a planar batch of unit impulses at 16 consecutive input positions of the interior block
(both parities of the (re, im) = (2n, 2n + 1) packing: a misplaced element shows at full scale).
Measured figures and two mutation runs: profiles/NOTES_fft_block.md."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import _block_probe as bp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DBG_LIB = os.path.join(os.path.dirname(HERE), "python-soxr_amd", "_variants", "dbg", "libhipsoxr.so")
REL_BAR, POINT_BAR = 1e-6, 4e-5           # tests/test_gpu_fft.py
PAIRED_FORMS = ("pair2", "strided2_cp", "strided2_st")


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


@pytest.fixture(scope="module")
def planned():
    """The parsed instances, every job, the geometry per (case, child), the inputs and one reference per distinct column."""
    from oracle import oracle as o
    parsed = bp.parse_run_passes()
    jobs, geoms = bp.all_jobs(parsed, lambda r, q: o.plan(r[0], r[1], q))
    inputs, refs, cache = {}, {}, {}
    for j in jobs:
        key = (j["case"], "nopair" if j["name"].startswith("twin__") else j["child"])
        x = bp.signal(j, geoms[key]["hop_out"])
        inputs[j["name"]] = x
        cols = []
        for c in range(x.shape[0]):
            ck = (j["rates"][0], j["rates"][1], j["quality"], j["n_in"], j["signal"], c)
            if ck not in cache:
                cache[ck] = o.resample(x[c], j["rates"][0], j["rates"][1], j["quality"], mode="ref")
            cols.append(cache[ck])
        refs[j["name"]] = cols
    return dict(parsed=parsed, jobs=jobs, geoms=geoms, inputs=inputs, refs=refs)


@pytest.fixture(scope="module")
def results(planned, tmp_path_factory):
    """child -> the probe's results (one process per switch setting)."""
    assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
    tmp = tmp_path_factory.mktemp("fft_block")
    got, t0 = {}, time.time()
    for child, switches in bp.CHILDREN.items():
        mine = [j for j in planned["jobs"] if j["child"] == child]
        data = {"x_" + j["name"]: planned["inputs"][j["name"]] for j in mine}
        data["meta"] = np.array(json.dumps(mine))
        np.savez(tmp / f"jobs_{child}.npz", **data)
        env = {key: v for key, v in os.environ.items() if not key.startswith("HIPSOXR_")}
        env.update(switches)
        env.update({"HIPSOXR_LIBRARY": DBG_LIB, "HIPSOXR_DEBUG_LAUNCH_LOG": str(tmp / f"launch_{child}.log")})
        r = subprocess.run([sys.executable, os.path.join(HERE, "_block_probe.py"), "CHILD", str(tmp / f"jobs_{child}.npz"), str(tmp / f"results_{child}.npz")],
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (child, r.stdout[-1000:], r.stderr[-2000:])
        got[child] = dict(np.load(tmp / f"results_{child}.npz"))
    got["seconds"] = time.time() - t0
    return got


def _check_job(j, planned, results, fails, figs):
    """One job against its conditions; what fails goes to `fails`, the figures of its columns to `figs`."""
    name, res = j["name"], results[j["child"]]
    tag = f"{j['tag']}/{j['layout']}"
    if "err_" + name in res:
        fails.append(f"{tag}: raised: {res['err_' + name]}")
        return None
    if "y_" + name not in res:
        fails.append(f"{tag}: not run (the child stopped at an earlier error)")
        return None
    clips, ch, ch_all, _ = bp.LAYOUTS[j["layout"]]
    # ---- the launch log
    lines = json.loads(str(res["log_" + name]))
    if len(lines) != 1:
        fails.append(f"{tag}: {len(lines)} launch log lines: {lines}")
    elif j["log"] is None:
        if lines[0].get("form") not in PAIRED_FORMS:
            fails.append(f"{tag}: the twin job was served by {lines[0]}")
    else:
        w = j["log"]
        want = dict(form="block", L=str(j["L"]), M=str(j["M"]), kind="f32", k=str(w["k"]), small="-1", nt=str(bp.NT), lds=str(w["lds"]),
                    grid="%dx%dx1" % (w["n_blocks"], clips * ch), hop_out=str(w["hop_out"]), n_blocks=str(w["n_blocks"]), window="0")
        bad = {f: (lines[0].get(f), v) for f, v in want.items() if lines[0].get(f) != v}
        if bad:
            fails.append(f"{tag}: launch log (got, planned) {bad}")
    # ---- memory
    buf = res["y_" + name]
    if buf.shape != (clips, j["n_out"] + 2 * bp.GUARD, ch_all):
        fails.append(f"{tag}: buffer shape {buf.shape}")
        return None
    idx = bp.payload(j["layout"], j["n_out"])
    outside = buf.copy()
    outside[idx] = bp.POISON
    if not np.all(outside == bp.POISON):
        fails.append(f"{tag}: {int(np.count_nonzero(outside != bp.POISON))} guard elements were written")
    y = buf[idx]                                                            # [clips, n_out, ch]
    if np.isnan(y).any():
        fails.append(f"{tag}: {int(np.isnan(y).sum())} elements of the result are NaN (not written, or computed from a read outside the column)")
    if not bool(res["same_" + name]):
        fails.append(f"{tag}: two runs of the job differ")
    # ---- values
    cols = np.ascontiguousarray(y.transpose(0, 2, 1)).reshape(clips * ch, j["n_out"]).astype(np.float64)
    for c, ref in enumerate(planned["refs"][name]):
        if ref.shape != (j["n_out"],):
            fails.append(f"{tag} column {c}: oracle length {ref.shape}")
            continue
        err = cols[c] - ref
        s = _rms(ref)
        rel, worst = _rms(err) / s, float(np.abs(err).max()) / s
        figs["rel"], figs["point"] = max(figs.get("rel", 0.0), rel), max(figs.get("point", 0.0), worst)
        if j["signal"] == "impulses":
            figs["imp_rel"], figs["imp_point"] = max(figs.get("imp_rel", 0.0), rel), max(figs.get("imp_point", 0.0), worst)
        print(f"{name} column {c}: rel RMS {rel:.3g}  worst point {worst:.3g} x RMS")
        if not rel <= REL_BAR:
            fails.append(f"{tag} column {c}: rel RMS {rel:.3g} > {REL_BAR:g}")
        if not worst <= POINT_BAR:
            fails.append(f"{tag} column {c}: worst point {worst:.3g} x RMS > {POINT_BAR:g}")
    return cols


def _case_figures(child, c, planned, results):
    """Every job of a case in a child -> (what failed, the case's record: geometry and the largest figures)."""
    name = bp.case_name(c)
    fails, figs, by_job = [], {}, {}
    mine = [j for j in planned["jobs"] if j["case"] == name and (j["child"] == child or (child == "nopair" and j["log"] is None))]
    assert mine
    for j in mine:
        by_job[j["name"]] = _check_job(j, planned, results, fails, figs)
    if child == "nopair":                                                   # k_fft_block against the paired kernels, job by job
        for j in mine:
            twin = by_job.get("twin__" + j["name"])
            if j["log"] is None or by_job[j["name"]] is None or twin is None:
                continue
            for col in range(twin.shape[0]):
                d = _rms(by_job[j["name"]][col] - twin[col]) / _rms(twin[col])
                figs["twin"] = max(figs.get("twin", 0.0), d)
                if not d <= REL_BAR:
                    fails.append(f"{j['tag']}/{j['layout']} column {col}: {d:.3g} relative RMS from the paired kernel's result")
    g = planned["geoms"][(name, child)]
    return fails, dict(figs, k=g["k"], A=g["A"], fwd=bp.sched_text(g["fwd"]), B=g["B"], inv=bp.sched_text(g["inv"]), hop_out=g["hop_out"], v0=g["v0"],
                       jobs=len(mine))


def _run_case(child, c, planned, results):
    fails, _ = _case_figures(child, c, planned, results)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("c", bp.CASES, ids=bp.case_name)
def test_product_reachable_case(c, planned, results):
    _run_case("plain", c, planned, results)


@pytest.mark.parametrize("c", [c for c in bp.CASES if c["large"]], ids=bp.case_name)
def test_large_variant(c, planned, results):
    g = planned["geoms"][(bp.case_name(c), "large")]
    assert (g["k"], g["A"], g["B"]) == c["large"]
    _run_case("large", c, planned, results)


@pytest.mark.parametrize("c", bp.NOPAIR_CASES, ids=bp.case_name)
def test_no_pair_case_and_its_paired_twin(c, planned, results):
    _run_case("nopair", c, planned, results)


def test_every_parsed_instance_ran_under_form_block(planned, results):
    """The instances of the cases whose every job the launch log gave to k_fft_block, on the planned geometry, with no
    switch set: all that run_passes holds."""
    ran = set()
    for c in bp.CASES:
        mine = [j for j in planned["jobs"] if j["case"] == bp.case_name(c) and j["child"] == "plain" and j["log"]]
        lines = [json.loads(str(results["plain"].get("log_" + j["name"], "[]"))) for j in mine]
        if all(len(l) == 1 and l[0].get("form") == "block" and l[0].get("k") == str(j["log"]["k"]) and l[0].get("hop_out") == str(j["log"]["hop_out"])
               for l, j in zip(lines, mine)):
            ran |= planned["geoms"][(bp.case_name(c), "plain")]["instances"]
    missing = sorted(set(bp.instances(planned["parsed"])) - ran)
    assert not missing, missing


def test_record(planned, results, capsys):
    """The figures of every case (profiles/NOTES_fft_block.md) and the children's time; every case has its figures."""
    rows = [("plain", c) for c in bp.CASES] + [("large", c) for c in bp.CASES if c["large"]] + [("nopair", c) for c in bp.NOPAIR_CASES]
    record = {}
    for child, c in rows:
        _, r = _case_figures(child, c, planned, results)
        record[(child, bp.case_name(c))] = r
    capsys.readouterr()                                                     # (the per-column lines were printed by the case tests)
    print("child case | k | A [fwd] | B [inv] | hop_out v0 | jobs | rel RMS | worst point x RMS | impulses rel, point | vs paired")
    for (child, name), r in sorted(record.items()):
        print("%s %s | %d | %d [%s] | %d [%s] | %d %d | %d | %.3g | %.3g | %s | %s" % (
            child, name, r["k"], r["A"], r["fwd"], r["B"], r["inv"], r["hop_out"], r["v0"], r["jobs"], r.get("rel", float("nan")),
            r.get("point", float("nan")), "%.3g, %.3g" % (r["imp_rel"], r["imp_point"]) if "imp_rel" in r else "-",
            "%.3g" % r["twin"] if "twin" in r else "-"))
    print("the three child processes: %.1f s" % results["seconds"])
    assert all("rel" in r and "point" in r for r in record.values()), "a case without figures: " + str([k for k, r in record.items() if "rel" not in r])
