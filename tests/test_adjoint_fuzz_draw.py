"""tests/fuzz/fuzz_adjoint.py draw(): what the GPU run of tests/test_gpu_adjoint_fuzz.py will do, enumerated on the CPU — the
draw is deterministic, imports neither torch nor the native library, stays within the size limits, keeps the refusals it
predicts under the cap, and meets every listed size class, layout, type and selector at the seeds and counts the GPU test
uses.  No GPU."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "fuzz"))
import fuzz_adjoint as fa  # noqa: E402
import test_gpu_adjoint_fuzz as gf  # noqa: E402

PARAMS = [(family, seed) for family in fa.FAMILIES for seed in gf.SEEDS[family]]


@pytest.fixture(scope="module")
def draws():
    return {p: fa.draw(p[0], gf.CASES[p[0]], p[1]) for p in PARAMS}


def test_draw_is_deterministic_plain_and_needs_no_library(draws):
    for (family, seed), jobs in draws.items():
        assert jobs == fa.draw(family, gf.CASES[family], seed) and len(jobs) == gf.CASES[family]
        assert json.loads(json.dumps(jobs)) == jobs, "plain dicts"
        assert [c["index"] for c in jobs] == list(range(len(jobs))) and len({c["seed"] for c in jobs}) == len(jobs)
    assert draws[PARAMS[0]] != fa.draw(PARAMS[0][0], gf.CASES[PARAMS[0][0]], PARAMS[0][1] + 1000)
    # in a fresh interpreter: the same jobs, and neither torch nor the native library was imported for them
    code = ("import sys, json; sys.path.insert(0, %r); import fuzz_adjoint as fa; d = fa.draw('fast', 6, 3); "
            "assert 'torch' not in sys.modules and not any(m.startswith('soxr_amd') for m in sys.modules); print(json.dumps(d))" % os.path.join(HERE, "fuzz"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert json.loads(out.stdout) == fa.draw("fast", 6, 3)


@pytest.mark.parametrize("family,seed", PARAMS)
def test_size_limits(draws, family, seed):
    for c in draws[(family, seed)]:
        frames, elems = fa.job_extent(c)
        assert frames <= fa.MAX_FRAMES and elems <= fa.MAX_ELEMS, c
        if family != "ragged":
            assert c["n_x"] >= 1 and 0 <= c["n_y"] <= (2 * c["n_x"] * c["L"] + c["M"]) // (2 * c["M"]), c
            assert c["rank"] == 3 or c["clips"] == 1 and (c["rank"] == 2 or c["channels"] == 1), c
        else:
            assert 2 <= len(c["rows"]) <= 9 and 1 <= c["channels"] <= 3
            assert all(0 <= n_y <= (2 * n_x * c["L"] + c["M"]) // (2 * c["M"]) for n_x, n_y in c["rows"]), c
        assert max(c["rates"][0] / c["rates"][1], c["rates"][1] / c["rates"][0]) <= 6


@pytest.mark.parametrize("family,seed", PARAMS)
def test_predicted_refusals_stay_under_the_cap(draws, family, seed):
    jobs = draws[(family, seed)]
    for sel in {s for c in jobs for s in c["selectors"]}:
        mine = [c for c in jobs if sel in c["selectors"]]
        refused = [c for c in mine if c.get("refusal")]
        assert len(refused) * fa.REFUSAL_CAP <= len(mine), (sel, len(refused), len(mine))
        assert all(sel == fa.ADJOINT_TWO_STAGE for c in refused)
    for c in jobs:
        assert not (c.get("refusal") and c["autograd"])


@pytest.mark.parametrize("seed", gf.SEEDS["exact"])
def test_exact_family_meets_every_class(draws, seed):
    jobs = draws[("exact", seed)]
    assert all(not c["phases"] and c["selectors"] == [fa.AUTO, fa.EXACT, fa.ADJOINT] for c in jobs)
    assert {c["n_x_class"] for c in jobs} >= set(fa.EXACT_N_X)
    assert {c["layout"] for c in jobs} == set(fa.LAYOUTS) and {c["kind"] for c in jobs} == {"f32", "f64", "f16", "bf16"}
    assert {c["quality"] for c in jobs} == set(fa.RECIPES) and {c["rank"] for c in jobs} == {1, 2, 3}
    assert {c["cut"] for c in jobs} == {"full", "truncated", "empty"} and any(c["autograd"] for c in jobs)
    assert {c["source"] for c in jobs} == {"std", "int", "prime"}
    # what the random integer pairs are there for: L < 16, M < 16 and both parities of the replicated period Lc
    lc = [max(-(-16 // c["M"]), -(-64 // c["L"])) * c["L"] for c in jobs]
    assert any(c["L"] < 16 for c in jobs) and any(c["M"] < 16 for c in jobs)
    assert any(v % 2 for v in lc) and any(v % 2 == 0 for v in lc)


@pytest.mark.parametrize("seed", gf.SEEDS["interp"])
def test_interp_family_meets_every_class(draws, seed):
    jobs = draws[("interp", seed)]
    assert all(c["phases"] and c["selectors"] == [fa.ADJOINT] and c["channels"] <= 3 and 1 <= c["n_x"] <= 20000 for c in jobs)
    big = [c for c in jobs if c["n_x"] >= 8192]
    assert 2 * len(big) >= len(jobs) - 1 and len(big) < len(jobs)
    assert {c["layout"] for c in jobs} == set(fa.LAYOUTS) and {c["kind"] for c in jobs} == {"f32", "f64"}
    assert {c["source"] for c in jobs} == {"int", "float"} and any(c["autograd"] for c in jobs)


@pytest.mark.parametrize("seed", gf.SEEDS["fast"])
def test_fast_family_meets_every_class(draws, seed):
    jobs = draws[("fast", seed)]
    by = {s: [c for c in jobs if c["selectors"] == [s]] for s in (fa.ADJOINT_AUTO, fa.ADJOINT_FFT, fa.ADJOINT_TWO_STAGE)}
    assert all(by.values()) and sum(len(v) for v in by.values()) == len(jobs)
    assert len(by[fa.ADJOINT_AUTO]) >= len(jobs) // 2 - 1
    assert all(not c["phases"] and c["quality"] in ("HQ", "VHQ") for c in by[fa.ADJOINT_FFT])
    assert all(c["phases"] and c["quality"] in ("HQ", "VHQ") for c in by[fa.ADJOINT_TWO_STAGE])
    # AUTO: both kinds of plan, every selector it can resolve to, both sides of both thresholds
    auto = by[fa.ADJOINT_AUTO]
    assert {c["resolves"] for c in auto} == {fa.ADJOINT, fa.ADJOINT_FFT, fa.ADJOINT_TWO_STAGE}
    assert {c["n_x_class"] for c in auto if not c["phases"]} >= {"below", "at", "above"}
    every = {"smallest-1", "smallest", "smallest+1", "random"}
    assert {c["n_x_class"] for c in auto if c["phases"]} == every and {c["n_x_class"] for c in by[fa.ADJOINT_TWO_STAGE]} == every
    # the named selector's "one below" size is a predicted refusal, and the draw holds one (the cap admits exactly one of 8 cases)
    refused = [c for c in by[fa.ADJOINT_TWO_STAGE] if c["refusal"]]
    assert len(by[fa.ADJOINT_TWO_STAGE]) == 8 and len(refused) == 1 and refused[0]["n_x_class"] == "smallest-1" and refused[0]["refusal"] == "frames"
    assert all(c["n_x_class"] != "smallest-1" for c in by[fa.ADJOINT_TWO_STAGE] if not c["refusal"])
    # autograd: every selector, and no forward on the frequency-domain engine (the launch log's FFT lines are adjoints')
    assert all(any(c["autograd"] for c in v) for v in by.values()) and all(c["forward"] == fa.EXACT for c in jobs)
    # AUTO meets the pairs KERNEL_ADJOINT_FFT is not drawn on; the named selector does not
    assert all(c["rates"][0] != c["rates"][1] and {c["rates"][0], c["rates"][1]} not in fa.FFT_NOT_SERVED for c in by[fa.ADJOINT_FFT])
    for c in auto:
        if not c["phases"] and c["n_x_class"] in ("below", "at", "above"):
            total = c["n_y"] * c["clips"] * c["channels"]
            assert (total >= fa.FFT_AUTO_MIN) == (c["n_x_class"] != "below") and abs(total - fa.FFT_AUTO_MIN) <= 2 * c["clips"] * c["channels"]
    assert {c["layout"] for c in jobs} == set(fa.LAYOUTS) and {c["kind"] for c in jobs} == {"f32", "f64"}


@pytest.mark.parametrize("seed", gf.SEEDS["ragged"])
def test_ragged_family_meets_every_class(draws, seed):
    jobs = draws[("ragged", seed)]
    assert {c["group"] for c in jobs} == {"exact", "fft", "interp", "auto-interp"}
    assert {s for c in jobs for s in c["selectors"]} >= {fa.ADJOINT, fa.ADJOINT_FFT, fa.ADJOINT_AUTO}
    assert {x for c in jobs for x in c["row_classes"]} == set(fa.RAGGED_LEN)
    assert any(n_y == 0 < n_x for c in jobs for n_x, n_y in c["rows"]), "a clip without cotangent"
    assert any(any(c["admitted"]) and not all(c["admitted"]) for c in jobs), "a table with admitted and other clips"
    assert all(any(c["admitted"]) for c in jobs if c["group"] == "auto-interp"), "every KERNEL_ADJOINT_AUTO table holds an admitted clip"
    assert all(c["forward"] == fa.EXACT for c in jobs)
    # the tables steered to k_adj_tile's 32- and 16-lane slabs: interleaved channels, a clip long enough for the tiled kernel
    lanes = {c["lanes"]: c for c in jobs if c["lanes"]}
    assert sorted(lanes) == [16, 32]
    for c in lanes.values():
        mc = max(-(-16 // c["M"]), -(-64 // c["L"])) * c["M"]
        assert c["group"] == "exact" and c["channels"] in (2, 3) and max(n_x for n_x, _ in c["rows"]) >= 4 * mc
    assert {c["channels"] for c in jobs} == {1, 2, 3} and {c["kind"] for c in jobs} == {"f32", "f64"}
