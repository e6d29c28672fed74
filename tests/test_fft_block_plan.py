"""The case plan of tests/test_gpu_fft_block.py (tests/_block_probe.py), held to its conditions without a GPU: the pass
instances of k_fft_block are parsed from the `switch` of run_passes (csrc/fft.hip); every one of them must be run by a
case the product reaches with no switch set, at a ratio outside the schedule table; the schedule each case is expected to
run, typed into the plan, must be what the restatement of factor_radices / fft_kept_run / fft_geometry gives on the
oracle's plan.  So an instance added, removed or re-thresholded in the source fails here until the plan follows — shown on
doctored copies of run_passes.  (The launch log ties the restatement to the product's own choice: the GPU test.)"""
import re

import pytest

import _block_probe as bp
from oracle import oracle as o


def plan_of(rates, quality):
    return o.plan(rates[0], rates[1], quality)


@pytest.fixture(scope="module")
def parsed():
    return bp.parse_run_passes()


@pytest.fixture(scope="module")
def planned(parsed):
    return bp.all_jobs(parsed, plan_of)


def test_the_parse(parsed):
    inst = bp.instances(parsed)
    assert parsed["signs"] == [-1, 1] and parsed["default"] == 2
    assert len(inst) == len(set(inst)) == 2 * sum(len(v) for v in parsed["rules"].values())
    assert set(parsed["rules"]) == {2, 3, 4, 5, 7, 8, 16}, "factor_radices emits these radices; each needs a pass of its own"
    # the bound run_passes states: N / R butterflies fit NB rounds of the 256 threads for every N <= 4096
    for R, lst in parsed["rules"].items():
        assert (bp.MAX_HALF // R + bp.NT - 1) // bp.NT <= lst[-1][1], (R, lst)
        for per_max, nb in lst[:-1]:
            assert per_max <= nb, (R, lst)


def test_coverage(parsed):
    assert bp.check_plan(parsed, plan_of) == []


def test_every_case_is_within_bounds(parsed):
    for c in bp.CASES + bp.NOPAIR_CASES:
        g = bp.block_job(parsed, plan_of(c["rates"], c["quality"]), "small")
        assert 0 < g["A"] <= 4096 and 0 < g["B"] <= 4096 and g["lds_bytes"] <= bp.LDS_BOUND
        assert g["lds_bytes"] >= (max(g["A"], g["B"]) + 1) * 8, "k_fft_block: a single buffer of max(A, B) + 1 complex values"
        assert g["A"] % 2 == 0 and g["B"] % 2 == 0 and g["hop_out"] % 2 == 0, "k >= 4 and hop_periods = k - 2 lead_periods: always even"
        assert g["hop_periods"] == g["k"] - 2 * g["lead_periods"]


def _doctored(change):
    body = bp.run_passes_text()
    new = change(body)
    assert new != body
    with open(bp.FFT_SRC) as f:
        return bp.parse_run_passes(body=new, text=f.read())


def test_doctored_source_an_instance_added():
    p = _doctored(lambda b: b.replace("        default:", "        case 6: fft_pass<6, SIGN, 2>(buf, N, Ns, W); break;\n        default:"))
    assert (6, 2, -1) in bp.instances(p)
    bad = bp.check_plan(p, plan_of)
    assert any("fft_pass<6, -1, 2>" in b for b in bad) and any("fft_pass<6, +1, 2>" in b for b in bad), bad


def test_doctored_source_a_threshold_changed():
    p = _doctored(lambda b: b.replace("case 7: if (per <= 2)", "case 7: if (per <= 1)"))
    bad = bp.check_plan(p, plan_of)
    assert any(b.startswith("8000_28000_VHQ:") for b in bad), bad        # 3584 / 7 = 512 butterflies: two rounds, now NB = 3
    p = _doctored(lambda b: b.replace("case 3: if (per <= 4)", "case 3: if (per <= 5)"))
    bad = bp.check_plan(p, plan_of)
    assert any(b.startswith("44100_20000_VHQ:") for b in bad), bad       # 3528 / 3 = 1176 butterflies: five rounds, now NB = 4


def test_doctored_source_an_instance_removed():
    p = _doctored(lambda b: re.sub(r"\n        case 4:[^\n]*", "", b))
    assert 4 not in p["rules"]
    bad = bp.check_plan(p, plan_of)
    assert any(b.startswith("8000_28000_VHQ:") for b in bad), bad        # [4, 16, 16] would run the default's radix-2 pass


def test_restatement_on_a_tabled_pair(parsed):
    pl = o.plan(48000, 44100, "VHQ")
    assert bp.on_table(pl.L, pl.M)
    large, small = bp.block_job(parsed, pl, "large"), bp.block_job(parsed, pl, "small")
    assert (large["k"], large["hop_out"], large["A"], large["B"]) == (32, 4410, 2560, 2352)
    assert (small["k"], small["hop_out"], small["A"], small["B"]) == (16, 2058, 1280, 1176)
    # ... and against the restatement tests/_table_probe.py keeps of the kept run
    for g in (large, small):
        assert bp.tp.hop_out(pl.L, pl.M, pl.T, g["k"]) == g["hop_out"]


def test_geometry_classes(parsed, planned):
    jobs, geoms = planned
    by_case = {(bp.case_name(c), "plain"): c for c in bp.CASES + bp.NOPAIR_CASES}
    up = {bp.case_name(c) for c in bp.CASES if c["A"] < c["B"]}
    down = {bp.case_name(c) for c in bp.CASES if c["A"] > c["B"]}
    assert up and down
    v0 = {name: g["v0"] for (name, child), g in geoms.items() if child == "plain"}
    # a kept run [v0, v0 + hop_out) that begins and ends at an odd local output: both ends split the (re, im) = (2n, 2n + 1) pair of an LDS element
    assert any(v0[n] % 2 for n in up) and any(v0[n] % 2 for n in down) and any(v0[n] % 2 == 0 for n in up | down)
    for side in (up, down):
        mine = [j for j in jobs if j["case"] in side and j["log"]]
        assert any(j["n_in"] % 2 for j in mine) and any(j["n_in"] % 2 == 0 for j in mine), "odd and even in_frames"
    assert {j["child"] for j in jobs} == set(bp.CHILDREN)
    assert any(c["large"] for c in bp.CASES)
    for (name, child), g in geoms.items():
        if child == "large":
            assert g["k"] > geoms[(name, "plain")]["k"]
    assert by_case


def test_job_lengths_layouts_and_selectors(parsed, planned):
    jobs, geoms = planned
    names = [j["name"] for j in jobs]
    assert len(names) == len(set(names))
    for j in jobs:
        pl = plan_of(j["rates"], j["quality"])
        key = (j["case"], "nopair" if j["name"].startswith("twin__") else j["child"])
        hop = geoms[key]["hop_out"]
        assert pl.out_len(j["n_in"]) == j["n_out"]
        if j["tag"] == "one":
            assert j["n_out"] == hop
        elif j["tag"] == "plus1":
            assert j["n_out"] > hop and pl.out_len(j["n_in"] - 1) <= hop
            if pl.L < pl.M:
                assert j["n_out"] == hop + 1
        else:
            assert j["n_out"] > 2 * hop and j["n_out"] % hop, "first, interior and a partial last block"
        if j["kernel"] == bp.AUTO:
            assert j["n_out"] >= bp.AUTO_MIN and j["child"] == "plain" and j["log"]
        else:
            assert j["kernel"] == bp.FFT
        if j["log"]:
            assert j["log"]["n_blocks"] == -(-j["n_out"] // hop) and j["log"]["lds"] == (max(geoms[key]["A"], geoms[key]["B"]) + 8) * 8
        if j["signal"] == "impulses":
            p0 = bp.impulse_at(j["n_in"], hop, pl.L, pl.M)
            for p in (p0, p0 + 15):                       # the impulse's own output instant lies in the interior block's kept run
                assert hop <= p * pl.L // pl.M < 2 * hop and p < j["n_in"]
    for c in bp.CASES:
        mine = [j for j in jobs if j["case"] == bp.case_name(c) and j["child"] == "plain" and j["log"]]
        layouts = {j["layout"] for j in mine}
        assert layouts == ({"mono", "il3", "planar3", "slice", "imp16"} if c.get("wide") else {"mono", "il3"})
        assert any(j["kernel"] == bp.AUTO for j in mine) == bool(c.get("auto"))
    # lengths below 2^13 outputs go by name
    assert all(j["kernel"] == bp.FFT for j in jobs if j["n_out"] < bp.AUTO_MIN)
