"""Every kernel instance of the paired-block schedule table (csrc/fft.hip, fft_pairs) against the oracle's float64 direct
form, knowingly: the table is parsed from the source (tests/_table_probe.py), every (row, instance, recipe) that
fft_geometry admits gets jobs that must land on that instance — the row chosen by the debug-switch build's
HIPSOXR_FFT_LARGE_ONLY / _SMALL_ONLY / _NO_TINY / HIPSOXR_DEBUG_FFT_K, the instance by element type, selector and layout
— and the launch record of that build (HIPSOXR_DEBUG_LAUNCH_LOG) must name the intended form, row and kind, and the
hop_out that Python recomputes from the plan: a job served by anything else fails its case.

Per job: exact shape; written through `out=` into a buffer whose 8 elements before and behind every column stay intact;
twice the same bytes.  Output lengths end just before, on and just behind the kept run of one work item (two for
channel pairs), at an odd block count and at several items plus a seeded remainder.  float32 at the bars of
tests/test_gpu_fft.py (1e-6 relative RMS, 4e-5 x RMS pointwise, 4e-6 x RMS per 2048-sample stretch, 1e-5 at both ends);
float64 and float32-on-float64 at theirs (2e-9 / 5e-8 VHQ, 1e-6 HQ) and, per stretch and pointwise, at four times what
the float64 overlap-save model at the row's block size leaves on the same inputs (tests/golden/fft_table_floor.json;
float32 results: plus their rounding, 2^-24 of the sample); int16 / int32 equal to the float job of the same row plus
oracle.quantize, sample for sample, clip count included.

One child process per switch setting, one after another; each reports through one JSON line."""
import json
import os
import subprocess
import sys
import time

import pytest

import _table_probe as tp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DBG_LIB = os.path.join(os.path.dirname(HERE), "python-soxr_amd", "_variants", "dbg", "libhipsoxr.so")


@pytest.fixture(scope="module")
def table_and_plan():
    from soxr_amd import device as dev
    rows, macros = tp.parse_table()
    cases, status = tp.case_plan(rows, macros, lambda L, M, q: dev.Plan(*tp.rates_of(L, M), q).taps)
    return rows, macros, cases, status


@pytest.fixture(scope="module")
def runs(table_and_plan, tmp_path_factory):
    rows = table_and_plan[0]
    assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
    out = {}
    for name, switches in tp.children(rows).items():
        env = {k: v for k, v in os.environ.items() if not k.startswith("HIPSOXR_")}
        env.update(switches)
        env["HIPSOXR_LIBRARY"] = DBG_LIB
        env["HIPSOXR_DEBUG_LAUNCH_LOG"] = str(tmp_path_factory.mktemp("launch_log") / (name + ".log"))
        t0 = time.time()
        r = subprocess.run([sys.executable, os.path.join(HERE, "_table_probe.py"), name], env=env, capture_output=True, text=True, timeout=1500)
        started = [l for l in r.stdout.splitlines() if l.startswith("TABLE_CASE ")]
        assert r.returncode == 0, (name, "last case started: " + (started[-1] if started else "none"), r.stderr[-2000:])
        line = [l for l in r.stdout.splitlines() if l.startswith("TABLE_PROBE ")][-1]
        out[name] = json.loads(line[len("TABLE_PROBE "):])
        print(f"child {name}: {len(out[name])} cases, {sum(v['jobs'] for v in out[name].values())} jobs, {time.time() - t0:.0f} s")
    return out


def test_every_admissible_instance_is_launched_and_within_its_bars(table_and_plan, runs):
    rows, macros, cases, status = table_and_plan
    done = {}
    for name, res in runs.items():
        done.update(res)
    failed = []
    mark = {}
    for c in cases:
        r = done.get(tp.case_id(c))
        ok = bool(r and r["ok"] and r["jobs"] > 0)
        mark[(c["row"], (c["form"], c["kind"]), c["quality"])] = "R" if ok else "F"
        if not ok:
            failed.append((tp.case_id(c), r and r["fails"]))
    # the census: row x instance, VHQ/HQ each — R reached (launched by its own instance, every check held), F failed,
    # U unreachable under any switch (tests/_table_probe.py UNREACHABLE), I not admitted by fft_geometry for the recipe
    print("census (VHQ/HQ): " + "  ".join("%s.%s" % i for i in tp.INSTANCES))
    for r in rows:
        cells = []
        for inst in tp.INSTANCES:
            if inst not in tp.instances_of(r, macros):
                cells.append("-/-")
                continue
            cells.append("/".join(mark.get((tp.row_key(r), inst, q), {"unreachable": "U", "inadmissible": "I"}.get(status[(tp.row_key(r), inst, q)], "?"))
                                  for q in tp.QUALITIES))
        print("%-16s %s" % (tp.row_name(r), " ".join(cells)))
    worst = {}
    for cid, r in done.items():
        for k, v in r["share_of_bar"].items():
            kind = cid.split("/")[2]
            if v > worst.get((kind, k), (0, ""))[0]:
                worst[(kind, k)] = (v, cid)
    for (kind, k), (v, cid) in sorted(worst.items()):
        print(f"largest share of its bar: {kind} {k}: {v:.3f} ({cid})")
    assert not failed, (len(failed), failed[:10])
    assert set(done) == {tp.case_id(c) for c in cases}
    # nothing admissible is left unlaunched but what UNREACHABLE lists with its host condition
    for (row, inst, q), st in status.items():
        if st == "unreachable":
            assert (row, inst) in tp.UNREACHABLE, (row, inst, q)
        elif st == "case":
            assert mark[(row, inst, q)] == "R"
