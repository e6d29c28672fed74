"""Every float16 / bfloat16 kernel instance of the paired-block schedule table (csrc/fft.hip: fft_half_kernels, the
HIPSOXR_HALF_ROW / HIPSOXR_HALF_ROW_F32 rows over the instantiation lists), knowingly — the half counterpart of
tests/test_gpu_fft_table.py, in a module and child processes of its own.  The half table is parsed from the source
(tests/_table_probe.py parse_half); a half job takes the row the float32 job of its shape takes, so every (row, half
instance, recipe) that fft_geometry admits gets the jobs of the float32 instance of its form — the same lengths around the
seams of its work items, under the same switches — and the launch record of the debug-switch build must name the form, the
row, kind=f16 / bf16 and the recomputed hop_out for the half job, and the same form and row with kind=f32 for its float32
twin: a half job that fell back to the widening passes, or a twin served by another row, fails its case.

The contract is an identity: the half result equals the float32 job of the same row and layout on the exactly widened
values, rounded once (`.to(dtype)`), bit for bit in every column.  Layouts: unit-stride columns as a 1-D column, a
(3, n, 1) batch (float16: column 2 at 2^-12, most outputs subnormal), the input at an odd element with the output at an
odd element, the output 6 elements into a 16-byte granule; channel pairs as (n, 2), (2, n, 4) and input and output one
frame in.  Per unit-stride case one ragged job over a clip table (clips of 3 hop + 5 outputs, one frame short of the
two-item seam, 1 frame and none, packed at odd offsets with guards).  8 sentinel elements before and behind every column
and the guards stay intact; the shape is exact; the first layout of each length twice gives the same bytes.

Independently of the twin, every point is held to the oracle's float64 direct form on the widened input:
|y - ref| <= 4e-5 x RMS(ref) + half an ulp of the half type at |ref| + 4e-5 x RMS(ref) — the float32 engine's pointwise bar
of tests/test_gpu_fft.py plus the one rounding at the largest magnitude the float32 value can have.

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
    half = tp.parse_half()
    cases, status = tp.case_plan(rows, macros, lambda L, M, q: dev.Plan(*tp.rates_of(L, M), q).taps, half=half)
    return rows, half, cases, status


@pytest.fixture(scope="module")
def runs(table_and_plan, tmp_path_factory):
    rows = table_and_plan[0]
    assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
    out = {}
    for name, switches in tp.children(rows).items():
        env = {k: v for k, v in os.environ.items() if not k.startswith("HIPSOXR_")}
        env.update(switches)
        env["HIPSOXR_LIBRARY"] = DBG_LIB
        env["HIPSOXR_DEBUG_LAUNCH_LOG"] = str(tmp_path_factory.mktemp("launch_log_half") / (name + ".log"))
        t0 = time.time()
        r = subprocess.run([sys.executable, os.path.join(HERE, "_table_probe.py"), "half:" + name], env=env, capture_output=True, text=True, timeout=1500)
        started = [l for l in r.stdout.splitlines() if l.startswith("TABLE_CASE ")]
        assert r.returncode == 0, (name, "last case started: " + (started[-1] if started else "none"), r.stderr[-2000:])
        line = [l for l in r.stdout.splitlines() if l.startswith("TABLE_PROBE ")][-1]
        out[name] = json.loads(line[len("TABLE_PROBE "):])
        print(f"child {name}: {len(out[name])} cases, {sum(v['jobs'] for v in out[name].values())} jobs, {time.time() - t0:.0f} s")
    return out


def test_every_admissible_half_instance_is_launched_and_equals_its_float32_twin(table_and_plan, runs):
    rows, half, cases, status = table_and_plan
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
    # the census: row x half instance, VHQ/HQ each — R reached (launched by its own instance beside its float32 twin, every
    # check held), F failed, I not admitted by fft_geometry for the recipe, - the row has no such pointer
    print("census (VHQ/HQ): " + "  ".join("%s.%s" % i for i in tp.HALF_INSTANCES))
    for r in rows:
        cells = []
        for inst in tp.HALF_INSTANCES:
            if inst not in tp.half_instances_of(r, half):
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
    print(f"{len(cases)} cases, {len(failed)} failed")
    assert not failed, (len(failed), failed[:10])
    assert set(done) == {tp.case_id(c) for c in cases}
    # nothing admissible is left unlaunched: no half instance is unreachable
    for (row, inst, q), st in status.items():
        assert st != "unreachable", (row, inst, q)
        if st == "case":
            assert mark[(row, inst, q)] == "R"
