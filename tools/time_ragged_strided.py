#!/usr/bin/env python3
"""Ragged batches of INTERLEAVED clips ([frames, channels]: what dist.RaggedJob builds for every multichannel clip) — what one
call costs now that the frequency-domain engine's strided kernel reads a clip table (exact-bank plans, by name) and the two-stage
form admits tables at a frame stride (interpolated-phase plans, KERNEL_AUTO).  Run this tool once per library (HIPSOXR_LIBRARY
selects it), each run a process of its own, alternated, with --json; then --merge the records (tools/time_ragged_two_stage.py is
the same tool for mono tables).

Rows, exact-bank ("by name"): per table three contestants, each timed on the library of the run —
    table   RaggedJob(kernel=KERNEL_FFT) (int16: KERNEL_FFT_PCM).launch(): ONE launch here; the parent refuses it (recorded)
    loop    a Python loop of resample_tensor(plan, clip, kernel=KERNEL_FFT / _PCM) per clip: the parent's way to the fast engine
    exact   RaggedJob(kernel=KERNEL_EXACT).launch(): the parent's one-launch alternative (the exact engine, bit-exact)
Rows, two-stage: RaggedJob(plan, clips).launch() under KERNEL_AUTO, the same call on both libraries.
Tables: 64 and 1024 stereo float32 clips of 1-10 s and of 0.1-1 s; 64 clips of 8 channels at 44.1k -> 16k; 64 stereo int16
clips; 64 stereo float64 clips.  Clips are views of one packed buffer.  Per repetition one call is timed between two HIP events on
the current stream, host-side work included; median (min-max) over the repetitions.

--shape F (debug-switch build with HIPSOXR_DEBUG_LAUNCH_LOG): one launch per exact-bank row, no timing; from the launch's own
log line (form, hop_out) and the table the tool counts the work items each of the 8 XCDs gets under the kernel's map — per_xcd
from the clip's OWN item count — and under the alternative, per_xcd from the longest clip: busiest XCD / mean.

    HIPSOXR_LIBRARY=<parent build>/libhipsoxr.so python tools/time_ragged_strided.py --json parent1.json
    python tools/time_ragged_strided.py --json this1.json          (and once more each: parent2.json, this2.json)
    HIPSOXR_LIBRARY=<debug-switch build> HIPSOXR_DEBUG_LAUNCH_LOG=log python tools/time_ragged_strided.py --shape shape.json
    python tools/time_ragged_strided.py --merge parent1.json this1.json parent2.json this2.json --with-shape shape.json --out rows.md

--merge pools the repetitions of each library and states the acceptance per row: this tree's median must not exceed the better
contestant's median (parent's library) by more than the larger of the two min-max spreads."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "python-soxr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

LONG, SHORT = (1.0, 10.0), (0.1, 1.0)
# kind, name, in rate, out rate, quality, dtype, channels, [(clips, seconds)]
WORKLOADS = [
    ("by name", "48000->44100 VHQ float32 stereo", 48000, 44100, "VHQ", "float32", 2, [(64, LONG), (1024, LONG), (64, SHORT), (1024, SHORT)]),
    ("by name", "44100->16000 HQ float32 8 ch", 44100, 16000, "HQ", "float32", 8, [(64, LONG)]),
    ("by name", "48000->44100 HQ int16 stereo", 48000, 44100, "HQ", "int16", 2, [(64, LONG)]),
    ("by name", "48000->44100 VHQ float64 stereo", 48000, 44100, "VHQ", "float64", 2, [(64, LONG)]),
    ("two-stage", "48000->44101 VHQ float32 stereo", 48000, 44101, "VHQ", "float32", 2, [(64, LONG), (1024, LONG), (64, SHORT), (1024, SHORT)]),
    ("two-stage", "44100->16001 HQ float32 8 ch", 44100, 16001, "HQ", "float32", 8, [(64, LONG)]),
    ("two-stage", "48000->44101 VHQ float64 stereo", 48000, 44101, "VHQ", "float64", 2, [(64, LONG)]),
]


def fmt(ts):
    return "%.0f (%.0f-%.0f)" % (statistics.median(ts), min(ts), max(ts)) if ts else "refused"


def merge(paths, out, shape_path=None):
    shape = {}
    if shape_path:
        with open(shape_path) as f:
            shape = {(r["name"], r["clips"], tuple(r["seconds"])): r for r in json.load(f)["rows"]}
    recs = []
    for p in paths:
        with open(p) as f:
            recs.append(json.load(f))
    parents, these = recs[0::2], recs[1::2]
    by = ["| table | clip lengths, s | clips | frames in all | parent: loop of KERNEL_FFT, us | parent: RaggedJob(KERNEL_EXACT), us | parent: RaggedJob by name | this tree: one launch by name, us | best parent / this | accepted | form, hop_out | busiest XCD / mean: own per_xcd (as built) | ... per_xcd of the longest clip |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    two = ["| table | clip lengths, s | clips | frames in all | parent (clip by clip), us | this tree, us | parent / this | accepted |", "|---|---|---|---|---|---|---|---|"]
    for i, rb in enumerate(these[0]["rows"]):
        for r in parents + these:
            ri = r["rows"][i]
            assert (ri["name"], ri["seconds"], ri["clips"], ri["frames"]) == (rb["name"], rb["seconds"], rb["clips"], rb["frames"])
            assert ri["sums_equal"], "a library's result changed between repetitions: %r" % rb["name"]
        pool = lambda rs, mode: [t for r in rs for t in (r["rows"][i]["modes"][mode] or [])]  # noqa: E731
        head = "| %s | %g-%g | %d | %d |" % (rb["name"], rb["seconds"][0], rb["seconds"][1], rb["clips"], rb["frames"])
        if rb["kind"] == "by name":
            loop, exact, ptab, mine = pool(parents, "loop"), pool(parents, "exact"), pool(parents, "table"), pool(these, "table")
            best = min((loop, exact), key=statistics.median)
            spread = max(max(best) - min(best), max(mine) - min(mine))
            ok = statistics.median(mine) <= statistics.median(best) + spread
            sh = shape.get((rb["name"], rb["clips"], tuple(rb["seconds"])))
            by.append("%s %s | %s | %s | %s | %.2f | %s | %s | %s | %s |" % (
                head, fmt(loop), fmt(exact), fmt(ptab), fmt(mine), statistics.median(best) / statistics.median(mine), "yes" if ok else "NO",
                "%s, %d" % (sh["form"], sh["hop_out"]) if sh else "n/a", "%.3f" % sh["own"] if sh else "n/a", "%.3f" % sh["longest"] if sh else "n/a"))
        else:
            pa, pb = pool(parents, "table"), pool(these, "table")
            spread = max(max(pa) - min(pa), max(pb) - min(pb))
            ok = statistics.median(pb) <= statistics.median(pa) + spread
            two.append("%s %s | %s | %.2f | %s |" % (head, fmt(pa), fmt(pb), statistics.median(pa) / statistics.median(pb), "yes" if ok else "NO"))
    text = "Exact-bank plans, by name:\n\n" + "\n".join(by) + "\n\nInterpolated-phase plans, KERNEL_AUTO (the two-stage form):\n\n" + "\n".join(two) + "\n"
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(text)


def xcd_balance(n_out, hop, chpair, own):
    """work items per XCD over the table under item = xcd * per_xcd + chunk (csrc/fft_ragged_rules.h fft_xcd_map), per_xcd from
    the clip's own item count or from the longest clip's: busiest XCD / mean (the channel units multiply every XCD alike)"""
    def items(o):
        blocks = -(-o // hop) if o > 0 else 0
        return blocks if chpair else (blocks + 1) // 2
    longest = max(items(o) for o in n_out)
    load = np.zeros(8)
    for o in n_out:
        n = items(o)
        per = -(-(n if own else longest) // 8)
        for x in range(8):
            load[x] += max(0, min(n, (x + 1) * per) - x * per) if per else 0
    return float(load.max() / load.mean())


def timed(fn, reps, torch):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)  # us
    torch.cuda.synchronize()
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", help="write this library's rows here")
    ap.add_argument("--merge", nargs="+", metavar="JSON", help="PARENT THIS [PARENT THIS ...] --json records -> markdown tables")
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shape", help="debug-switch build with HIPSOXR_DEBUG_LAUNCH_LOG: one launch per exact-bank row, the XCD balance -> this file")
    ap.add_argument("--with-shape", help="(--merge) a --shape record: fills the form and balance columns")
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out, args.with_shape)
    import torch
    assert torch.cuda.is_available(), "time_ragged_strided.py needs a GPU"
    from soxr_amd import _native, device as dev, dist

    rows = []
    for kind, name, fi, fo, q, dtype, ch, tables in WORKLOADS:
        if args.shape and kind != "by name":
            continue
        plan = dev.Plan(fi, fo, q)
        assert (plan.phases != 0) == (kind == "two-stage")
        tdt = getattr(torch, dtype)
        by_name = _native.KERNEL_FFT_PCM if dtype == "int16" else _native.KERNEL_FFT
        for n_clips, (lo, hi) in tables:
            rng = np.random.default_rng(n_clips)
            n_in = [int(v) for v in rng.integers(int(lo * fi), int(hi * fi) + 1, n_clips)]
            total = sum(n_in)
            g = torch.Generator(device="cuda").manual_seed(n_clips)
            packed = torch.rand((total, ch), dtype=torch.float32, device="cuda", generator=g) - 0.5
            packed = (packed * 20000).to(tdt) if dtype == "int16" else packed.to(tdt)
            clips = list(torch.split(packed, n_in))
            row = dict(kind=kind, name=name, seconds=[lo, hi], clips=n_clips, frames=total, modes={}, sums_equal=True, refusal=None)
            if args.shape:
                log_path = os.environ.get("HIPSOXR_DEBUG_LAUNCH_LOG")
                assert log_path, "--shape reads HIPSOXR_DEBUG_LAUNCH_LOG (debug-switch build)"
                log_pos = os.path.getsize(log_path) if os.path.exists(log_path) else 0
                job = dist.RaggedJob(plan, clips, kernel=by_name)
                job.launch()
                torch.cuda.synchronize()
                with open(log_path) as fh:
                    fh.seek(log_pos)
                    lines = [dict(tok.split("=", 1) for tok in ln.split()) for ln in fh.read().split("\n") if ln.startswith("form=")]
                assert len(lines) == 1 and "ragged" in lines[0], lines
                form, hop = lines[0]["form"], int(lines[0]["hop_out"])
                row.update(form=form, hop_out=hop, own=xcd_balance(job.n_out, hop, form == "strided2_cp", True),
                           longest=xcd_balance(job.n_out, hop, form == "strided2_cp", False))
                print("%-34s %4g-%-4g s %5d clips  %s hop_out %d  busiest XCD / mean: own %.3f, longest %.3f" % (name, lo, hi, n_clips, form, hop, row["own"], row["longest"]), flush=True)
                rows.append(row)
                del job, clips, packed
                torch.cuda.empty_cache()
                continue

            def table_mode(kernel):
                job = dist.RaggedJob(plan, clips, kernel=kernel)
                try:
                    job.launch()
                except RuntimeError as e:
                    row["refusal"] = str(e)
                    return None
                torch.cuda.synchronize()
                first = float(job.y.to(torch.float64).sum().item())
                ts = timed(job.launch, args.reps, torch)
                row["sums_equal"] = row["sums_equal"] and first == float(job.y.to(torch.float64).sum().item())
                return ts
            if kind == "two-stage":
                row["modes"]["table"] = table_mode(_native.KERNEL_AUTO)
            else:
                kw = dict(kernel=by_name, dither=True) if dtype == "int16" else dict(kernel=by_name)
                row["modes"]["table"] = table_mode(by_name)
                row["modes"]["loop"] = timed(lambda: [dev.resample_tensor(plan, c, **kw) for c in clips], args.reps, torch)
                row["modes"]["exact"] = table_mode(_native.KERNEL_EXACT)
            print("%-34s %4g-%-4g s %5d clips %10d frames  %s  sums %s" % (name, lo, hi, n_clips, total, "  ".join("%s %s" % (m, fmt(t)) for m, t in row["modes"].items()),
                                                                      "equal" if row["sums_equal"] else "DIFFER"), flush=True)
            if row["refusal"]:
                print("    refused: " + row["refusal"], flush=True)
            rows.append(row)
            del clips, packed
            torch.cuda.empty_cache()
    path = args.shape or args.json
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump(dict(library=_native.LIB_PATH, rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
