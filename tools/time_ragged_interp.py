#!/usr/bin/env python3
"""Ragged batches on interpolated-phase plans (arbitrary ratios): what `dist.RaggedJob.launch()` costs for the jobs the exact
engine serves on such a plan — one launch of the RAGGED form of k_interp_tile / k_interp_wave / k_interp over the clip table,
where the parent commit's library ran one launch per clip inside the same C call.  The yardstick is the PARENT's library
running the very same calls, not a loop written here: run this tool once per library (HIPSOXR_LIBRARY selects it) with
--json, then merge the two records into a table (tools/time_ragged_exact.py is the same tool for exact-bank plans).

Workloads at 48000 -> 44101 VHQ: 64 and 1024 clips, lengths uniform (seeded) in 1 to 10 s and in 0.1 to 1 s, clips views of
one packed buffer:
    int16 mono                        (default selector: integers are pinned to the canonical order)
    float32 stereo interleaved        KERNEL_EXACT
Per repetition one `launch()` is timed between two HIP events on the current stream — host-side work between the launches
of a per-clip loop included — median over the repetitions (min-max in brackets).  The result of the first launch is hashed
(sum of the packed output as int64 / float64) so that the two records can be checked to have computed the same.  GPU only.

    HIPSOXR_LIBRARY=<parent build>/libhipsoxr.so python tools/time_ragged_interp.py --json parent.json
    python tools/time_ragged_interp.py --json this.json
    python tools/time_ragged_interp.py --merge parent.json this.json --out profiles/ragged_interp_rows.md

--merge also states the acceptance per row: the one launch must not exceed the parent's median by more than the larger of
the two min-max spreads."""
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

# name, in rate, out rate, quality, dtype, channels, selector (None: the default)
WORKLOADS = [("48000->44101 VHQ int16 mono", 48000, 44101, "VHQ", "int16", 1, None),
             ("48000->44101 VHQ float32 stereo", 48000, 44101, "VHQ", "float32", 2, "KERNEL_EXACT")]
RANGES = [(1.0, 10.0), (0.1, 1.0)]  # shortest and longest clip, seconds


def merge(parent_path, this_path, out):
    with open(parent_path) as f:
        a = json.load(f)
    with open(this_path) as f:
        b = json.load(f)
    lines = ["| workload | clip lengths, s | clips | frames in all | parent (launch per clip), us | one ragged launch, us | parent / this | accepted |",
             "|---|---|---|---|---|---|---|---|"]
    for ra, rb in zip(a["rows"], b["rows"]):
        assert (ra["name"], ra["seconds"], ra["clips"], ra["frames"]) == (rb["name"], rb["seconds"], rb["clips"], rb["frames"])
        assert ra["checksum"] == rb["checksum"], "the two libraries computed different results: %r" % ra["name"]
        spread = max(ra["max"] - ra["min"], rb["max"] - rb["min"])
        ok = rb["median"] <= ra["median"] + spread
        lines.append("| %s | %g-%g | %d | %d | %.0f (%.0f-%.0f) | %.0f (%.0f-%.0f) | %.2f | %s |" % (
            ra["name"], ra["seconds"][0], ra["seconds"][1], ra["clips"], ra["frames"], ra["median"], ra["min"], ra["max"], rb["median"], rb["min"], rb["max"],
            ra["median"] / rb["median"], "yes" if ok else "NO"))
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", help="write this library's rows here")
    ap.add_argument("--merge", nargs=2, metavar=("PARENT", "THIS"), help="two --json records -> a markdown table")
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--clips", type=int, nargs="*", default=[64, 1024])
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge[0], args.merge[1], args.out)
    import torch
    assert torch.cuda.is_available(), "time_ragged_interp.py needs a GPU"
    from soxr_amd import _native, device as dev, dist

    rows = []
    for name, fi, fo, q, dtype, ch, sel in WORKLOADS:
        plan = dev.Plan(fi, fo, q)
        assert plan.phases != 0, "an interpolated-phase plan"
        kernel = getattr(_native, sel) if sel else _native.KERNEL_AUTO
        tdt = getattr(torch, dtype)
        for lo, hi in RANGES:
            for n_clips in args.clips:
                rng = np.random.default_rng(n_clips)
                n_in = [int(v) for v in rng.integers(int(lo * fi), int(hi * fi) + 1, n_clips)]
                total = sum(n_in)
                g = torch.Generator(device="cuda").manual_seed(n_clips)
                if tdt.is_floating_point:
                    packed = (torch.rand((total, ch), dtype=torch.float32, device="cuda", generator=g) - 0.5).to(tdt)
                else:
                    packed = torch.randint(-8000, 8000, (total, ch), dtype=torch.int32, device="cuda", generator=g).to(tdt)
                clips = list(torch.split(packed, n_in))
                job = dist.RaggedJob(plan, clips, kernel=kernel)
                job.launch()
                torch.cuda.synchronize()
                checksum = float(job.y.to(torch.float64).sum().item()) if tdt.is_floating_point else int(job.y.to(torch.int64).sum().item())
                for _ in range(2):
                    job.launch()
                torch.cuda.synchronize()
                ts = []
                for _ in range(args.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    job.launch()
                    e1.record()
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1) * 1e3)  # us
                rows.append(dict(name=name, seconds=[lo, hi], clips=n_clips, frames=total, checksum=checksum, median=statistics.median(ts), min=min(ts),
                                 max=max(ts)))
                print("%-34s %4g-%-4g s %5d clips  %10d frames  %.0f us (%.0f-%.0f)" % (name, lo, hi, n_clips, total, rows[-1]["median"], min(ts), max(ts)),
                      flush=True)
                del job, clips, packed
                torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(dict(library=_native.LIB_PATH, rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
