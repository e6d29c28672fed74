#!/usr/bin/env python3
"""Speed perturbation, a factor per clip: the one-launch form against the two loops it replaces (profiles/NOTES_varispeed.md).

Contestants per row, timed between two HIP events on the current stream, INTERLEAVED in one process (A B C D A B C D ...: what
disturbs one disturbs all), after a warm-up of every contestant; median of --steps:

  varispeed  one `dist.resample_varispeed(plan, clips, factors)` call on a variable-rate plan designed for the largest factor:
             the clip and clock tables built and uploaded, ONE launch
  prepared   the same job built once (`dist.RaggedJob(..., io_ratios=factors)`): `launch()` alone
  streams    one variable-rate `TensorStream` per clip (made beforehand): clear, set_io_ratio, resample_chunk(last=True)
  plans      what a pipeline with THREE factors (0.9, 1.0, 1.1) does today: one constant-rate plan per factor, the batch
             regrouped by factor, one prepared `RaggedJob(kernel=KERNEL_EXACT)` per factor — three launches; the clips keep
             their lengths but take the nearest of the three factors (it cannot serve continuous factors at all)

Rows: 64 and 1024 mono clips of 1-10 s at 16 kHz, factors uniform in [0.9, 1.1], HQ and VHQ, float32 and int16.  An event pair
around host-driven work measures the host too wherever the GPU waits for it: that is the point of the comparison.
--forms: no timing; one launch per row on the debug-switch build (HIPSOXR_LIBRARY, HIPSOXR_DEBUG_LAUNCH_LOG) and the launch
log's kernel names.  GPU only.

    python tools/varispeed_time.py --warmup 3 --steps 50 --json out.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "python-soxr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

RATE = 16000
THREE = (0.9, 1.0, 1.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--clips", type=int, nargs="*", default=[64, 1024])
    ap.add_argument("--forms", action="store_true")
    ap.add_argument("--json")
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "varispeed_time.py needs a GPU"
    from soxr_amd import _native, device as dev, dist

    log_path = os.environ.get("HIPSOXR_DEBUG_LAUNCH_LOG")
    rows = []
    for quality in ("HQ", "VHQ"):
        plan = dev.Plan(max(THREE) * RATE, RATE, quality, vr=True)
        three = [dev.Plan(f * RATE, RATE, quality) for f in THREE]
        for dtype in (torch.float32, torch.int16):
            for n in args.clips:
                rng = np.random.default_rng(n)
                lengths = rng.integers(RATE, 10 * RATE + 1, n)
                factors = rng.uniform(0.9, 1.1, n)
                g = torch.Generator(device="cuda").manual_seed(n)
                buf = torch.randn(int(lengths.sum()), dtype=torch.float32, device="cuda", generator=g) * 0.1
                if dtype == torch.int16:
                    buf = (buf * 32767).to(torch.int16)
                ends = np.cumsum(lengths)
                clips = [buf[int(e - m):int(e)] for e, m in zip(ends, lengths)]
                ratios = [float(f) for f in factors]
                job = dist.RaggedJob(plan, clips, io_ratios=ratios)
                if args.forms:
                    assert log_path, "--forms reads HIPSOXR_DEBUG_LAUNCH_LOG (the debug-switch build writes it)"
                    torch.cuda.synchronize()
                    pos = os.path.getsize(log_path) if os.path.exists(log_path) else 0
                    job.launch()
                    torch.cuda.synchronize()
                    with open(log_path) as fh:
                        fh.seek(pos)
                        lines = [ln.strip() for ln in fh.read().split("\n") if ln.strip()]
                    print("%s %s %d clips: %s" % (quality, str(dtype).split(".")[1], n, " | ".join(lines)), flush=True)
                    rows.append(dict(quality=quality, dtype=str(dtype).split(".")[1], clips=n, launches=lines))
                    continue
                streams = [dev.TensorStream(plan.in_rate, plan.out_rate, 1, dtype, quality, vr=True) for _ in clips]
                nearest = [min(range(3), key=lambda k: abs(THREE[k] - f)) for f in factors]
                jobs3 = [dist.RaggedJob(three[k], [c for c, q in zip(clips, nearest) if q == k], kernel=_native.KERNEL_EXACT) for k in range(3)]

                def varispeed():
                    dist.resample_varispeed(plan, clips, ratios)

                def per_stream():
                    for ts, c, r in zip(streams, clips, ratios):
                        ts.clear()
                        ts.set_io_ratio(r, 1.0)
                        ts.resample_chunk(c, last=True)

                def per_plan():
                    for j3 in jobs3:
                        j3.launch()

                contestants = [("varispeed", varispeed), ("prepared", job.launch), ("streams", per_stream), ("plans", per_plan)]
                for _ in range(args.warmup):
                    for _, fn in contestants:
                        fn()
                torch.cuda.synchronize()
                ts_ = {k: [] for k, _ in contestants}
                for _ in range(args.steps):
                    for k, fn in contestants:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        fn()
                        e1.record()
                        e1.synchronize()
                        ts_[k].append(e0.elapsed_time(e1) * 1e3)  # us
                torch.cuda.synchronize()
                row = dict(quality=quality, dtype=str(dtype).split(".")[1], clips=n, in_frames=int(lengths.sum()), outputs=int(sum(job.n_out)),
                           us={k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in ts_.items()})
                rows.append(row)
                print("%-3s %-7s %5d clips  " % (quality, row["dtype"], n) +
                      "  ".join("%s %.0f us (%.0f-%.0f)" % (k, row["us"][k]["median"], row["us"][k]["min"], row["us"][k]["max"]) for k, _ in contestants) +
                      "  streams / varispeed %.1f  plans / varispeed %.2f" % (row["us"]["streams"]["median"] / row["us"]["varispeed"]["median"],
                                                                            row["us"]["plans"]["median"] / row["us"]["varispeed"]["median"]), flush=True)
                del streams, jobs3
                torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(dict(library=_native.LIB_PATH, warmup=args.warmup, steps=args.steps, rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
