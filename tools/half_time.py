#!/usr/bin/env python3
"""float16 device jobs against float32 ones and against the caller's own conversions (profiles/NOTES_half.md).

Three contestants per shape, each one `launch()` of prepared work on preallocated tensors, timed between two HIP events on
the current stream, INTERLEAVED in one process (A B C A B C ...: what disturbs one disturbs all), after a warm-up of every
contestant:

  fused    the float16 job (conversion fused into k_fft_pair2: 2 + 2.18 algorithmic bytes per output at 48k -> 44.1k)
  float32  the float32 job of the same shape (4 + 4.35)
  three    what a caller wrote before there were half jobs: x.float() -> float32 job -> .half(), as two copy_ kernels
           around the float32 job on preallocated tensors (no allocator in the window: the three launches alone)

Shapes: the 128 x 10 s batch and the 60 s mono clip, VHQ, 48k -> 44.1k and 44.1k -> 48k (there the float32 batch runs the
one-wave kernel and the float16 batch stays on k_fft_pair2).  Reported per row: median (min-max) in microseconds, the
algorithmic bytes per output sample, and whether `fused` and `three` gave the same bits — they must wherever float32 and
float16 take the same kernel form (not on the 44.1k -> 48k batch).  GPU only.

    python tools/half_time.py --warmup 5 --steps 50 --json out.json"""
import argparse
import json
import os
import statistics
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "python-soxr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = [("128 x 10 s", 128, 10.0), ("1 x 60 s", 1, 60.0)]
RATES = [(48000, 44100), (44100, 48000)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--dtype", default="float16", choices=["float16", "bfloat16"])
    ap.add_argument("--json")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "half_time.py needs a GPU"
    from soxr_amd import _native, device as dev
    hdt = getattr(torch, args.dtype)

    rows = []
    for fi, fo in RATES:
        plan = dev.Plan(fi, fo, "VHQ")
        for name, clips, seconds in SHAPES:
            frames = int(seconds * fi)
            n_out = plan.out_len(frames)
            g = torch.Generator(device="cuda").manual_seed(clips)
            xh = (torch.randn((clips, frames, 1), dtype=torch.float32, device="cuda", generator=g) * 0.1).to(hdt)
            xf = xh.float()
            yh, yf = torch.empty((clips, n_out, 1), dtype=hdt, device="cuda"), torch.empty((clips, n_out, 1), dtype=torch.float32, device="cuda")
            xf3, yf3, yh3 = torch.empty_like(xf), torch.empty_like(yf), torch.empty_like(yh)
            job_h, job_f, job_3 = dev.PreparedJob(plan, xh, yh), dev.PreparedJob(plan, xf, yf), dev.PreparedJob(plan, xf3, yf3)

            def three():
                xf3.copy_(xh)
                job_3.launch()
                yh3.copy_(yf3)

            contestants = [("fused", job_h.launch), ("float32", job_f.launch), ("three", three)]
            for _ in range(args.warmup):
                for _, fn in contestants:
                    fn()
            torch.cuda.synchronize()
            ts = {k: [] for k, _ in contestants}
            for _ in range(args.steps):
                for k, fn in contestants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    ts[k].append(e0.elapsed_time(e1) * 1e3)  # us
            torch.cuda.synchronize()
            same = bool(torch.equal(yh.view(torch.int16), yh3.view(torch.int16)))
            worst = float((yh.float() - yh3.float()).abs().max().item())
            r = fi / fo
            row = dict(rates=[fi, fo], shape=name, dtype=args.dtype, outputs=clips * n_out, same_bits=same, max_abs_diff=worst,
                       bytes_per_output=dict(fused=2 * r + 2, float32=4 * r + 4, three=(2 + 4) * r + (4 * r + 4) + (4 + 2)),
                       us={k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in ts.items()})
            rows.append(row)
            print("%d -> %d  %-10s %s  " % (fi, fo, name, args.dtype) +
                  "  ".join("%s %.1f us (%.1f-%.1f)" % (k, row["us"][k]["median"], row["us"][k]["min"], row["us"][k]["max"]) for k, _ in contestants) +
                  "  fused / float32 %.2f  fused / three %.2f  bits %s (max |diff| %.2e)" % (
                      row["us"]["fused"]["median"] / row["us"]["float32"]["median"], row["us"]["fused"]["median"] / row["us"]["three"]["median"],
                      "same" if same else "DIFFER", worst), flush=True)
            del job_h, job_f, job_3, xh, xf, yh, yf, xf3, yf3, yh3
            torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(dict(library=_native.LIB_PATH, warmup=args.warmup, steps=args.steps, rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
