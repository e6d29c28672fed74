#!/usr/bin/env python3
"""The transposed operator (hipsoxr_run_device_adjoint, csrc/adjoint.hip) against the forward exact engine at equal shape —
equal multiply-add count: n_out * taps per column either way.

Rows: 60 s mono 48k -> 44.1k VHQ float32; the same in float64; 128 clips x 10 s float32; 10 s x 8 channels interleaved
44.1k -> 16k float32; then the interpolated-phase plans (kernel=KERNEL_ADJOINT, k_adj_interp): 60 s mono and stereo
48000 -> 44101 VHQ and 10 s x 8 channels 44100 -> 16000.5 VHQ, each in float32 and float64, against the forward exact engine
on the same plan and shape (k_interp_tile / k_interp_wave / k_interp).  Per row the forward job (kernel=KERNEL_EXACT) and the adjoint job run on the same tensors (x -> y,
y -> gx): HIP-event time over blocks of launches, the two kinds alternated, median of the blocks; tensors are warmed first.
Prints a markdown table (also to --out).  GPU only.

    python tools/time_adjoint.py --out profiles/adjoint_rows.md [--blocks 7] [--launches 20]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "python-soxr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

ROWS = [("60 s mono 48k->44.1k VHQ f32", 48000, 44100, "VHQ", "float32", (60 * 48000,)),
        ("60 s mono 48k->44.1k VHQ f64", 48000, 44100, "VHQ", "float64", (60 * 48000,)),
        ("128 clips x 10 s 48k->44.1k VHQ f32", 48000, 44100, "VHQ", "float32", (128, 10 * 48000, 1)),
        ("10 s x 8 ch interleaved 44.1k->16k VHQ f32", 44100, 16000, "VHQ", "float32", (10 * 44100, 8)),
        ("interp 60 s mono 48000->44101 VHQ f32", 48000, 44101, "VHQ", "float32", (60 * 48000,)),
        ("interp 60 s mono 48000->44101 VHQ f64", 48000, 44101, "VHQ", "float64", (60 * 48000,)),
        ("interp 60 s stereo 48000->44101 VHQ f32", 48000, 44101, "VHQ", "float32", (60 * 48000, 2)),
        ("interp 60 s stereo 48000->44101 VHQ f64", 48000, 44101, "VHQ", "float64", (60 * 48000, 2)),
        ("interp 10 s x 8 ch 44100->16000.5 VHQ f32", 44100, 16000.5, "VHQ", "float32", (10 * 44100, 8)),
        ("interp 10 s x 8 ch 44100->16000.5 VHQ f64", 44100, 16000.5, "VHQ", "float64", (10 * 44100, 8))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rows", type=int, nargs="*", help="row indices (default: all)")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "time_adjoint.py needs a GPU"
    from soxr_amd import device as dev

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.launches  # us per launch

    lines = ["| job | taps | forward exact, us | adjoint, us | adjoint / forward | adjoint GFMA/s |", "|---|---|---|---|---|---|"]
    for i, (name, fi, fo, q, dt, shape) in enumerate(ROWS):
        if args.rows and i not in args.rows:
            continue
        plan = dev.Plan(fi, fo, q)
        x = torch.randn(*shape, dtype=getattr(torch, dt), device="cuda") * 0.25
        frames = shape[0] if len(shape) < 3 else shape[1]
        y = dev.resample_tensor(plan, x, kernel=dev.KERNEL_EXACT)
        gx = torch.empty_like(x)
        fwd = lambda: dev.resample_tensor(plan, x, out=y, kernel=dev.KERNEL_EXACT)
        sel = dev.KERNEL_ADJOINT if plan.phases else dev.KERNEL_AUTO  # (interpolated-phase plans: by name)
        adj = lambda: dev.resample_tensor_adjoint(plan, y, frames, out=gx, kernel=sel)
        for _ in range(3):
            fwd(), adj()
        torch.cuda.synchronize()
        tf, ta = [], []
        for _ in range(args.blocks):
            tf.append(block(fwd))
            ta.append(block(adj))
        f, a = statistics.median(tf), statistics.median(ta)
        fma = y.numel() * plan.taps  # multiply-adds of the operator, either direction
        lines.append("| %s | %d | %.1f (%.1f-%.1f) | %.1f (%.1f-%.1f) | %.2f | %.0f |"
                     % (name, plan.taps, f, min(tf), max(tf), a, min(ta), max(ta), a / f, fma / a * 1e-3))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
