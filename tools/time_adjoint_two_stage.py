#!/usr/bin/env python3
"""The two-stage form's adjoint (kernel=KERNEL_ADJOINT_TWO_STAGE; csrc/twostage.hip k_poly_adj + the FFT stage's transposed
plan) against the exact adjoint of the same interpolated-phase plan (KERNEL_ADJOINT: k_adj_interp) and against the forward
under KERNEL_AUTO — the two-stage job it transposes — at equal shape.  The expectation to confirm or refute: the adjoint costs
what the forward two-stage job costs.

Rows: 60 s mono and stereo 48000 -> 44101 VHQ in float32 and float64; 60 s mono and stereo 44101 -> 48000 VHQ float32;
128 clips x 10 s mono 48000 -> 44101 VHQ float32.  Per row all kinds run on the same tensors (x -> y, y -> gx): HIP-event time
over blocks of launches, the kinds alternated block by block, median of the blocks (min-max in brackets); tensors are warmed
first.  The last column is the relative RMS of the new selector's gradient against the exact adjoint's.  Prints a markdown
table (also to --out).  GPU only.  (--launches-only N: N launches of each kind of the chosen rows and nothing else — the
target of a kernel trace, for the per-stage split.)

    python tools/time_adjoint_two_stage.py --out profiles/adjoint_two_stage_rows.md [--blocks 9] [--launches 20]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "python-soxr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

ROWS = [("60 s mono 48000->44101 VHQ f32", 48000, 44101, "VHQ", "float32", (60 * 48000,)),
        ("60 s stereo 48000->44101 VHQ f32", 48000, 44101, "VHQ", "float32", (60 * 48000, 2)),
        ("60 s mono 48000->44101 VHQ f64", 48000, 44101, "VHQ", "float64", (60 * 48000,)),
        ("60 s stereo 48000->44101 VHQ f64", 48000, 44101, "VHQ", "float64", (60 * 48000, 2)),
        ("60 s mono 44101->48000 VHQ f32", 44101, 48000, "VHQ", "float32", (60 * 44101,)),
        ("60 s stereo 44101->48000 VHQ f32", 44101, 48000, "VHQ", "float32", (60 * 44101, 2)),
        ("128 clips x 10 s mono 48000->44101 VHQ f32", 48000, 44101, "VHQ", "float32", (128, 10 * 48000, 1))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rows", type=int, nargs="*", help="row indices (default: all)")
    ap.add_argument("--launches-only", type=int, default=0)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "time_adjoint_two_stage.py needs a GPU"
    from soxr_amd import device as dev
    K = dev.KERNEL_ADJOINT_TWO_STAGE

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.launches  # us per launch

    lines = ["| job | forward KERNEL_AUTO (two-stage), us | exact adjoint KERNEL_ADJOINT, us | ADJOINT_TWO_STAGE, us | exact / ADJOINT_TWO_STAGE | ADJOINT_TWO_STAGE / forward | rel. RMS vs exact |",
             "|---|---|---|---|---|---|---|"]
    for i, (name, fi, fo, q, dt, shape) in enumerate(ROWS):
        if args.rows and i not in args.rows:
            continue
        plan = dev.Plan(fi, fo, q)
        x = torch.randn(*shape, dtype=getattr(torch, dt), device="cuda") * 0.25
        frames = shape[0] if len(shape) < 3 else shape[1]
        y = dev.resample_tensor(plan, x)
        assert not torch.equal(y, dev.resample_tensor(plan, x, kernel=dev.KERNEL_EXACT)), "AUTO ran the exact engine: not the two-stage form"
        gx, gx2 = torch.empty_like(x), torch.empty_like(x)
        kinds = {"fwd": lambda: dev.resample_tensor(plan, x, out=y),
                 "exact": lambda: dev.resample_tensor_adjoint(plan, y, frames, out=gx2, kernel=dev.KERNEL_ADJOINT),
                 "two": lambda: dev.resample_tensor_adjoint(plan, y, frames, out=gx, kernel=K)}
        if args.launches_only:
            for fn in kinds.values():
                for _ in range(args.launches_only):
                    fn()
            torch.cuda.synchronize()
            continue
        for _ in range(3):
            for fn in kinds.values():
                fn()
        torch.cuda.synchronize()
        rel = float((gx.double() - gx2.double()).norm() / gx2.double().norm())
        t = {k: [] for k in kinds}
        for _ in range(args.blocks):
            for k, fn in kinds.items():
                t[k].append(block(fn))
        med = {k: statistics.median(v) for k, v in t.items()}
        cell = lambda k: "%.1f (%.1f-%.1f)" % (med[k], min(t[k]), max(t[k]))
        lines.append("| %s | %s | %s | %s | %.2f | %.2f | %.2g |" % (name, cell("fwd"), cell("exact"), cell("two"), med["exact"] / med["two"], med["two"] / med["fwd"], rel))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
