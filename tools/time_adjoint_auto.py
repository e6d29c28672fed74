#!/usr/bin/env python3
"""KERNEL_ADJOINT_AUTO on a clip table of an interpolated-phase plan (csrc/twostage.hip launch_adjoint_two_stage_ragged: per range
one ragged k_poly_adj launch and one FFT-stage launch, whatever the number of clips) against what a caller had before it:
the ragged exact adjoint (KERNEL_ADJOINT: one k_adj_interp launch), the clip-by-clip loop of KERNEL_ADJOINT_TWO_STAGE, and —
the yardstick — the ragged forward under KERNEL_AUTO that the new launch transposes.  The expectation to confirm or refute:
the ragged forward's launch time multiplied by the 1.6-2.4 adjoint / forward ratio of profiles/NOTES_adjoint_two_stage.md.

Rows: 48000 -> 44101 VHQ; the corpora of tools/time_ragged_two_stage.py (lengths uniform in 1 to 10 s, seeded by the clip count):
64 and 1024 mono float32 clips, 64 interleaved stereo float32 clips, 64 mono float64 clips.  Per row all kinds run on the same
tensors: HIP-event time over blocks of launches — host-side work between the launches included — the kinds alternated block
by block, median of the blocks (min-max in brackets); tensors are warmed first.  The last column is the relative RMS of the new
launch's gradients against the ragged exact adjoint's.  Prints a markdown table (also to --out).  GPU only.

    python tools/time_adjoint_auto.py --out profiles/adjoint_auto_rows.md [--blocks 9] [--launches 5] [--rows 0 2 3]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "python-soxr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

ROWS = [("64 clips of 1-10 s mono f32", 64, 1, "float32"),
        ("1024 clips of 1-10 s mono f32", 1024, 1, "float32"),
        ("64 clips of 1-10 s stereo interleaved f32", 64, 2, "float32"),
        ("64 clips of 1-10 s mono f64", 64, 1, "float64")]
FI, FO, Q = 48000, 44101, "VHQ"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="*", help="row indices (default: all)")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "time_adjoint_auto.py needs a GPU"
    from soxr_amd import device as dev, dist

    def block(fn, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches  # us per launch

    lines = ["| table | frames in all | ragged forward KERNEL_AUTO, us | ragged KERNEL_ADJOINT (k_adj_interp), us | KERNEL_ADJOINT_TWO_STAGE clip by clip, us | ragged KERNEL_ADJOINT_AUTO, us | "
             "exact / AUTO | loop / AUTO | AUTO / forward | rel. RMS vs exact |", "|---|---|---|---|---|---|---|---|---|---|"]
    plan = dev.Plan(FI, FO, Q)
    for i, (name, n_clips, ch, dt) in enumerate(ROWS):
        if args.rows and i not in args.rows:
            continue
        tdt = getattr(torch, dt)
        rng = np.random.default_rng(n_clips)
        n_in = [int(v) for v in rng.integers(FI, 10 * FI + 1, n_clips)]
        g = torch.Generator(device="cuda").manual_seed(n_clips)
        packed = (torch.rand((sum(n_in), ch), dtype=torch.float32, device="cuda", generator=g) - 0.5).to(tdt)
        xs = [c[:, 0] if ch == 1 else c for c in torch.split(packed, n_in)]
        job = dist.RaggedJob(plan, xs)
        job.launch()
        gys = [y.detach() for y in job.outputs()]
        kinds = {"fwd": job.launch,
                 "exact": lambda: dist.resample_ragged_adjoint(plan, gys, n_in, kernel=dev.KERNEL_ADJOINT),
                 "loop": lambda: [dev.resample_tensor_adjoint(plan, gy, n, kernel=dev.KERNEL_ADJOINT_TWO_STAGE) for gy, n in zip(gys, n_in)],
                 "auto": lambda: dist.resample_ragged_adjoint(plan, gys, n_in, kernel=dev.KERNEL_ADJOINT_AUTO)}
        # the exact adjoint of 1024 clips takes a tenth of a second a launch: fewer launches per block for it
        launches = {k: (max(1, args.launches // 5) if k == "exact" and n_clips > 64 else args.launches) for k in kinds}
        for fn in kinds.values():
            fn()
        torch.cuda.synchronize()
        a, e = torch.cat([v.reshape(-1) for v in kinds["auto"]()]).double(), torch.cat([v.reshape(-1) for v in kinds["exact"]()]).double()
        rel = float((a - e).norm() / e.norm())
        del a, e
        t = {k: [] for k in kinds}
        for _ in range(args.blocks):
            for k, fn in kinds.items():
                t[k].append(block(fn, launches[k]))
        med = {k: statistics.median(v) for k, v in t.items()}
        cell = lambda k: "%.0f (%.0f-%.0f)" % (med[k], min(t[k]), max(t[k]))
        lines.append("| %s | %d | %s | %s | %s | %s | %.2f | %.2f | %.2f | %.2g |" % (name, sum(n_in), cell("fwd"), cell("exact"), cell("loop"), cell("auto"),
                                                                               med["exact"] / med["auto"], med["loop"] / med["auto"], med["auto"] / med["fwd"], rel))
        print(lines[-1], flush=True)
        del job, gys, xs, packed
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
