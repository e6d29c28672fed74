#!/usr/bin/env python3
"""Gradients of a ragged batch: ONE launch over a clip table (dist.resample_ragged_adjoint ->
hipsoxr_run_device_adjoint_ragged) against what a caller had before it — a Python loop of device.resample_tensor_adjoint
calls, one launch per clip.

Batches: 64 and 1024 mono float32 clips of 1 to 10 s at 48 kHz (lengths uniform, seeded), on 48000 -> 44100 VHQ (exact bank:
k_adj_tile) and 48000 -> 44101 VHQ (interpolated phases, kernel=KERNEL_ADJOINT: k_adj_interp).  Both contenders read the same
cotangent views of one packed buffer.  Per repetition the loop and the ragged call are each timed once between two HIP
events on the current stream — the time a training step sees, host-side work between launches included — the two alternated,
median over the repetitions (min-max in brackets).  A third column times the raw launch alone (Plan.run_adjoint_ragged on a
prepared table with a device copy, output buffer reused): the kernel without the Python around it.  Results are compared
bit for bit before anything is timed.  Prints a markdown table (also to --out).  GPU only.

    python tools/time_adjoint_ragged.py --out profiles/adjoint_ragged_rows.md [--reps 50] [--clips 64 1024]
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

PLANS = [("48000->44100 VHQ", 48000, 44100, "VHQ"), ("48000->44101 VHQ", 48000, 44101, "VHQ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--clips", type=int, nargs="*", default=[64, 1024])
    ap.add_argument("--seconds", type=float, nargs=2, default=[1.0, 10.0], help="shortest and longest clip")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "time_adjoint_ragged.py needs a GPU"
    from soxr_amd import _native, device as dev, dist

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3  # us

    def cell(ts):
        return "%.0f (%.0f-%.0f)" % (statistics.median(ts), min(ts), max(ts))

    lines = ["| plan | clips | frames in all | longest / mean clip | loop of launches, us | one ragged call, us | loop / ragged | raw ragged launch, us |",
             "|---|---|---|---|---|---|---|---|"]
    for name, fi, fo, q in PLANS:
        plan = dev.Plan(fi, fo, q)
        sel = dev.KERNEL_ADJOINT if plan.phases else dev.KERNEL_AUTO
        for n_clips in args.clips:
            rng = np.random.default_rng(n_clips)
            n_x = [int(v) for v in rng.integers(int(args.seconds[0] * fi), int(args.seconds[1] * fi) + 1, n_clips)]
            n_y = [plan.out_len(n) for n in n_x]
            packed = torch.randn(sum(n_y), dtype=torch.float32, device="cuda") * 0.25
            gys = list(torch.split(packed, n_y))
            loop = lambda: [dev.resample_tensor_adjoint(plan, g, n, kernel=sel) for g, n in zip(gys, n_x)]
            ragged = lambda: dist.resample_ragged_adjoint(plan, gys, n_x, kernel=sel)
            # the raw launch: table and its device copy prepared once, the output buffer reused
            gx = torch.empty(sum(n_x), dtype=torch.float32, device="cuda")
            table = np.stack([np.concatenate([[0], np.cumsum(n_y)[:-1]]), n_y, np.concatenate([[0], np.cumsum(n_x)[:-1]]), n_x],
                             axis=1).astype(np.int64)
            table_dev = torch.from_numpy(table).cuda()
            stream = torch.cuda.current_stream().cuda_stream
            raw = lambda: plan.run_adjoint_ragged(packed.data_ptr(), gx.data_ptr(), _native.F32, 1, table, (1, 1), (1, 1),
                                                  stream=stream, kernel=sel, table_dev=table_dev.data_ptr())
            a, b = loop(), ragged()  # (warm-up, and the check: the same bits)
            raw()
            torch.cuda.synchronize()
            assert all(torch.equal(u, v) for u, v in zip(a, b)) and torch.equal(torch.cat(b), gx), "ragged and per-clip results differ"
            del a, b
            for _ in range(2):
                loop(), ragged(), raw()
            torch.cuda.synchronize()
            tl, tr, tk = [], [], []
            for _ in range(args.reps):
                tl.append(timed(loop))
                tr.append(timed(ragged))
                tk.append(timed(raw))
            lines.append("| %s | %d | %d | %.2f | %s | %s | %.2f | %s |"
                         % (name, n_clips, sum(n_x), max(n_x) / (sum(n_x) / n_clips), cell(tl), cell(tr),
                            statistics.median(tl) / statistics.median(tr), cell(tk)))
            print(lines[-1], flush=True)
            del packed, gys, gx
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
