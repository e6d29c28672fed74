#!/usr/bin/env python3
"""The adjoint on the frequency-domain engine (kernel=KERNEL_ADJOINT_FFT, csrc/adjoint_fft.hip) against the exact engine's
adjoint (KERNEL_AUTO: k_adj_tile / k_adj_gather) and against the forward under KERNEL_FFT, at equal shape.

Rows: the four of profiles/NOTES_adjoint.md — 60 s mono 48k -> 44.1k VHQ float32; the same in float64; 128 clips x 10 s
float32; 10 s x 8 channels interleaved 44.1k -> 16k float32 — and a ragged table of 64 mono clips of 1 .. 10 s (48k -> 44.1k
VHQ float32; one launch each way).  A fifth column times what the adjoint is expected to cost: the FORWARD under KERNEL_FFT of
the reversed ratio on the cotangent's shape (the transposed plan is that plan with a longer filter).  Per row all kinds run on
the same tensors (x -> y, y -> gx): HIP-event time over blocks of launches, the kinds alternated block by block, median of
the blocks (min-max in brackets); tensors are warmed first.  Prints a markdown table (also to --out).  GPU only.

    python tools/time_adjoint_fft.py --out profiles/adjoint_fft_rows.md [--blocks 9] [--launches 20]
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

ROWS = [("60 s mono 48k->44.1k VHQ f32", 48000, 44100, "VHQ", "float32", (60 * 48000,)),
        ("60 s mono 48k->44.1k VHQ f64", 48000, 44100, "VHQ", "float64", (60 * 48000,)),
        ("128 clips x 10 s 48k->44.1k VHQ f32", 48000, 44100, "VHQ", "float32", (128, 10 * 48000, 1)),
        ("10 s x 8 ch interleaved 44.1k->16k VHQ f32", 44100, 16000, "VHQ", "float32", (10 * 44100, 8)),
        ("ragged: 64 mono clips of 1-10 s 48k->44.1k VHQ f32", 48000, 44100, "VHQ", "float32", None)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rows", type=int, nargs="*", help="row indices (default: all)")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "time_adjoint_fft.py needs a GPU"
    from soxr_amd import device as dev, dist
    K = dev.KERNEL_ADJOINT_FFT

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.launches  # us per launch

    def equal_length(fi, fo, q, dt, shape):
        plan, rev = dev.Plan(fi, fo, q), dev.Plan(fo, fi, q)
        x = torch.randn(*shape, dtype=getattr(torch, dt), device="cuda") * 0.25
        frames = shape[0] if len(shape) < 3 else shape[1]
        y = dev.resample_tensor(plan, x, kernel=dev.KERNEL_FFT)
        gx, gx2 = torch.empty_like(x), torch.empty_like(x)
        r = dev.resample_tensor(rev, y, kernel=dev.KERNEL_FFT)  # the reversed ratio on the cotangent's shape
        kinds = {"fwd": lambda: dev.resample_tensor(plan, x, out=y, kernel=dev.KERNEL_FFT),
                 "exact": lambda: dev.resample_tensor_adjoint(plan, y, frames, out=gx2, kernel=dev.KERNEL_AUTO),
                 "fft": lambda: dev.resample_tensor_adjoint(plan, y, frames, out=gx, kernel=K),
                 "rev": lambda: dev.resample_tensor(rev, y, out=r, kernel=dev.KERNEL_FFT)}
        return plan, kinds, (gx, gx2)

    def ragged(fi, fo, q, dt):
        plan, rev = dev.Plan(fi, fo, q), dev.Plan(fo, fi, q)
        rng = np.random.default_rng(64)
        n_x = [int(n) for n in rng.integers(1 * fi, 10 * fi + 1, 64)]
        clips = [torch.randn(n, dtype=getattr(torch, dt), device="cuda") * 0.25 for n in n_x]
        job = dist.RaggedJob(plan, clips, kernel=dev.KERNEL_FFT)
        job.launch()
        gys = [g.clone() for g in job.outputs()]
        n_y = [int(g.shape[0]) for g in gys]
        # the adjoint's table over one packed cotangent and one packed gradient, uploaded once (as RaggedJob's is)
        gy_all, gx = torch.cat(gys), torch.empty(sum(n_x), dtype=clips[0].dtype, device="cuda")
        gx2 = torch.empty_like(gx)
        off = lambda ns: np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64)
        table = np.ascontiguousarray(np.stack([off(n_y), n_y, off(n_x), n_x], axis=1), dtype=np.int64)
        tdev = torch.from_numpy(table).cuda()
        elem, st = dev._torch_elem(gx.dtype), torch.cuda.current_stream().cuda_stream
        rjob = dist.RaggedJob(rev, gys, kernel=dev.KERNEL_FFT)
        kinds = {"fwd": job.launch,
                 "exact": lambda: plan.run_adjoint_ragged(gy_all.data_ptr(), gx2.data_ptr(), elem, 1, table, (1, 1), (1, 1), stream=st,
                                                          kernel=dev.KERNEL_AUTO, table_dev=tdev.data_ptr()),
                 "fft": lambda: plan.run_adjoint_ragged(gy_all.data_ptr(), gx.data_ptr(), elem, 1, table, (1, 1), (1, 1), stream=st,
                                                        kernel=K, table_dev=tdev.data_ptr()),
                 "rev": rjob.launch}
        return plan, kinds, (gx, gx2)

    lines = ["| job | taps -> T' | forward KERNEL_FFT, us | exact adjoint (AUTO), us | ADJOINT_FFT, us | forward KERNEL_FFT of the reversed ratio, us | exact / ADJOINT_FFT | ADJOINT_FFT / forward | rel. RMS vs exact |",
             "|---|---|---|---|---|---|---|---|---|"]
    for i, (name, fi, fo, q, dt, shape) in enumerate(ROWS):
        if args.rows and i not in args.rows:
            continue
        plan, kinds, (gx, gx2) = ragged(fi, fo, q, dt) if shape is None else equal_length(fi, fo, q, dt, shape)
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
        tt = (2 * -(-(plan.L * (plan.taps // 2) + 1) // plan.M) + 7) // 8 * 8
        lines.append("| %s | %d -> %d | %s | %s | %s | %s | %.2f | %.2f | %.2g |" % (name, plan.taps, tt, cell("fwd"), cell("exact"), cell("fft"), cell("rev"),
                                                                              med["exact"] / med["fft"], med["fft"] / med["fwd"], rel))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
