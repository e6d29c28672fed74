#!/usr/bin/env python3
"""The gradient of speed perturbation with a factor per clip: the one-launch adjoint against the forward it transposes and
against the loop it replaces (profiles/NOTES_varispeed_adjoint.md).

Contestants per row, timed between two HIP events on the current stream, INTERLEAVED in one process (A B C D A B C D ...: what
disturbs one disturbs all), after a warm-up of every contestant; median of --steps with min-max:

  forward   the prepared varispeed forward at equal shape (`dist.RaggedJob(..., io_ratios=factors).launch()`): ONE launch
  adjoint   the new entry on a prepared table (`Plan.run_vr_ragged_adjoint` with a device copy of the table): the clock table
            uploaded, ONE launch of k_adj_interp's variable-rate form over all clips
  operator  `dist.resample_varispeed_adjoint(plan, gys, in_frames, factors)`: the same with the table built, the result
            allocated and the clip table uploaded on every call — what a backward pass calls
  loop      a per-clip loop of one-row tables through the same entry: what serves this gradient without the one-launch form

Rows: 64 and 1024 mono clips of 1-10 s at 16 kHz, factors uniform in [0.9, 1.1], HQ and VHQ, float32 and float64.  An event
pair around host-driven work measures the host too wherever the GPU waits for it: that is the point of the loop's figure.
Each row also states the launch's grid and the share of its workgroups that leave at the skip test (a tile at or behind its
clip's n_x): the grid's frame axis is the LONGEST clip's.
--forms: no timing; one launch per row on the debug-switch build (HIPSOXR_LIBRARY, HIPSOXR_DEBUG_LAUNCH_LOG) and the launch
log's line.  GPU only.

    python tools/varispeed_adjoint_time.py --warmup 3 --steps 50 --json out.json"""
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
TOP = 1.1


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
    assert torch.cuda.is_available(), "varispeed_adjoint_time.py needs a GPU"
    from soxr_amd import _native, device as dev, dist

    tile = _native.ADJOINT_INTERP_TILE
    log_path = os.environ.get("HIPSOXR_DEBUG_LAUNCH_LOG")
    rows = []
    for quality in ("HQ", "VHQ"):
        plan = dev.Plan(TOP * RATE, RATE, quality, vr=True)
        for dtype in (torch.float32, torch.float64):
            for n in args.clips:
                rng = np.random.default_rng(n)
                lengths = [int(v) for v in rng.integers(RATE, 10 * RATE + 1, n)]
                ratios = [float(f) for f in rng.uniform(0.9, TOP, n)]
                g = torch.Generator(device="cuda").manual_seed(n)
                buf = torch.randn(sum(lengths), dtype=dtype, device="cuda", generator=g) * 0.1
                ends = np.cumsum(lengths)
                clips = [buf[int(e - m):int(e)] for e, m in zip(ends, lengths)]
                fwd = dist.RaggedJob(plan, clips, io_ratios=ratios)
                fwd.launch()
                torch.cuda.synchronize()
                gys = [y.clone() for y in fwd.outputs()]      # cotangents of the forward's own shape
                gy = torch.cat(gys)
                gys = list(torch.split(gy, fwd.n_out))        # ... cut from one buffer
                gx = torch.empty(sum(lengths), dtype=dtype, device="cuda")
                gy_off = np.concatenate([[0], np.cumsum(fwd.n_out)[:-1]]).astype(np.int64)
                gx_off = np.concatenate([[0], ends[:-1]]).astype(np.int64)
                table = np.ascontiguousarray(np.stack([gy_off, fwd.n_out, gx_off, lengths], axis=1), dtype=np.int64)
                table_dev = torch.from_numpy(table).cuda()
                elem, st = dev._torch_elem(dtype), torch.cuda.current_stream().cuda_stream
                gx_tiles = -(-max(lengths) // tile)
                live = sum(-(-m // tile) for m in lengths)
                skip_share = 1.0 - live / float(gx_tiles * n)

                def adjoint():
                    plan.run_vr_ragged_adjoint(gy.data_ptr(), gx.data_ptr(), elem, 1, table, ratios, (1, 1), (1, 1), stream=st,
                                               kernel=_native.KERNEL_ADJOINT, table_dev=table_dev.data_ptr())

                if args.forms:
                    assert log_path, "--forms reads HIPSOXR_DEBUG_LAUNCH_LOG (the debug-switch build writes it)"
                    torch.cuda.synchronize()
                    pos = os.path.getsize(log_path) if os.path.exists(log_path) else 0
                    adjoint()
                    torch.cuda.synchronize()
                    with open(log_path) as fh:
                        fh.seek(pos)
                        lines = [ln.strip() for ln in fh.read().split("\n") if ln.strip()]
                    print("%s %s %d clips: %s" % (quality, str(dtype).split(".")[1], n, " | ".join(lines)), flush=True)
                    rows.append(dict(quality=quality, dtype=str(dtype).split(".")[1], clips=n, launches=lines))
                    continue

                def operator():
                    dist.resample_varispeed_adjoint(plan, gys, lengths, ratios, kernel=_native.KERNEL_ADJOINT)

                one_rows = [table[c:c + 1].copy() for c in range(n)]

                def loop():
                    for c in range(n):
                        plan.run_vr_ragged_adjoint(gy.data_ptr(), gx.data_ptr(), elem, 1, one_rows[c], ratios[c:c + 1], (1, 1), (1, 1),
                                                   stream=st, kernel=_native.KERNEL_ADJOINT)

                contestants = [("forward", fwd.launch), ("adjoint", adjoint), ("operator", operator), ("loop", loop)]
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
                row = dict(quality=quality, dtype=str(dtype).split(".")[1], clips=n, in_frames=sum(lengths), cotangent_samples=int(sum(fwd.n_out)),
                           grid=[gx_tiles, n], skip_share=skip_share,
                           us={k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in ts_.items()})
                rows.append(row)
                med = {k: row["us"][k]["median"] for k, _ in contestants}
                print("%-3s %-7s %5d clips  " % (quality, row["dtype"], n) +
                      "  ".join("%s %.0f us (%.0f-%.0f)" % (k, row["us"][k]["median"], row["us"][k]["min"], row["us"][k]["max"]) for k, _ in contestants) +
                      "  adjoint / forward %.2f  loop / adjoint %.1f  grid %dx%d, %.0f%% of its workgroups skip"
                      % (med["adjoint"] / med["forward"], med["loop"] / med["adjoint"], gx_tiles, n, 100 * skip_share), flush=True)
                del fwd, gys, gy, gx, buf, clips
                torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(dict(library=_native.LIB_PATH, warmup=args.warmup, steps=args.steps, rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
