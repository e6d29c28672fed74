#!/usr/bin/env python
"""Launch time of float32 unit-stride jobs over clip length: mono and 2 planar columns, both directions of 48k <-> 44.1k
(VHQ), one `device.PreparedJob` per row — the sweep behind the block-size rule of one-round jobs (csrc/fft.hip,
kOneRoundCost) and its "nothing else got slower" check.  Per row: `windows` HIP-event windows of `launches` back-to-back
launches; the record holds the median, the fastest and the slowest window in microseconds per launch.

    python tools/one_round_sweep.py --out FILE.json [--root TREE] [--seconds 2,5,...] [--windows 9] [--launches 200]

--root TREE: import the package of another checkout (a build of the parent commit beside this one), so that two trees
are timed by the same script.  The library and its debug switches come from the environment as usual (HIPSOXR_LIBRARY,
HIPSOXR_DEBUG_FFT_K=k with the debug-switch build: every row on blocks of k periods).
"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--seconds", default="2,5,10,20,30,45,60,90,120,240")
ap.add_argument("--cols", default="1,2")
ap.add_argument("--windows", type=int, default=9)
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--tag", default="")
args = ap.parse_args()
root = os.path.abspath(args.root)
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "python-soxr_amd"))
import torch  # noqa: E402
from soxr_amd import device as dev  # noqa: E402

rows = []
torch.manual_seed(5)
for fi, fo in ((48000, 44100), (44100, 48000)):
    plan = dev.Plan(fi, fo, "VHQ")
    for cols in [int(c) for c in args.cols.split(",")]:
        for sec in [int(s) for s in args.seconds.split(",")]:
            n = fi * sec
            x = (torch.randn((cols, n), device="cuda") * 0.25).T      # [frames, cols]: planar columns, frame stride 1
            y = torch.empty((cols, plan.out_len(n)), device="cuda").T
            if cols == 1:
                x, y = x[:, 0].contiguous(), y[:, 0].contiguous()
            job = dev.PreparedJob(plan, x, y)
            for _ in range(20):
                job.launch()
            torch.cuda.synchronize()
            per = []
            for _ in range(args.windows):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    job.launch()
                e1.record()
                e1.synchronize()
                per.append(e0.elapsed_time(e1) * 1e3 / args.launches)
            per.sort()
            row = {"dir": "%d->%d" % (fi, fo), "cols": cols, "seconds": sec, "median_us": per[len(per) // 2], "min_us": per[0], "max_us": per[-1]}
            rows.append(row)
            print("%s %-13s cols %d %4d s  median %7.2f us  [%7.2f .. %7.2f]" % (args.tag, row["dir"], cols, sec, row["median_us"], per[0], per[-1]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump({"tag": args.tag, "root": os.path.relpath(root), "library": os.environ.get("HIPSOXR_LIBRARY", "product"),
               "force_k": os.environ.get("HIPSOXR_DEBUG_FFT_K"), "windows": args.windows, "launches": args.launches, "rows": rows}, f, indent=1)
