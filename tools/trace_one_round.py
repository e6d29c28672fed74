#!/usr/bin/env python
"""Debug aid: ONE launch of k_fft_pair2 on a single mono clip (default 60 s, 48k -> 44.1k VHQ float32) from a build with
-DFFT2_TRACE -DHIPSOXR_DEBUG_SWITCHES; reads the per-wave s_memtime stamps (stamp layout: tools/trace_pair2.py) and
answers what the one-round block-size rule (csrc/fft.hip, kOneRoundCost) is built on:
  * how many workgroups each CU really received;
  * how long one workgroup's chain is on a CU that holds n of them;
  * when the last workgroup of a CU starts and when the CU is done (counters of different parts of the chip are not
    synchronised: every span is taken inside one CU).

    HIPSOXR_VARIANT=trace HIPSOXR_EXTRA_FLAGS="-DFFT2_TRACE -DHIPSOXR_DEBUG_SWITCHES" bash python-soxr_amd/build.sh
    HIPSOXR_LIBRARY=python-soxr_amd/_variants/trace/libhipsoxr.so [HIPSOXR_DEBUG_FFT_K=k] python tools/trace_one_round.py [--root TREE] [--seconds 60] [--up]
"""
import argparse
import os
import sys
import tempfile

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--seconds", type=int, default=60)
ap.add_argument("--up", action="store_true")
ap.add_argument("--waves", type=int, default=6, help="waves per workgroup of the kernel that runs: 6 (k = 16, 32), 5 (k = 14, 20), 4 (k = 8)")
args = ap.parse_args()
root = os.path.abspath(args.root)
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "python-soxr_amd"))
path = os.path.join(tempfile.mkdtemp(), "trace.bin")
os.environ["HIPSOXR_DEBUG_TRACE"] = path
import torch  # noqa: E402
from soxr_amd import device as dev  # noqa: E402

fi, fo = (44100, 48000) if args.up else (48000, 44100)
plan = dev.Plan(fi, fo, "VHQ")
x = torch.randn(fi * args.seconds, device="cuda") * 0.25
for _ in range(5):                                   # (every traced launch is synchronous and rewrites the file: the last one counts)
    y = dev.resample_tensor(plan, x)
    torch.cuda.synchronize()
raw = np.fromfile(path, dtype=np.uint64).astype(np.int64)
NW = args.waves
if raw.size % (NW * 16):
    raise SystemExit("%d words are not records of %d waves" % (raw.size, NW))
t = raw.reshape(-1, NW, 16)
print("clip %d s %d->%d: %d workgroups of %d waves" % (args.seconds, fi, fo, t.shape[0], NW))
ws, we = t[:, :, 0].min(axis=1), t[:, :, 15].max(axis=1)
hw, xcc = t[:, 0, 13], t[:, 0, 14] & 0xF
key = ((xcc * 8 + ((hw >> 13) & 7)) * 2 + ((hw >> 12) & 1)) * 16 + ((hw >> 8) & 0xF)
cus, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
print("CUs that received work: %d; workgroups per CU: " % len(cus) + ", ".join("%d CUs x %d" % ((cnt == c).sum(), c) for c in np.unique(cnt)))
life = we - ws
load = cnt[inv]                                       # how many workgroups the CU of this workgroup holds
print("ticks are s_memtime units; every figure below is in ticks")
for c in np.unique(cnt):
    m = load == c
    print("chain of one workgroup on a CU that holds %d: median %.0f  p10 %.0f  p90 %.0f  (n = %d)" % ((c,) + tuple(np.percentile(life[m], [50, 10, 90])) + (m.sum(),)))
# One CU's workgroups share a clock for certain: every span below is taken inside one CU.
for c in np.unique(cnt):
    busy, last_start = [], []
    for k in cus[cnt == c]:
        m = key == k
        busy.append(we[m].max() - ws[m].min())
        last_start.append(ws[m].max() - ws[m].min())
    print("a CU that holds %d: first start -> last end median %.0f  p90 %.0f  max %.0f; its last workgroup starts %.0f after its first (p90 %.0f)" % (
        c, np.median(busy), np.percentile(busy, 90), max(busy), np.median(last_start), np.percentile(last_start, 90)))
# phases of a chain (wave 0): load + first pass | rest of forward | inverse | store
seg = {"F1 (loads + pass 1)": (0, 1), "forward rest": (1, 6), "inverse + staging": (6, 12), "store": (12, 15)}
print("chain phases, wave 0, median: " + "  ".join("%s %.0f" % (n, np.median(t[:, 0, b] - t[:, 0, a])) for n, (a, b) in seg.items()))
