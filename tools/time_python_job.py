#!/usr/bin/env python
"""Host cost of the Python layer that describes a job to the library, one sample per process, as one JSON line:

    time_python_job.py stub [--package DIR]   no GPU: the C entries that take a job are stubbed and the stream query faked —
                                              us per `Plan.run` with integer arguments (20 000 calls) and us per
                                              `RaggedJob` over 64 host clips (2 000 constructions)
    time_python_job.py gpu [--package DIR]    us per `resample_tensor(plan, x)` on a 480-frame float32 mono device tensor
                                              (5 000 calls, one synchronise at the end)

--package: the directory that holds the `soxr_amd` to time (default: this checkout's python-soxr_amd) — another checkout's
copy of the .py files serves, with HIPSOXR_LIBRARY naming the library to load.  Run the two trees alternately."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=("stub", "gpu"))
ap.add_argument("--package", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "python-soxr_amd"))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.package))
import torch  # noqa: E402
from soxr_amd import _native, device as dev, dist  # noqa: E402

res = {"package": os.path.dirname(os.path.abspath(dev.__file__)), "what": args.what}
if args.what == "stub":
    class _Stream:
        cuda_stream = 0
    for name in ("hipsoxr_run_device", "hipsoxr_run_device_vr_ragged"):
        setattr(_native.lib, name, lambda *a: None)
    torch.cuda.current_stream = lambda device=None: _Stream()
    plan = dev.Plan(48000, 44100, "HQ")
    run, n = plan.run, 20000
    for _ in range(2000):
        run(4096, 8192, _native.F32, 1, 1, 480, 441, (0, 1, 1), (0, 1, 1), 0, _native.KERNEL_EXACT)
    t0 = time.perf_counter()
    for _ in range(n):
        run(4096, 8192, _native.F32, 1, 1, 480, 441, (0, 1, 1), (0, 1, 1), 0, _native.KERNEL_EXACT)
    res["plan_run_us"] = (time.perf_counter() - t0) / n * 1e6
    buf = torch.zeros(64 * 1000)
    clips, n = [buf[1000 * i:1000 * i + 500 + 7 * i] for i in range(64)], 2000
    for _ in range(100):
        dist.RaggedJob(plan, clips)
    t0 = time.perf_counter()
    for _ in range(n):
        dist.RaggedJob(plan, clips)
    res["ragged_job_us"] = (time.perf_counter() - t0) / n * 1e6
else:
    plan, n = dev.Plan(48000, 44100, "HQ"), 5000
    x = torch.zeros(480, device="cuda")
    for _ in range(500):
        dev.resample_tensor(plan, x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        dev.resample_tensor(plan, x)
    torch.cuda.synchronize()
    res["resample_tensor_us"] = (time.perf_counter() - t0) / n * 1e6
print(json.dumps(res))
