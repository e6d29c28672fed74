"""Run in a child process with the debug-switch build (HIPSOXR_LIBRARY) by tests/test_gpu_half.py: half jobs of the shapes
whose fused forms the launch log must name, under HIPSOXR_DEBUG_FFT_K (a forced one-round block size, so that the mono job's
block size differs by construction from the one the parent's float32 job takes).  Writes the mono result to argv[1] (.npy,
the float16 bits as int16) and prints the launch log as one JSON line."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "python-soxr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import torch
    torch.cuda.init()
    torch.zeros(1, device="cuda").cpu()
    from soxr_amd import device as dev, dist
    out_path, log_path = sys.argv[1], os.environ["HIPSOXR_DEBUG_LAUNCH_LOG"]
    plan = dev.Plan(48000, 44100, "VHQ")
    rng = np.random.default_rng(2024)
    x = torch.from_numpy((rng.standard_normal(9001) * 0.1).astype(np.float32)).cuda()   # the parent draws the same signal
    marks = {}

    def lines_of(fn):
        before = open(log_path).read().count("\n") if os.path.exists(log_path) else 0
        r = fn()
        torch.cuda.synchronize()
        return r, open(log_path).read().splitlines()[before:]

    y, marks["mono_f16_fft"] = lines_of(lambda: dev.resample_tensor(plan, x.half(), kernel=dev.KERNEL_FFT))
    np.save(out_path, y.cpu().view(torch.int16).numpy())
    xs = torch.from_numpy((rng.standard_normal((30011, 2)) * 0.1).astype(np.float32)).cuda()
    _, marks["stereo_bf16_auto"] = lines_of(lambda: dev.resample_tensor(plan, xs.bfloat16()))
    _, marks["stereo3_f16_auto"] = lines_of(lambda: dev.resample_tensor(plan, xs[:, :1].repeat(1, 3).half()))
    clips = [x[:n].half() for n in (1, 4705, 9001)]
    _, marks["ragged_f16_auto"] = lines_of(lambda: dist.RaggedJob(plan, clips).launch())
    _, marks["small_f16_auto"] = lines_of(lambda: dev.resample_tensor(plan, x[:500].half()))
    _, marks["exact_f16"] = lines_of(lambda: dev.resample_tensor(plan, x.half(), kernel=dev.KERNEL_EXACT))
    print("HALF_PROBE " + json.dumps(marks))


if __name__ == "__main__":
    main()
