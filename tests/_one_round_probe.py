"""Helper of tests/test_gpu_one_round_chain.py: runs the jobs of an .npz file (written by the test, which also holds their
references) on the GPU under the process's HIPSOXR_* environment — the debug-switch build with HIPSOXR_DEBUG_FFT_K = 14 or
20 and HIPSOXR_DEBUG_LAUNCH_LOG — and writes the results to another .npz:

    python tests/_one_round_probe.py JOBS.npz RESULTS.npz

Per job `name` (input `x_<name>`: [frames] mono or [3, frames] planar batch): the output buffer WITH its 8 guard elements
either side of every column (`y_<name>`), whether a second run gave the same bytes (`same_<name>`), and the launch log's
line for the job (`log_<name>`).  With `clip60` in the file: the 60 s clip's relative RMS error against the exact engine
(`clip60_rel`)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "python-soxr_amd"))
import torch  # noqa: E402
from soxr_amd import device as dev  # noqa: E402

GUARD, POISON = 8, 12345.0
FFT, EXACT = dev._n.KERNEL_FFT, 6  # (by name: AUTO keeps jobs this small on the exact engine)


def log_tail(path, pos):
    if not os.path.exists(path):
        return "", pos
    with open(path) as f:
        f.seek(pos)
        txt = f.read()
    return txt, pos + len(txt)


def run(plan, x):
    """x: [frames] or [clips, frames] float32 -> the guarded output buffer [clips, GUARD + n_out + GUARD]"""
    mono = x.ndim == 1
    xt = torch.from_numpy(np.atleast_2d(x)).cuda()
    clips, n = xt.shape
    n_out = plan.out_len(n)
    buf = torch.full((clips, n_out + 2 * GUARD), POISON, dtype=torch.float32, device="cuda")
    if mono:
        dev.resample_tensor(plan, xt[0], out=buf[0, GUARD:GUARD + n_out], kernel=FFT)
    else:
        dev.resample_tensor(plan, xt[:, :, None], out=buf[:, GUARD:GUARD + n_out, None], kernel=FFT)   # (3, n, 1): clip stride n_out + 16
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def main():
    jobs = np.load(sys.argv[1])
    log_path, pos = os.environ["HIPSOXR_DEBUG_LAUNCH_LOG"], 0
    plans = {"down": dev.Plan(48000, 44100, "VHQ"), "up": dev.Plan(44100, 48000, "VHQ")}
    out = {}
    for key in jobs.files:
        if not key.startswith("x_"):
            continue
        name = key[2:]
        plan = plans[name.split("_")[0]]
        _, pos = log_tail(log_path, pos)
        y1 = run(plan, jobs[key])
        line, pos = log_tail(log_path, pos)
        y2 = run(plan, jobs[key])
        out["y_" + name], out["same_" + name], out["log_" + name] = y1, np.array(y1.tobytes() == y2.tobytes()), np.array(line.strip())
    if "clip60" in jobs.files:
        xt = torch.from_numpy(jobs["clip60"]).cuda()
        y = dev.resample_tensor(plans["down"], xt).cpu().numpy().astype(np.float64)
        e = dev.resample_tensor(plans["down"], xt, kernel=EXACT).cpu().numpy().astype(np.float64)
        out["clip60_rel"] = np.array(np.sqrt(np.mean((y - e) ** 2)) / np.sqrt(np.mean(e ** 2)))
    np.savez(sys.argv[2], **out)
    print("ONE_ROUND_PROBE done: %d jobs" % sum(k.startswith("y_") for k in out))


if __name__ == "__main__":
    main()
