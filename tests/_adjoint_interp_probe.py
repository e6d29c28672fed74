"""Helper of tests/test_gpu_adjoint_interp.py: runs adjoint jobs with kernel=KERNEL_ADJOINT from an .npz file (written by the
test, which holds their references) on the GPU under the process's HIPSOXR_* environment — the debug-switch build with
HIPSOXR_DEBUG_LAUNCH_LOG — and writes the results to another .npz:

    python tests/_adjoint_interp_probe.py JOBS.npz RESULTS.npz

`meta` in the jobs file is a JSON list of {"name", "case": [in_rate, out_rate, quality], "n_x"}; the cotangent of a job is
`gy_<name>`, always [clips, n_y, channels] (channels > 1: interleaved frames).  Per job: the output buffer WITH its 8 guard
frames either side of every clip, the payload pre-filled with NaN (`gx_<name>`: [clips, 8 + n_x + 8, channels]), and the
launch log's lines for the job (`log_<name>`).  Nothing is compared here."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "python-soxr_amd"))
import torch  # noqa: E402
from soxr_amd import device as dev  # noqa: E402

GUARD, POISON = 8, 12345.0


def log_tail(path, pos):
    if not os.path.exists(path):
        return "", pos
    with open(path) as f:
        f.seek(pos)
        txt = f.read()
    return txt, pos + len(txt)


def main():
    jobs = np.load(sys.argv[1])
    log_path, pos = os.environ["HIPSOXR_DEBUG_LAUNCH_LOG"], 0
    plans, out = {}, {}
    for job in json.loads(str(jobs["meta"])):
        name, case, n_x = job["name"], tuple(job["case"]), int(job["n_x"])
        if case not in plans:
            plans[case] = dev.Plan(*case)
        gy = torch.from_numpy(jobs["gy_" + name]).cuda()
        clips, _, ch = gy.shape
        buf = torch.full((clips, n_x + 2 * GUARD, ch), POISON, dtype=gy.dtype, device="cuda")
        buf[:, GUARD:GUARD + n_x] = float("nan")
        _, pos = log_tail(log_path, pos)
        dev.resample_tensor_adjoint(plans[case], gy, n_x, out=buf[:, GUARD:GUARD + n_x], kernel=dev.KERNEL_ADJOINT)
        torch.cuda.synchronize()
        line, pos = log_tail(log_path, pos)
        out["gx_" + name], out["log_" + name] = buf.cpu().numpy(), np.array(line.strip())
        del gy, buf
    np.savez(sys.argv[2], **out)
    print("ADJOINT_INTERP_PROBE done: %d jobs" % sum(k.startswith("gx_") for k in out))


if __name__ == "__main__":
    main()
