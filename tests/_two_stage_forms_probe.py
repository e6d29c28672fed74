"""Helper of tests/test_gpu_two_stage_forms.py: runs the two-stage jobs of an .npz file (written by the test) on the GPU under
the process's HIPSOXR_* environment — the debug-switch build with HIPSOXR_DEBUG_LAUNCH_LOG — and writes the results to
another .npz:

    python tests/_two_stage_forms_probe.py JOBS.npz RESULTS.npz

`meta` in the jobs file is a JSON list of {"name", "case": [in_rate, out_rate, quality], "layout": "inter" | "planar"}; the
input of a job is `x_<name>`, always [clips, frames, channels].  Per job: the output buffer of the job under KERNEL_AUTO WITH
its 8 guard frames either side of every clip — so 8 poison elements either side of every column — the payload pre-filled
with NaN (`y_<name>`: [clips, 8 + n_out + 8, channels] whatever the layout in memory), the same job under KERNEL_EXACT
(`ye_<name>`: [clips, n_out, channels]) and the launch log's lines of the AUTO run (`log_<name>`).  Nothing is compared here."""
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
        name, case, planar = job["name"], tuple(job["case"]), job["layout"] == "planar"
        if case not in plans:
            plans[case] = dev.Plan(*case)
        x = torch.from_numpy(jobs["x_" + name]).cuda()           # [clips, frames, channels], interleaved
        clips, frames, ch = x.shape
        n_out = plans[case].out_len(frames)
        if planar:                                                 # the same values as [clips][channel][frames]
            x = x.permute(0, 2, 1).contiguous().permute(0, 2, 1)
            buf = torch.full((clips, ch, n_out + 2 * GUARD), POISON, dtype=x.dtype, device="cuda").permute(0, 2, 1)
        else:
            buf = torch.full((clips, n_out + 2 * GUARD, ch), POISON, dtype=x.dtype, device="cuda")
        buf[:, GUARD:GUARD + n_out] = float("nan")
        _, pos = log_tail(log_path, pos)
        dev.resample_tensor(plans[case], x, out=buf[:, GUARD:GUARD + n_out])
        torch.cuda.synchronize()
        lines, pos = log_tail(log_path, pos)
        ye = dev.resample_tensor(plans[case], x, kernel=dev.KERNEL_EXACT)
        out["y_" + name], out["ye_" + name], out["log_" + name] = buf.cpu().numpy(), ye.cpu().numpy(), np.array(lines.strip())
        del x, buf, ye
    np.savez(sys.argv[2], **out)
    print("TWO_STAGE_FORMS_PROBE done: %d jobs" % sum(k.startswith("y_") for k in out))


if __name__ == "__main__":
    main()
