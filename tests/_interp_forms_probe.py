"""Helper of tests/test_gpu_interp_forms.py: runs the interpolated-phase forward jobs of an .npz file (written by the test,
which holds their references) on the GPU under the process's HIPSOXR_* environment — the debug-switch build with
HIPSOXR_DEBUG_LAUNCH_LOG — and writes the results to another .npz:

    python tests/_interp_forms_probe.py JOBS.npz RESULTS.npz

`meta` in the jobs file is a JSON list of jobs; the input of a job is `x_<name>`, always [clips, frames, channels].

Device jobs — {"name", "case": [in_rate, out_rate, quality], "layout": "inter" | "planar" | "view", "dither", "seed",
"counter"} — go through device.PreparedJob under KERNEL_EXACT into a buffer with 8 guard frames of poison either side of
every clip, the payload pre-filled with NaN (integers: a sentinel).  "planar": [clips][channel][frames] memory on both
sides; "view": the job's channels are channels 1 .. n of tensors with n + 2 channels, input and output, and the buffer comes
back whole, so the channels beside the job's are guards too.  Per job `y_<name>` ([clips, 8 + n_out + 8, channels], for
"view" channels + 2), the launch log's lines `log_<name>` and, where "counter" is set, `clips_<name>`.

Streams — {"name", "stream": {"case", "vr", "dither", "seed", "flush"}, "chunks": [[frames, [in, out, slew] | null], ...]} —
feed x_<name> ([1, frames, channels]) to ONE device.TensorStream in the given chunks, the last with last=True where "flush"
is set, the ratio change after the chunk it stands with: `y_<name>_<i>` and `log_<name>_<i>` per chunk (a stream owns its output buffers: no guards).

Nothing is compared here."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "python-soxr_amd"))
import torch  # noqa: E402
from soxr_amd import device as dev  # noqa: E402

GUARD, POISON = 8, 12345
INT_SENT = {torch.int16: -12345, torch.int32: -123456789}


def log_tail(path, pos):
    if not os.path.exists(path):
        return "", pos
    with open(path) as f:
        f.seek(pos)
        txt = f.read()
    return txt, pos + len(txt)


def run_job(job, x, plan):
    """-> (guarded buffer [clips, GUARD + n_out + GUARD, channels (+ 2)], clip count or None)"""
    layout = job["layout"]
    clips, frames, ch = x.shape
    n_out = plan.out_len(frames)
    fill = INT_SENT.get(x.dtype, float("nan"))
    side = 1 if layout == "view" else 0
    if side:  # the job's channels in the middle of wider tensors
        wide = torch.zeros((clips, frames, ch + 2), dtype=x.dtype, device="cuda")
        wide[:, :, 1:1 + ch] = x
        x = wide[:, :, 1:1 + ch]
    if layout == "planar":  # the same values as [clips][channel][frames]
        x = x.permute(0, 2, 1).contiguous().permute(0, 2, 1)
        buf = torch.full((clips, ch, n_out + 2 * GUARD), POISON, dtype=x.dtype, device="cuda").permute(0, 2, 1)
    else:
        buf = torch.full((clips, n_out + 2 * GUARD, ch + 2 * side), POISON, dtype=x.dtype, device="cuda")
    view = buf[:, GUARD:GUARD + n_out, side:side + ch]
    view[:] = fill
    counter = torch.zeros(1, dtype=torch.int64, device="cuda") if job.get("counter") else None
    dev.PreparedJob(plan, x, view, kernel=dev.KERNEL_EXACT, dither=bool(job.get("dither")), clip_counter=counter,
                    dither_seed=int(job.get("seed", 0))).launch()
    torch.cuda.synchronize()
    return buf.cpu().numpy(), (None if counter is None else int(counter.item()))


def main():
    jobs = np.load(sys.argv[1])
    log_path, pos = os.environ["HIPSOXR_DEBUG_LAUNCH_LOG"], 0
    plans, out = {}, {}
    for job in json.loads(str(jobs["meta"])):
        name = job["name"]
        x = torch.from_numpy(jobs["x_" + name]).cuda()
        _, pos = log_tail(log_path, pos)
        if "stream" in job:
            s = job["stream"]
            ts = dev.TensorStream(s["case"][0], s["case"][1], x.shape[2], dtype=x.dtype, quality=s["case"][2], vr=bool(s["vr"]),
                                  dither=bool(s.get("dither")), dither_seed=int(s.get("seed", 0)))
            xs, at = (x[0, :, 0] if x.shape[2] == 1 else x[0]), 0
            for i, (n, change) in enumerate(job["chunks"]):
                y = ts.resample_chunk(xs[at:at + n], last=(bool(s.get("flush")) and i == len(job["chunks"]) - 1))
                torch.cuda.synchronize()
                lines, pos = log_tail(log_path, pos)
                out["y_%s_%d" % (name, i)], out["log_%s_%d" % (name, i)] = y.cpu().numpy(), np.array(lines.strip())
                at += n
                if change:
                    ts.set_io_ratio(*change)
            assert at == x.shape[1]
            del ts
        else:
            case = tuple(job["case"])
            if case not in plans:
                plans[case] = dev.Plan(*case)
            buf, n_clipped = run_job(job, x, plans[case])
            lines, pos = log_tail(log_path, pos)
            out["y_" + name], out["log_" + name] = buf, np.array(lines.strip())
            if n_clipped is not None:
                out["clips_" + name] = np.array(n_clipped)
        del x
    np.savez(sys.argv[2], **out)
    print("INTERP_FORMS_PROBE done: %d jobs" % sum(k.startswith("log_") for k in out))


if __name__ == "__main__":
    main()
