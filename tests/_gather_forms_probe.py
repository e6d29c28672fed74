"""Helper of tests/test_gpu_gather_forms.py: runs the exact-bank jobs and streams of an .npz file (written by the test, which
holds their references) on the GPU under the process's HIPSOXR_* environment — the debug-switch build with
HIPSOXR_DEBUG_LAUNCH_LOG — and writes the results to another .npz:

    python tests/_gather_forms_probe.py JOBS.npz RESULTS.npz

`meta` in the jobs file is a JSON list of entries; the input of an entry is `x_<name>`.

Device jobs — {"name", "case": [in_rate, out_rate, quality], "kernel": "gather" | "exact", "layout": "inter" | "planar" |
"view", "dither", "seed", "counter"}, x [clips, frames, channels] — go through device.PreparedJob into a buffer with 8 guard
frames of poison either side of every clip, the payload pre-filled with NaN (integers: a sentinel).  "planar":
[clips][channel][frames] memory on both sides; "view": the job's channels are channels 1 .. n of tensors with n + 2 channels,
input and output, and the buffer comes back whole, so the channels beside the job's are guards too.  Per job `y_<name>`
([clips, 8 + n_out + 8, channels], for "view" channels + 2), the launch log's lines `log_<name>` and, where "counter" is set,
`clips_<name>`.

Streams own their output buffers (no guards); per call `y_<name>_<i>` and `log_<name>_<i>`, and `n_<name>` = the frames fed
by each call:
  * {"host": {"case", "seed"}, "chunks": [frames, ...]}, x [frames, channels]: ONE soxr_amd.ResampleStream (numpy in, numpy
    out; int16 dithered as the surface does by default), then one empty call with last=True;
  * {"stream": {"case", "vr", "dither", "seed"}, "chunks": [[frames, [in, out, slew] | null, "once" | "until_move" | "last"],
    ...], "max_move": n}, x [frames, channels]: ONE device.TensorStream; the ratio change after the call it stands with;
    "until_move": calls of that many frames until the launch log shows moving=1, max_move of them at the most; "last": with
    last=True;
  * {"group": {"case", "seeds", "prefix": [frames, ...], "calls", "frames", "flush": i}}, x [streams, frames, channels]:
    ONE device.TensorStreamGroup; stream i is first fed prefix[i] frames alone (`y_<name>_pre<i>`), then `calls` group calls of
    `frames` frames (`y_<name>_<c>` [streams, cap, channels] and `counts_<name>_<c>`), then stream `flush` is ended alone with
    an empty chunk (`y_<name>_flush`).

Nothing is compared here."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "python-soxr_amd"))
import torch  # noqa: E402
import soxr_amd  # noqa: E402
from soxr_amd import device as dev  # noqa: E402

GUARD, POISON = 8, 12345
INT_SENT = {torch.int16: -12345, torch.int32: -123456789}


class Log:
    def __init__(self, path):
        self.path, self.pos = path, 0

    def tail(self):
        """the lines written since the last call"""
        if not os.path.exists(self.path):
            return ""
        with open(self.path) as f:
            f.seek(self.pos)
            txt = f.read()
        self.pos += len(txt)
        return txt.strip()


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
    kernel = {"gather": dev.KERNEL_GATHER, "exact": dev.KERNEL_EXACT}[job["kernel"]]
    dev.PreparedJob(plan, x, view, kernel=kernel, dither=bool(job.get("dither")), clip_counter=counter,
                    dither_seed=int(job.get("seed", 0))).launch()
    torch.cuda.synchronize()
    return buf.cpu().numpy(), (None if counter is None else int(counter.item()))


def run_host_stream(name, job, x, log, out):
    h = job["host"]
    mono = x.shape[1] == 1
    rs = soxr_amd.ResampleStream(h["case"][0], h["case"][1], x.shape[1], dtype=x.dtype, quality=h["case"][2], dither_seed=int(h.get("seed", 0)))
    xs, at, fed = (x[:, 0] if mono else x), 0, []
    for i, n in enumerate(list(job["chunks"]) + [None]):
        if n is None:
            y = rs.resample_chunk(xs[at:at], last=True)
        else:
            y = rs.resample_chunk(np.ascontiguousarray(xs[at:at + n]))
            at += n
        fed.append(0 if n is None else n)
        out["y_%s_%d" % (name, i)], out["log_%s_%d" % (name, i)] = np.array(y), np.array(log.tail())
    assert at == x.shape[0]
    out["n_" + name] = np.array(fed)
    del rs


def run_tensor_stream(name, job, x, log, out):
    s = job["stream"]
    x = torch.from_numpy(x).cuda()
    ts = dev.TensorStream(s["case"][0], s["case"][1], x.shape[1], dtype=x.dtype, quality=s["case"][2], vr=bool(s["vr"]),
                          dither=bool(s.get("dither")), dither_seed=int(s.get("seed", 0)))
    xs, at, fed = (x[:, 0] if x.shape[1] == 1 else x), 0, []

    def call(n, last):
        nonlocal at
        y = ts.resample_chunk(xs[at:at + n], last=last)
        torch.cuda.synchronize()
        at += n
        lines = log.tail()
        out["y_%s_%d" % (name, len(fed))], out["log_%s_%d" % (name, len(fed))] = y.cpu().numpy(), np.array(lines)
        fed.append(n)
        return lines

    for n, change, how in job["chunks"]:
        if how == "until_move":
            for _ in range(int(job["max_move"])):
                if " moving=1" in call(n, False):
                    break
        else:
            call(n, how == "last")
        if change:
            ts.set_io_ratio(*change)
    assert at <= x.shape[0]
    out["n_" + name] = np.array(fed)
    del ts


def run_group(name, job, x, log, out):
    g = job["group"]
    x = torch.from_numpy(x).cuda()
    n, ch = x.shape[0], x.shape[2]
    grp = dev.TensorStreamGroup(n, g["case"][0], g["case"][1], num_channels=ch, dtype=x.dtype, quality=g["case"][2], dither=True, dither_seeds=g["seeds"])
    for i, pre in enumerate(g["prefix"]):
        if pre:
            y = grp.streams[i].resample_chunk(x[i, :pre] if ch > 1 else x[i, :pre, 0])
            torch.cuda.synchronize()
            out["y_%s_pre%d" % (name, i)], out["log_%s_pre%d" % (name, i)] = y.cpu().numpy(), np.array(log.tail())
    frames = int(g["frames"])
    for c in range(int(g["calls"])):
        chunk = torch.stack([x[i, pre + c * frames:pre + (c + 1) * frames] for i, pre in enumerate(g["prefix"])])
        y, counts = grp.resample_chunks(chunk if ch > 1 else chunk[:, :, 0])
        torch.cuda.synchronize()
        out["y_%s_%d" % (name, c)], out["counts_%s_%d" % (name, c)], out["log_%s_%d" % (name, c)] = y.cpu().numpy(), np.array(counts), np.array(log.tail())
    i = int(g["flush"])
    y = grp.streams[i].resample_chunk(x[i, :0] if ch > 1 else x[i, :0, 0], last=True)
    torch.cuda.synchronize()
    out["y_%s_flush" % name], out["log_%s_flush" % name] = y.cpu().numpy(), np.array(log.tail())
    del grp


def main():
    jobs = np.load(sys.argv[1])
    log = Log(os.environ["HIPSOXR_DEBUG_LAUNCH_LOG"])
    plans, out = {}, {}
    for job in json.loads(str(jobs["meta"])):
        name = job["name"]
        x = jobs["x_" + name]
        log.tail()
        if "host" in job:
            run_host_stream(name, job, x, log, out)
        elif "stream" in job:
            run_tensor_stream(name, job, x, log, out)
        elif "group" in job:
            run_group(name, job, x, log, out)
        else:
            case = tuple(job["case"])
            if case not in plans:
                plans[case] = dev.Plan(*case)
            buf, n_clipped = run_job(job, torch.from_numpy(x).cuda(), plans[case])
            out["y_" + name], out["log_" + name] = buf, np.array(log.tail())
            if n_clipped is not None:
                out["clips_" + name] = np.array(n_clipped)
    np.savez(sys.argv[2], **out)
    print("GATHER_FORMS_PROBE done: %d entries" % sum(k.startswith("log_") for k in out))


if __name__ == "__main__":
    main()
