"""Helper of tests/test_gpu_poly_instances.py: runs the two-stage jobs of a JSON file (written by the test) on the GPU under the
process's HIPSOXR_* environment — the debug-switch build with HIPSOXR_DEBUG_LAUNCH_LOG, with or without
HIPSOXR_POLY_NO_PAIR=1 — and writes what came out to an .npz:

    python tests/_poly_instances_probe.py JOBS.json RESULTS.npz

A job is {"name", "leg": "A" | "B", "case": [in_rate, out_rate, quality], "dtype": "f32" | "f64", "frames", "clips", "ch",
"seed"}: [clips, frames, ch] interleaved white noise of RMS 0.25, every column from a generator seeded for that column alone.
The job runs under KERNEL_AUTO through `out=` into a buffer [clips, 8 + n_out + 8, ch]: 8 poison elements either side of every
column, the payload pre-filled with NaN.

Leg A (one clip; inputs made on the host): `x_`, `y_` (the buffer, guards included), `log_` (the launch log's lines of the run)
and `same_` — the job once more into a fresh buffer gave the same bytes, guards included.
Leg B (about 1024 columns; inputs made on the device, nothing of that size leaves it): the same job under KERNEL_EXACT, and per
column, computed on the device, `rel_` (RMS of the difference over the RMS of the exact engine's column), `max_` (largest
difference), `rms_` (the exact engine's column) — each [clips, ch] — `ok_` = (every guard element intact, payload elements
still NaN, payload elements that are not finite), `log_`, and the raw data of three columns — the first, the middle one, the
last: `cols_` = their (clip, channel), `x_` [3, frames], `y_` [3, n_out].
`wall_` per job and `wall` for the process, seconds.  A line `POLY_CASE <name>` is printed before each job.  Nothing is
compared against a bar here."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ragged_exact_probe import DTYPE, Log  # noqa: E402  (puts the repository and the package on sys.path)
import torch  # noqa: E402
from soxr_amd import device as dev  # noqa: E402

GUARD, POISON = 8, 12345.0
NP = {"f32": np.float32, "f64": np.float64}


def column_seed(seed, col):
    return int(seed) * 100003 + int(col)


def guarded(clips, n_out, ch, dtype):
    buf = torch.full((clips, n_out + 2 * GUARD, ch), POISON, dtype=dtype, device="cuda")
    buf[:, GUARD:GUARD + n_out] = float("nan")
    return buf


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def leg_a(job, plan, log, out):
    name, clips, frames, ch = job["name"], int(job["clips"]), int(job["frames"]), int(job["ch"])
    x = np.empty((clips, frames, ch), NP[job["dtype"]])
    for c in range(clips * ch):
        x[c // ch, :, c % ch] = np.random.default_rng(column_seed(job["seed"], c)).standard_normal(frames) * 0.25
    xd = torch.from_numpy(x).cuda()
    n_out = plan.out_len(frames)
    buf = guarded(clips, n_out, ch, xd.dtype)
    torch.cuda.synchronize()
    log.tail()
    dev.resample_tensor(plan, xd, out=buf[:, GUARD:GUARD + n_out])
    torch.cuda.synchronize()
    out["log_" + name] = np.array(log.tail().strip())
    again = guarded(clips, n_out, ch, xd.dtype)
    dev.resample_tensor(plan, xd, out=again[:, GUARD:GUARD + n_out])
    torch.cuda.synchronize()
    log.tail()
    out["same_" + name] = np.array(bool(torch.equal(bits(buf), bits(again))))
    out["x_" + name], out["y_" + name] = x, buf.cpu().numpy()


def leg_b(job, plan, log, out):
    name, clips, frames, ch, dtype = job["name"], int(job["clips"]), int(job["frames"]), int(job["ch"]), DTYPE[job["dtype"]]
    x = torch.empty((clips, frames, ch), dtype=dtype, device="cuda")
    gen = torch.Generator(device="cuda")
    for c in range(clips * ch):
        gen.manual_seed(column_seed(job["seed"], c))
        x[c // ch, :, c % ch] = torch.randn(frames, generator=gen, dtype=dtype, device="cuda") * 0.25
    n_out = plan.out_len(frames)
    buf = guarded(clips, n_out, ch, dtype)
    torch.cuda.synchronize()
    log.tail()
    dev.resample_tensor(plan, x, out=buf[:, GUARD:GUARD + n_out])
    torch.cuda.synchronize()
    out["log_" + name] = np.array(log.tail().strip())
    ye = dev.resample_tensor(plan, x, kernel=dev.KERNEL_EXACT)
    torch.cuda.synchronize()
    log.tail()
    assert tuple(ye.shape) == (clips, n_out, ch)
    y = buf[:, GUARD:GUARD + n_out]
    guards_ok = bool((buf[:, :GUARD] == POISON).all() and (buf[:, GUARD + n_out:] == POISON).all())
    out["ok_" + name] = np.array([int(guards_ok), int(torch.isnan(y).sum()), int((~torch.isfinite(y)).sum())], np.int64)
    ref_sq = torch.zeros((clips, ch), dtype=torch.float64, device="cuda")
    d_sq, d_max = torch.zeros_like(ref_sq), torch.zeros_like(ref_sq)
    step = max(1, (1 << 24) // (n_out * ch))  # clips per pass: float64 temporaries of 128 MiB at the most
    for c0 in range(0, clips, step):
        r = ye[c0:c0 + step].double()
        d = y[c0:c0 + step].double() - r
        ref_sq[c0:c0 + step], d_sq[c0:c0 + step], d_max[c0:c0 + step] = (r * r).mean(dim=1), (d * d).mean(dim=1), d.abs().amax(dim=1)
    out["rel_" + name] = (d_sq.sqrt() / ref_sq.sqrt()).cpu().numpy()
    out["max_" + name], out["rms_" + name] = d_max.cpu().numpy(), ref_sq.sqrt().cpu().numpy()
    cols = [(0, 0), (clips // 2, ch // 2), (clips - 1, ch - 1)]
    out["cols_" + name] = np.array(cols, np.int64)
    out["x_" + name] = torch.stack([x[a, :, b] for a, b in cols]).cpu().numpy()
    out["y_" + name] = torch.stack([y[a, :, b] for a, b in cols]).cpu().numpy()


def main():
    t_all = time.time()
    with open(sys.argv[1]) as f:
        jobs = json.load(f)
    log = Log(os.environ["HIPSOXR_DEBUG_LAUNCH_LOG"])
    plans, out = {}, {}
    for job in jobs:
        print("POLY_CASE " + job["name"], flush=True)
        case = tuple(job["case"])
        if case not in plans:
            plans[case] = dev.Plan(*case)
        assert plans[case].phases != 0, "an interpolated-phase plan"
        t0 = time.time()
        {"A": leg_a, "B": leg_b}[job["leg"]](job, plans[case], log, out)
        out["wall_" + job["name"]] = np.array(time.time() - t0)
    out["wall"] = np.array(time.time() - t_all)
    np.savez(sys.argv[2], **out)
    print("POLY_INSTANCES_PROBE done: %d jobs, %.1f s" % (len(jobs), time.time() - t_all))


if __name__ == "__main__":
    main()
