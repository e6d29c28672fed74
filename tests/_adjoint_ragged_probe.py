"""Helper of tests/test_gpu_adjoint_ragged.py: runs ragged adjoint jobs (hipsoxr_run_device_adjoint_ragged through
Plan.run_adjoint_ragged) on the GPU under the process's HIPSOXR_* environment — the debug-switch build with
HIPSOXR_DEBUG_LAUNCH_LOG — and writes what it ran and what came out to an .npz:

    python tests/_adjoint_ragged_probe.py JOBS.json RESULTS.npz

JOBS.json is a list of jobs
    {"name", "case": [in_rate, out_rate, quality], "dtype": "f32" | "f64", "ch", "kernel", "seed",
     "clips": [[a, b, c, cut], ...], "layout": "packed" | "split" | "strided", "table_dev": bool,
     "inf": [clip, ...], "solo": "clip" | "class" | "none"}
A clip has n_x = a pb Mc + b Mc + c frames: Mc is the replicated period of csrc/adjoint.hip's tiled kernel (the formula of
tests/test_gpu_adjoint.py) and pb the periods per workgroup, which only the launcher knows — it is read from the launch log
of ONE equal-length job of 4 Mc frames of the same plan, type and channel count (jobs with a == 0 everywhere need none).
cut: n_y = out_len(n_x) - cut, or 0 where cut < 0.  The cotangent is standard normal from `seed` (jobs of one seed and one
shape share their data); "inf" puts one +inf into channel 0 at the middle sample of the named clips.

Layouts (elements; S = the sentinel every buffer is pre-filled with):
    packed   gy clips back to back, frames of interleaved channels; gx the same with ONE spare frame behind every clip
    split    channel planes: gy [ch][sum n_y], gx [ch][sum (n_x + 1)] — frame stride 1, one channel stride for the job
    strided  gy frames two frames apart (S in between), gx as packed

Per job: `table_<name>` [clips, 4] as passed, `geom_<name>` = (Mc, pb, gy frame stride, gy channel stride, gx frame stride,
gx channel stride), `gy_<name>` and `gx_<name>` the whole buffers as they lay in memory, `log_<name>` the launch log's lines
of the ragged launch, and `solo_<name>`: every clip's [n_x, ch] result of device.resample_tensor_adjoint, concatenated —
"clip": each clip run alone; "class": the clips of one (n_y, n_x) as one equal-length batch (mono jobs).  Nothing is
compared here."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "python-soxr_amd"))
import torch  # noqa: E402
from soxr_amd import _native, device as dev  # noqa: E402

SENTINEL = 12345.0
DTYPE = {"f32": torch.float32, "f64": torch.float64}


def log_tail(path, pos):
    if not os.path.exists(path):
        return "", pos
    with open(path) as f:
        f.seek(pos)
        txt = f.read()
    return txt, pos + len(txt)


def main():
    with open(sys.argv[1]) as f:
        jobs = json.load(f)
    log_path, pos = os.environ["HIPSOXR_DEBUG_LAUNCH_LOG"], 0
    plans, pbs, out = {}, {}, {}
    for job in jobs:
        name, case, ch, dtype, kernel = job["name"], tuple(job["case"]), int(job["ch"]), DTYPE[job["dtype"]], int(job["kernel"])
        if case not in plans:
            plans[case] = dev.Plan(*case)
        plan = plans[case]
        mc = max(-(-16 // plan.M), -(-64 // plan.L)) * plan.M
        pb = 0
        if any(c[0] for c in job["clips"]):
            key = (case, job["dtype"], ch, job["layout"])
            if key not in pbs:  # one equal-length launch of the tiled kernel in the job's layout says what pb is
                g = torch.zeros((plan.out_len(4 * mc), ch) if job["layout"] != "split" else (ch, plan.out_len(4 * mc)), dtype=dtype, device="cuda")
                _, pos = log_tail(log_path, pos)
                dev.resample_tensor_adjoint(plan, g if job["layout"] != "split" else g.t(), 4 * mc, kernel=kernel)
                torch.cuda.synchronize()
                line, pos = log_tail(log_path, pos)
                f = dict(tok.split("=", 1) for tok in line.split())
                assert f["kernel"] == "adj_tile", line
                pbs[key] = int(f["pb"])
            pb = pbs[key]
        n_x = [a * pb * mc + b * mc + c for a, b, c, _ in job["clips"]]
        n_y = [0 if cl[3] < 0 else plan.out_len(n) - cl[3] for n, cl in zip(n_x, job["clips"])]
        assert min(n_y) >= 0
        rng = np.random.default_rng(int(job["seed"]))
        data = [rng.standard_normal((n, ch)) for n in n_y]
        for c in job.get("inf", []):
            data[c][n_y[c] // 2, 0] = np.inf
        data = [torch.from_numpy(d).to(dtype) for d in data]
        sy, sx = int(sum(n_y)), int(sum(n_x)) + len(n_x)
        cy = np.concatenate([[0], np.cumsum(n_y)[:-1]]).astype(np.int64)
        cx = np.concatenate([[0], np.cumsum(np.array(n_x) + 1)[:-1]]).astype(np.int64)
        layout = job["layout"]
        if layout == "split":
            gy_s, gx_s, gy_off, gx_off = (1, max(sy, 1)), (1, sx), cy, cx
            gy_len, gx_len = ch * max(sy, 1), ch * sx
        elif layout == "strided":
            gy_s, gx_s, gy_off, gx_off = (2 * ch, 1), (ch, 1), 2 * ch * cy, ch * cx
            gy_len, gx_len = 2 * ch * max(sy, 1), ch * sx
        else:
            gy_s, gx_s, gy_off, gx_off = (ch, 1), (ch, 1), ch * cy, ch * cx
            gy_len, gx_len = ch * max(sy, 1), ch * sx
        gy = torch.full((gy_len,), SENTINEL, dtype=dtype)
        for d, off, n in zip(data, gy_off, n_y):
            torch.as_strided(gy, (n, ch), gy_s, int(off)).copy_(d)
        gy = gy.cuda()
        gx = torch.full((gx_len,), SENTINEL, dtype=dtype, device="cuda")
        table = np.ascontiguousarray(np.stack([gy_off, n_y, gx_off, n_x], axis=1), dtype=np.int64)
        table_dev = torch.from_numpy(table).cuda() if job.get("table_dev") else None
        torch.cuda.synchronize()
        _, pos = log_tail(log_path, pos)
        plan.run_adjoint_ragged(gy.data_ptr(), gx.data_ptr(), _native.F32 if dtype == torch.float32 else _native.F64, ch, table,
                                gy_s, gx_s, stream=torch.cuda.current_stream().cuda_stream, kernel=kernel,
                                table_dev=table_dev.data_ptr() if table_dev is not None else None)
        torch.cuda.synchronize()
        line, pos = log_tail(log_path, pos)
        out["table_" + name] = table
        out["geom_" + name] = np.array([mc, pb, gy_s[0], gy_s[1], gx_s[0], gx_s[1]], np.int64)
        out["gy_" + name], out["gx_" + name], out["log_" + name] = gy.cpu().numpy(), gx.cpu().numpy(), np.array(line.strip())
        solo = job.get("solo", "clip")
        if solo == "clip":
            parts = [dev.resample_tensor_adjoint(plan, d.cuda(), n, kernel=kernel).reshape(n, ch) for d, n in zip(data, n_x)]
            out["solo_" + name] = torch.cat([p.reshape(-1) for p in parts]).cpu().numpy() if parts else np.zeros(0)
        elif solo == "class":
            assert ch == 1 and layout == "packed"
            flat = torch.zeros(int(sum(n_x)), dtype=dtype, device="cuda")
            start = torch.from_numpy(np.concatenate([[0], np.cumsum(n_x)[:-1]]).astype(np.int64)).cuda()
            t = torch.from_numpy(table).cuda()
            for ny, nx in sorted(set(zip(n_y, n_x))):
                if nx == 0:
                    continue
                idx = torch.nonzero((t[:, 1] == ny) & (t[:, 3] == nx))[:, 0]
                batch = gy[t[idx, 0][:, None] + torch.arange(ny, device="cuda")[None, :]]          # [clips of the class, n_y]
                res = dev.resample_tensor_adjoint(plan, batch[:, :, None], nx, kernel=kernel)       # one equal-length job
                flat[start[idx][:, None] + torch.arange(nx, device="cuda")[None, :]] = res[:, :, 0]
            out["solo_" + name] = flat.cpu().numpy()
        torch.cuda.synchronize()
        del gy, gx, data
    np.savez(sys.argv[2], **out)
    print("ADJOINT_RAGGED_PROBE done: %d jobs" % len(jobs))


if __name__ == "__main__":
    main()
