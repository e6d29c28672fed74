"""Helper of tests/test_gpu_ragged_interp.py: runs ragged FORWARD jobs on interpolated-phase plans (hipsoxr_run_device with a
clip_table, Plan.phases != 0) on the GPU under the process's HIPSOXR_* environment — the debug-switch build with
HIPSOXR_DEBUG_LAUNCH_LOG — and writes what it ran and what came out to an .npz:

    python tests/_ragged_interp_probe.py JOBS.json RESULTS.npz

JOBS.json is a list of jobs.  A job without "kind" is a raw table job
    {"name", "case": [in_rate, out_rate, quality], "dtype": "f32" | "f64" | "i32" | "i16", "ch", "kernel", "seed",
     "unit": 256 | 32 | "KO", "clips": [[m, add, cut], ...], "in_lengths": [...] (instead of unit / clips: input frames
     outright), "layout": "packed" | "split" | "strided", "table_dev": bool, "dither": bool, "dither_seed",
     "data": "normal" | "square", "counter": bool, "solo": "clip" | "class" | "none"}
A clip is to have m U + add outputs — U the outputs of one column per workgroup of the kernel form the job is to reach: 256
(k_interp), 32 (k_interp_wave), or "KO" (k_interp_tile), which only the launcher's cost model knows: the lengths are first
made with KO = 30 P, and made again ONCE with the KO the job's own log line shows where that differs.  in_frames is the
least count whose output length reaches m U + add; out_frames = that - cut (cut > 0: a truncated clip).

Layouts, buffers, sentinels and the per-job results (`table_`, `x_`, `y_`, `log_`, `count_`, `solo_`) are those of
tests/_ragged_exact_probe.py, whose helpers this file uses; `geom_<name>` = (U, 0, 0, in frame stride, in channel stride,
out frame stride, out channel stride).

Jobs with "kind": "py_forward", "py_batch" (as there) and "py_grad2" (below).  Nothing is compared here."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ragged_exact_probe import DTYPE, SENTINEL, Log, fields, in_frames_for, make_data, py_batch, py_forward, run_table  # noqa: E402
import torch  # noqa: E402
from soxr_amd import _native, device as dev, dist  # noqa: E402


def table_job(job, plans, log, out):
    name, case, ch, dtype, kernel = job["name"], tuple(job["case"]), int(job["ch"]), DTYPE[job["dtype"]], int(job["kernel"])
    plan = plans.setdefault(case, dev.Plan(*case))
    assert plan.phases != 0, "an interpolated-phase plan"
    unit = job.get("unit", 0)
    u = 30 * plan.phases if unit == "KO" else int(unit)
    sent, layout = SENTINEL[job["dtype"]], job.get("layout", "packed")
    for attempt in range(2):
        if "in_lengths" in job:
            n_in = [int(n) for n in job["in_lengths"]]
            n_out = [plan.out_len(n) for n in n_in]
        else:
            want = [m * u + add for m, add, _ in job["clips"]]
            n_in = [in_frames_for(plan, w) for w in want]
            n_out = [w - cl[2] for w, cl in zip(want, job["clips"])]
        assert min(n_out) >= 0 and all(o <= plan.out_len(i) for o, i in zip(n_out, n_in)), (name, u, n_out)
        rng = np.random.default_rng(int(job["seed"]))
        if "in_lengths" in job:  # (many tiny clips: one draw)
            flat = make_data(job.get("data", "normal"), rng, max(int(sum(n_in)), 1), ch, dtype)
            ends = np.cumsum(n_in)
            data = [flat[e - n:e] for e, n in zip(ends, n_in)]
        else:
            data = [make_data(job.get("data", "normal"), rng, n, ch, dtype) for n in n_in]
        out_fr = np.concatenate([[0], np.cumsum(np.array(n_out) + 1)[:-1]]).astype(np.int64)
        in_fr = np.concatenate([[0], np.cumsum(n_in)[:-1]]).astype(np.int64)
        si, so = max(int(sum(n_in)), 1), int(sum(n_out)) + len(n_out)
        if layout == "split":
            in_s, out_s, in_off, out_off, in_len, out_len = (1, si), (1, so), in_fr, out_fr, ch * si, ch * so
        elif layout == "strided":
            in_s, out_s, in_off, out_off, in_len, out_len = (2 * ch, 1), (ch, 1), 2 * ch * in_fr, ch * out_fr, 2 * ch * si, ch * so
        else:
            in_s, out_s, in_off, out_off, in_len, out_len = (ch, 1), (ch, 1), ch * in_fr, ch * out_fr, ch * si, ch * so
        x = torch.full((in_len,), sent, dtype=dtype)
        if "in_lengths" in job:
            assert layout == "packed"
            x[:ch * int(sum(n_in))] = flat[:int(sum(n_in))].reshape(-1)
        else:
            for d, off, n in zip(data, in_off, n_in):
                torch.as_strided(x, (n, ch), in_s, int(off)).copy_(d)
        x = x.cuda()
        y = torch.full((out_len,), sent, dtype=dtype, device="cuda")
        table = np.ascontiguousarray(np.stack([in_off, n_in, out_off, n_out], axis=1), dtype=np.int64)
        table_dev = torch.from_numpy(table).cuda() if job.get("table_dev") else None
        counter = torch.zeros(1, dtype=torch.int64, device="cuda") if job.get("counter") else None
        torch.cuda.synchronize()
        log.tail()
        run_table(plan, x.data_ptr(), y.data_ptr(), dtype, ch, table, in_s, out_s, kernel,
                  table_dev=table_dev.data_ptr() if table_dev is not None else None, dither=job.get("dither", False),
                  seed=job.get("dither_seed", 0), counter=counter.data_ptr() if counter is not None else None)
        torch.cuda.synchronize()
        lines = log.tail().strip()
        got = [int(fields(ln).get("KO", 0)) for ln in lines.split("\n") if ln]
        if unit != "KO" or not got or got[0] == u or got[0] == 0:
            break
        assert attempt == 0, "the launcher's KO did not settle: %r" % lines
        u = got[0]
    out["table_" + name] = table
    out["geom_" + name] = np.array([u, 0, 0, in_s[0], in_s[1], out_s[0], out_s[1]], np.int64)
    out["x_" + name], out["y_" + name], out["log_" + name] = x.cpu().numpy(), y.cpu().numpy(), np.array(lines)
    solo, solo_count = job.get("solo", "clip"), torch.zeros(1, dtype=torch.int64, device="cuda")
    kw = dict(kernel=_native.KERNEL_EXACT, dither=job.get("dither", False), dither_seed=job.get("dither_seed", 0))
    if counter is not None:  # the per-clip counts: each clip alone as a job of its own out_frames
        for d, o, n in zip(data, n_out, n_in):
            if o:
                xd, yd = d.cuda(), torch.empty((o, ch), dtype=dtype, device="cuda")
                plan.run(xd.data_ptr(), yd.data_ptr(), dev._torch_elem(dtype), 1, ch, n, o, (0, ch, 1), (0, ch, 1),
                         stream=torch.cuda.current_stream().cuda_stream, kernel=_native.KERNEL_EXACT, clip_counter=solo_count.data_ptr(),
                         dither=kw["dither"], dither_seed=kw["dither_seed"])
                torch.cuda.synchronize()
    if solo == "clip":
        full = [dev.resample_tensor(plan, d.cuda(), **kw)[:o] if n else torch.zeros((0, ch), dtype=dtype, device="cuda")
                for d, o, n in zip(data, n_out, n_in)]
        out["solo_" + name] = torch.cat([p.reshape(-1) for p in full]).cpu().numpy()
    elif solo == "class":  # the clips of one length as one equal-length batch
        assert ch == 1 and layout == "packed"
        flat_y = torch.zeros(int(sum(n_out)), dtype=dtype, device="cuda")
        start = torch.from_numpy(np.concatenate([[0], np.cumsum(n_out)[:-1]]).astype(np.int64)).cuda()
        t = torch.from_numpy(table).cuda()
        for ni, no in sorted(set(zip(n_in, n_out))):
            if no == 0:
                continue
            idx = torch.nonzero((t[:, 1] == ni) & (t[:, 3] == no))[:, 0]
            batch = x[t[idx, 0][:, None] + torch.arange(ni, device="cuda")[None, :]]   # [clips of the class, n_in]
            res = dev.resample_tensor(plan, batch[:, :, None], **kw)                     # one equal-length job
            flat_y[start[idx][:, None] + torch.arange(no, device="cuda")[None, :]] = res[:, :no, 0]
        out["solo_" + name] = flat_y.cpu().numpy()
    torch.cuda.synchronize()
    out["count_" + name] = np.array([int(counter.item()) if counter is not None else -1, int(solo_count.item())], np.int64)


def py_grad2(job, plans, log, out):
    """the double backward of dist.resample_ragged(..., kernel=KERNEL_EXACT, grad_kernel=KERNEL_ADJOINT) on float64 clips: its
    launches, and d/dw sum(A^T w) against A 1"""
    case = tuple(job["case"])
    plan = plans.setdefault(case, dev.Plan(*case))
    rng = np.random.default_rng(int(job["seed"]))
    clips = [torch.from_numpy(rng.standard_normal(n)).cuda().requires_grad_(True) for n in job["lengths"]]

    def f(*cs):
        return torch.cat(dist.resample_ragged(plan, list(cs), kernel=_native.KERNEL_EXACT, grad_kernel=_native.KERNEL_ADJOINT))
    y = f(*clips)
    w = torch.from_numpy(rng.standard_normal(y.shape[0])).cuda().requires_grad_(True)
    gx = torch.autograd.grad(y, clips, grad_outputs=w, create_graph=True)
    torch.cuda.synchronize()
    log.tail()
    ggw, = torch.autograd.grad(torch.cat(gx).sum(), w)   # the adjoint's backward: the ragged forward on the exact engine
    torch.cuda.synchronize()
    out["log_" + job["name"]] = np.array(log.tail().strip())
    with torch.no_grad():  # d/dw sum(A^T w) = A 1
        want = f(*[torch.ones_like(c) for c in clips])
    out["ggw_" + job["name"]], out["ggw_want_" + job["name"]] = ggw.cpu().numpy(), want.cpu().numpy()


def main():
    with open(sys.argv[1]) as f:
        jobs = json.load(f)
    log = Log(os.environ["HIPSOXR_DEBUG_LAUNCH_LOG"])
    plans, out = {}, {}
    for job in jobs:
        kind = job.get("kind", "table")
        if kind == "table":
            table_job(job, plans, log, out)
        elif kind == "py_forward":
            py_forward(job, plans, log, out)
        elif kind == "py_grad2":
            py_grad2(job, plans, log, out)
        elif kind == "py_batch":
            py_batch(job, plans, log, out)
        else:
            raise ValueError(kind)
    np.savez(sys.argv[2], **out)
    print("RAGGED_INTERP_PROBE done: %d jobs" % len(jobs))


if __name__ == "__main__":
    main()
