"""Helper of tests/test_gpu_vr_ragged_adjoint.py: runs jobs of the ragged variable-rate adjoint
(hipsoxr_run_device_vr_ragged_adjoint) on the GPU under the process's HIPSOXR_* environment — the debug-switch build with
HIPSOXR_DEBUG_LAUNCH_LOG — and writes what it ran and what came out to an .npz:

    python tests/_vr_ragged_adjoint_probe.py JOBS.json RESULTS.npz

JOBS.json is a list of jobs; nothing is compared here.

"table" {"name", "case": [in_rate, out_rate, quality], "dtype": "f32" | "f64", "ch", "lengths": [n_x per clip], "ratios",
         "cuts": [c per clip: n_y = max(0, vr_out_len(n_x, ratio) - c); "all": n_y = 0], "seed", "kernel", "table_dev": bool,
         "solo": bool, "mono": bool, "poke": [[clip, k, "nan" | "inf"], ...]}
    The cotangents are cut from ONE buffer with GAP frames between them; the gradients go to one packed buffer with GAP frames
    between the clips' ranges and GUARD frames either side, all of it pre-filled with POISON.  -> table_, ratios_, gy_ and gx_
    (the whole buffers as they lay in memory), log_ (the job's launch-log lines); solo_: every clip once more as a table of
    its own, the clips' frames concatenated; mono_: every column of every clip as a mono one-row table, put back into
    [frames, ch]; poke_<i>: the whole gx buffer of the job run once more with that one cotangent sample replaced.
"fold"  {"name", "case", "n_clips", "frames", "ratios", "seed"}: n_clips mono float32 clips of `frames` frames, clip c at
    ratios[c % len(ratios)] and with that class's cotangent — more columns than one grid holds, one call.
"py"    {"name", "case", "lengths", "ratios", "seed"}: the Python surface on float64 — the forward, the operator, autograd.
"const" {"name"}: a constant-rate HIPSOXR_KERNEL_ADJOINT job on an interpolated-phase plan: its log line, as it always was."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ragged_exact_probe import Log  # noqa: E402
import torch  # noqa: E402
from soxr_amd import _native, device as dev, dist  # noqa: E402

GAP, GUARD, POISON = 3, 8, 12345.0
DTYPE = {"f32": torch.float32, "f64": torch.float64}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _run(plan, gy, gx, dtype, ch, table, ratios, kernel, table_dev=False):
    td = torch.from_numpy(np.ascontiguousarray(table, np.int64)).cuda() if table_dev else None
    plan.run_vr_ragged_adjoint(gy.data_ptr(), gx.data_ptr(), dev._torch_elem(dtype), ch, table, ratios, (ch, 1), (ch, 1),
                               stream=_stream(), kernel=kernel, table_dev=td.data_ptr() if td is not None else None)
    torch.cuda.synchronize()


def table_job(job, plans, log, out):
    name, case, ch, dtype, kernel = job["name"], tuple(job["case"]), int(job["ch"]), DTYPE[job["dtype"]], int(job["kernel"])
    plan = plans.setdefault(case, dev.Plan(*case, vr=True))
    n_x, ratios = [int(n) for n in job["lengths"]], [float(r) for r in job["ratios"]]
    n_y = [0 if c == "all" else max(0, plan.vr_out_len(n, r) - int(c)) for n, r, c in zip(n_x, ratios, job["cuts"])]
    rng = np.random.default_rng(int(job["seed"]))
    gy_fr = np.concatenate([[0], np.cumsum(np.array(n_y) + GAP)[:-1]]).astype(np.int64) + GAP
    gx_fr = np.concatenate([[0], np.cumsum(np.array(n_x) + GAP)[:-1]]).astype(np.int64) + GUARD
    gy_host = torch.full((int(sum(n_y)) + GAP * (len(n_y) + 1), ch), POISON, dtype=dtype)
    for o, n in zip(gy_fr, n_y):
        gy_host[o:o + n] = torch.from_numpy(rng.standard_normal((n, ch))).to(dtype)
    gx_frames = int(sum(n_x)) + GAP * len(n_x) + 2 * GUARD
    table = np.ascontiguousarray(np.stack([ch * gy_fr, n_y, ch * gx_fr, n_x], axis=1), dtype=np.int64)
    gy = gy_host.cuda()
    gx = torch.full((gx_frames, ch), POISON, dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    log.tail()
    _run(plan, gy, gx, dtype, ch, table, ratios, kernel, bool(job.get("table_dev")))
    out["log_" + name] = np.array(log.tail().strip())
    out["table_" + name], out["ratios_" + name] = table, np.array(ratios, np.float64)
    out["gy_" + name], out["gx_" + name] = gy.cpu().numpy(), gx.cpu().numpy()
    if job.get("solo"):  # every clip as a table of its own, into a poisoned buffer of its own
        parts = []
        for c in range(len(n_x)):
            one = torch.full((n_x[c] + 2 * GUARD, ch), POISON, dtype=dtype, device="cuda")
            _run(plan, gy, one, dtype, ch, np.array([[table[c, 0], n_y[c], ch * GUARD, n_x[c]]], np.int64), ratios[c:c + 1], kernel)
            parts.append(one.cpu().numpy())
        out["solo_" + name] = np.concatenate(parts)
    if job.get("mono"):  # every column of every clip alone, as a mono clip
        parts = []
        for c in range(len(n_x)):
            cols = []
            for k in range(ch):
                col = gy[gy_fr[c]:gy_fr[c] + n_y[c], k].contiguous()
                if n_y[c] == 0:
                    col = torch.zeros(1, dtype=dtype, device="cuda")  # (an empty tensor has no address)
                one = torch.full((n_x[c] + 1,), POISON, dtype=dtype, device="cuda")
                _run(plan, col, one, dtype, 1, np.array([[0, n_y[c], 0, n_x[c]]], np.int64), ratios[c:c + 1], kernel)
                cols.append(one[:n_x[c]].cpu().numpy())
            parts.append(np.stack(cols, axis=1))
        out["mono_" + name] = np.concatenate(parts)
    for i, (c, k, what) in enumerate(job.get("poke", [])):
        g2 = gy.clone()
        g2[gy_fr[c] + int(k), 0] = float(what)
        x2 = torch.full((gx_frames, ch), POISON, dtype=dtype, device="cuda")
        _run(plan, g2, x2, dtype, ch, table, ratios, kernel)
        out["poke_%s_%d" % (name, i)] = x2.cpu().numpy()
    log.tail()


def fold_job(job, plans, log, out):
    name, case = job["name"], tuple(job["case"])
    plan = plans.setdefault(case, dev.Plan(*case, vr=True))
    n, frames, cyc = int(job["n_clips"]), int(job["frames"]), [float(r) for r in job["ratios"]]
    cls = np.arange(n) % len(cyc)
    n_y_cls = np.array([plan.vr_out_len(frames, r) for r in cyc], np.int64)
    gy_off_cls = np.concatenate([[0], np.cumsum(n_y_cls + 1)[:-1]]).astype(np.int64)
    rng = np.random.default_rng(int(job["seed"]))
    gy_host = np.full(int(n_y_cls.sum()) + len(cyc), POISON, np.float32)
    for o, m in zip(gy_off_cls, n_y_cls):
        gy_host[o:o + m] = rng.standard_normal(m).astype(np.float32)
    gx_off = np.arange(n, dtype=np.int64) * (frames + 1)
    table = np.ascontiguousarray(np.stack([gy_off_cls[cls], n_y_cls[cls], gx_off, np.full(n, frames)], axis=1), dtype=np.int64)
    gy = torch.from_numpy(gy_host).cuda()
    gx = torch.full((n * (frames + 1),), POISON, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    log.tail()
    _run(plan, gy, gx, torch.float32, 1, table, np.array(cyc)[cls], _native.KERNEL_ADJOINT)
    out["log_" + name] = np.array(log.tail().strip())
    out["gy_" + name], out["gx_" + name], out["table_" + name] = gy_host, gx.cpu().numpy(), table


def py_job(job, plans, log, out):
    name, case = job["name"], tuple(job["case"])
    plan = plans.setdefault(case, dev.Plan(*case, vr=True))
    ADJ = _native.KERNEL_ADJOINT
    rng = np.random.default_rng(int(job["seed"]))
    lengths, ratios = [int(n) for n in job["lengths"]], [float(r) for r in job["ratios"]]
    buf = torch.from_numpy(rng.standard_normal(sum(lengths) + GAP * len(lengths))).cuda()
    clips, pos = [], 0
    for n in lengths:  # views of one buffer, with gaps
        clips.append(buf[pos + GAP:pos + GAP + n])
        pos += n + GAP
    cat = lambda ts: torch.cat([t.reshape(-1) for t in ts]).detach().cpu().numpy()
    ys = dist.resample_varispeed(plan, clips, ratios)
    ws = [torch.from_numpy(rng.standard_normal(int(y.shape[0]))).cuda() for y in ys]
    torch.cuda.synchronize()
    log.tail()
    gxs = dist.resample_varispeed_adjoint(plan, ws, lengths, ratios)
    torch.cuda.synchronize()
    out["log_" + name] = np.array(log.tail().strip())
    out["x_" + name], out["y_" + name], out["w_" + name], out["gx_" + name] = cat(clips), cat(ys), cat(ws), cat(gxs)
    out["ny_" + name] = np.array([int(y.shape[0]) for y in ys], np.int64)
    out["gxauto_" + name] = cat(dist.resample_varispeed_adjoint(plan, ws, lengths, ratios, kernel=ADJ))
    # autograd: every clip but the second requires grad
    leaves = [c.clone().requires_grad_(i != 1) for i, c in enumerate(clips)]
    yg = dist.resample_varispeed(plan, leaves, ratios, grad_kernel=ADJ)
    out["yg_" + name] = cat(yg)
    out["has_grad_fn_" + name] = np.array([y.grad_fn is not None for y in yg])
    wl = [w.clone().requires_grad_(True) for w in ws]
    loss = sum((y * w).sum() for y, w in zip(yg, wl))
    need = [c for c in leaves if c.requires_grad]
    log.tail()
    grads = torch.autograd.grad(loss, need, create_graph=True)
    torch.cuda.synchronize()
    out["log_backward_" + name] = np.array(log.tail().strip())
    out["grad_" + name] = cat(grads)
    out["grad_idx_" + name] = np.array([i for i, c in enumerate(leaves) if c.requires_grad], np.int64)
    loss.backward(retain_graph=True)  # (what a training step calls: a clip that does not require grad gets none)
    out["grad_none_" + name] = np.array([c.grad is None for c in leaves])
    # double backward: d/dw of sum_c <grad_c, v_c> is the forward on v, sliced to the cotangents' lengths
    vs = [torch.from_numpy(rng.standard_normal(int(g.shape[0]))).cuda() for g in grads]
    log.tail()
    gg = torch.autograd.grad(sum((g * v).sum() for g, v in zip(grads, vs)), [wl[i] for i in out["grad_idx_" + name]])
    torch.cuda.synchronize()
    out["log_double_" + name] = np.array(log.tail().strip())
    out["gg_" + name] = cat(gg)
    keep = [int(i) for i in out["grad_idx_" + name]]
    out["fwd_v_" + name] = cat(dist.resample_varispeed(plan, vs, [ratios[i] for i in keep], kernel=_native.KERNEL_EXACT))
    # the operator itself is differentiable: the backward of <A^T w, v> in w is A v
    wl2 = [ws[i].clone().requires_grad_(True) for i in keep]
    op = dist.resample_varispeed_adjoint(plan, wl2, [lengths[i] for i in keep], [ratios[i] for i in keep], kernel=ADJ)
    out["gop_" + name] = cat(torch.autograd.grad(sum((g * v).sum() for g, v in zip(op, vs)), wl2))
    # gradcheck: one float64 clip of 40 frames at ratio 1.0
    x40 = torch.from_numpy(rng.standard_normal(40)).cuda().requires_grad_(True)
    f = lambda c: dist.resample_varispeed(plan, [c], [1.0], grad_kernel=ADJ)[0]
    out["gradcheck_" + name] = np.array(bool(torch.autograd.gradcheck(f, [x40], eps=1e-6, atol=1e-8, rtol=1e-6, raise_exception=False)))
    log.tail()


def const_job(job, plans, log, out):
    plan = dev.Plan(48000, 44101, "HQ")
    gy = torch.from_numpy(np.random.default_rng(3).standard_normal(plan.out_len(300)).astype(np.float32)).cuda()
    torch.cuda.synchronize()
    log.tail()
    gx = dev.resample_tensor_adjoint(plan, gy, 300, kernel=_native.KERNEL_ADJOINT)
    torch.cuda.synchronize()
    out["log_" + job["name"]] = np.array(log.tail().strip())
    out["gx_" + job["name"]] = gx.cpu().numpy()


def main():
    with open(sys.argv[1]) as f:
        jobs = json.load(f)
    log = Log(os.environ["HIPSOXR_DEBUG_LAUNCH_LOG"])
    plans, out = {}, {}
    kinds = {"table": table_job, "fold": fold_job, "py": py_job, "const": const_job}
    for job in jobs:
        kinds[job.get("kind", "table")](job, plans, log, out)
    np.savez(sys.argv[2], **out)
    print("VR_RAGGED_ADJOINT_PROBE done: %d jobs" % len(jobs))


if __name__ == "__main__":
    main()
