"""Helper of tests/test_gpu_ragged_two_stage.py: runs float clip tables of interpolated-phase plans under KERNEL_AUTO (the
two-stage form on a clip table, csrc/twostage.hip launch_two_stage_ragged) on the GPU under the process's HIPSOXR_* environment
— the debug-switch build with HIPSOXR_DEBUG_LAUNCH_LOG — and writes what it ran and what came out to an .npz:

    python tests/_ragged_two_stage_probe.py JOBS.json RESULTS.npz

A table job is {"name", "case": [in_rate, out_rate, quality], "dtype": "f32" | "f64", "ch", "seed", "layout": "packed" | "split" |
"rows"}.  Its nine clips are stated in OUTPUT frames, with U = 256 R the outputs of one polyphase tile — R is the launcher's:
the lengths are first made with R = 2 (R = 1 under HIPSOXR_DEBUG_POLY_R=1) and made again with the R of the job's own poly log
line until the two agree (R follows the longest clip, which follows U: a few rounds at the most) — and m U - 1 outputs the least such count admitted (8192 frames or more on both sides), plus one:
    0 the smallest admitted clip (8192 frames on its shorter side)      1 m U      2 m U - 1      3 (m + 5) U + 77, the longest
    4 m U + 1      5 (m + 2) U + 10 wanted, truncated 7 outputs below out_len      6 empty      7 about 100 outputs (short)
    8 one frame below admission (8191 frames on its shorter side: short)
in_frames is the least count whose output length reaches the wanted one.  Layouts: packed (mono, clips end to end, one spare
frame behind every output clip), split (planar channels a whole buffer apart), rows (mono; every output clip a row of a wider
buffer of one pitch).  Every buffer is pre-filled with a sentinel and returned as it lay in memory.
Per job: `table_`, `x_`, `y_`, `log_`, `geom_` = (U, m, 0, in channel stride, out channel stride, CUs), `short_` = the
non-empty clips the form does not admit run alone under KERNEL_EXACT (flat), `autodiff_` = per clip, the largest difference to the
clip run alone under KERNEL_AUTO (recorded for the notes, -1 where not run).
Jobs with "kind": "py_ragged" (dist.resample_ragged under defaults, its per-clip solo results, and the double backward with
grad_kernel=KERNEL_ADJOINT) and "py_batch" (dist.resample_batch on a float32 host corpus).  Nothing is compared here."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ragged_exact_probe import DTYPE, SENTINEL, Log, fields, in_frames_for, run_table  # noqa: E402
import torch  # noqa: E402
from soxr_amd import _native, device as dev, dist  # noqa: E402

AUTO = _native.KERNEL_AUTO


def clip_lengths(plan, u):
    """-> (m, [(in_frames, out_frames)] of the nine clips) for tiles of u outputs"""
    up = plan.out_len(100000) > 100000
    m = -(-8192 // u)
    while in_frames_for(plan, m * u - 1) < 8192:  # (up: the clip's shorter side is its input)
        m += 1
    m += 1

    def edge(frames):  # `frames` on the clip's shorter side
        if up:
            return frames, plan.out_len(frames)
        return in_frames_for(plan, frames), frames

    def out(want, cut=0):
        return in_frames_for(plan, want), want - cut
    return m, [edge(8192), out(m * u), out(m * u - 1), out((m + 5) * u + 77), out(m * u + 1), out((m + 2) * u + 10, 7), (0, 0), out(100), edge(8191)]


def table_job(job, plans, log, out):
    name, case, ch, dtype = job["name"], tuple(job["case"]), int(job["ch"]), DTYPE[job["dtype"]]
    plan = plans.setdefault(case, dev.Plan(*case))
    assert plan.phases != 0, "an interpolated-phase plan"
    sent, layout = SENTINEL[job["dtype"]], job.get("layout", "packed")
    u = int(job["u"]) if "u" in job else 256 * (1 if os.environ.get("HIPSOXR_DEBUG_POLY_R") == "1" else 2)  # ("u": the table of another run)
    for attempt in range(6):
        m, lens = clip_lengths(plan, u)
        lens += [lens[0]] * int(job.get("extra", 0))  # (more clips of the smallest admitted size)
        n_in, n_out = [a for a, _ in lens], [b for _, b in lens]
        assert all(o <= plan.out_len(i) for i, o in lens)
        rng = np.random.default_rng(int(job["seed"]))
        data = [torch.from_numpy(rng.standard_normal((n, ch)) * 0.25).to(dtype) for n in n_in]
        si, so = int(sum(n_in)), int(sum(n_out)) + len(n_out)
        in_fr = np.concatenate([[0], np.cumsum(n_in)[:-1]]).astype(np.int64)
        out_fr = np.concatenate([[0], np.cumsum(np.array(n_out) + 1)[:-1]]).astype(np.int64)
        if layout == "split":      # planar channels: the channel stride is the whole buffer of one channel
            in_chs, out_chs, in_len, out_len = si, so, ch * si, ch * so
        elif layout == "rows":     # every output clip a row of a wider buffer
            assert ch == 1
            pitch = max(n_out) + 37
            out_fr = np.arange(len(n_out), dtype=np.int64) * pitch
            in_chs, out_chs, in_len, out_len = 0, 0, si, len(n_out) * pitch
        else:
            assert ch == 1
            in_chs, out_chs, in_len, out_len = 0, 0, si, so
        x = torch.full((in_len,), sent, dtype=dtype)
        for d, off, n in zip(data, in_fr, n_in):
            for c in range(ch):
                x[int(off) + c * in_chs:int(off) + c * in_chs + n] = d[:, c]
        x = x.cuda()
        y = torch.full((out_len,), sent, dtype=dtype, device="cuda")
        table = np.ascontiguousarray(np.stack([in_fr, n_in, out_fr, n_out], axis=1), dtype=np.int64)
        torch.cuda.synchronize()
        log.tail()
        run_table(plan, x.data_ptr(), y.data_ptr(), dtype, ch, table, (1, max(in_chs, 1)), (1, max(out_chs, 1)), AUTO)
        torch.cuda.synchronize()
        lines = log.tail().strip()
        got = [int(fields(ln)["R"]) for ln in lines.split("\n") if ln.startswith("kernel=poly")]
        if not got or 256 * got[0] == u or "u" in job:
            break
        assert attempt < 5, "the launcher's R did not settle: %r" % lines
        u = 256 * got[0]
    out["table_" + name] = table
    out["geom_" + name] = np.array([u, m, 0, in_chs, out_chs, torch.cuda.get_device_properties(0).multi_processor_count], np.int64)
    out["x_" + name], out["y_" + name], out["log_" + name] = x.cpu().numpy(), y.cpu().numpy(), np.array(lines)
    # the clips alone: the short ones on the exact engine (their engine, bit for bit); the admitted ones under AUTO (recorded)
    short, autodiff = [], []
    yh = y.cpu()
    for c, (d, n, o) in enumerate(zip(data, n_in, n_out)):
        admitted = min(n, o) >= 8192
        if o == 0:
            autodiff.append(-1.)
            continue
        dd = d.cuda() if ch > 1 else d[:, 0].contiguous().cuda()
        if not admitted:
            short.append(dev.resample_tensor(plan, dd, kernel=_native.KERNEL_EXACT)[:o].reshape(o, ch).cpu().numpy())
            autodiff.append(-1.)
        elif job.get("solo_auto", True):
            alone = dev.resample_tensor(plan, dd)[:o].reshape(o, ch).cpu()
            mine = torch.stack([yh[int(out_fr[c]) + k * out_chs:int(out_fr[c]) + k * out_chs + o] for k in range(ch)], dim=1)
            autodiff.append(float((alone.double() - mine.double()).abs().max()))
        else:
            autodiff.append(-1.)
    out["short_" + name] = np.concatenate([s.reshape(-1) for s in short]) if short else np.zeros(0, x.cpu().numpy().dtype)
    out["autodiff_" + name] = np.array(autodiff)
    torch.cuda.synchronize()


def py_ragged(job, plans, log, out):
    """dist.resample_ragged(plan, clips) under defaults on float32 mono clips, and its double backward with KERNEL_ADJOINT"""
    case, name = tuple(job["case"]), job["name"]
    plan = plans.setdefault(case, dev.Plan(*case))
    rng = np.random.default_rng(int(job["seed"]))
    clips = [torch.from_numpy((rng.standard_normal(n) * 0.25).astype(np.float32)).cuda() for n in job["lengths"]]
    torch.cuda.synchronize()
    log.tail()
    ys = dist.resample_ragged(plan, clips)
    torch.cuda.synchronize()
    out["log_" + name] = np.array(log.tail().strip())
    out["x_" + name] = torch.cat(clips).cpu().numpy()
    out["y_" + name] = torch.cat([y.reshape(-1) for y in ys]).cpu().numpy()
    out["nout_" + name] = np.array([int(y.shape[0]) for y in ys], np.int64)
    solo = [dev.resample_tensor(plan, c, kernel=_native.KERNEL_EXACT) if c.shape[0] else c[:0] for c in clips]
    out["exact_" + name] = torch.cat([y.reshape(-1) for y in solo]).cpu().numpy()
    # the double backward (float64, small clips): d/dw sum(A^T w) = A 1
    small = [torch.from_numpy(rng.standard_normal(n)).cuda().requires_grad_(True) for n in job["grad_lengths"]]

    def f(*cs):
        return torch.cat(dist.resample_ragged(plan, list(cs), grad_kernel=_native.KERNEL_ADJOINT))
    yy = f(*small)
    w = torch.from_numpy(rng.standard_normal(yy.shape[0])).cuda().requires_grad_(True)
    gx = torch.autograd.grad(yy, small, grad_outputs=w, create_graph=True)
    ggw, = torch.autograd.grad(torch.cat(gx).sum(), w)
    torch.cuda.synchronize()
    log.tail()
    with torch.no_grad():
        want = torch.cat(dist.resample_ragged(plan, [torch.ones_like(c) for c in small], kernel=_native.KERNEL_EXACT))
    out["ggw_" + name], out["ggw_want_" + name] = ggw.cpu().numpy(), want.cpu().numpy()


def py_batch(job, plans, log, out):
    """dist.resample_batch on a float32 mono host corpus: results, the log"""
    in_rate, out_rate, quality = job["case"]
    rng = np.random.default_rng(int(job["seed"]))
    clips = [(rng.standard_normal(n) * 0.25).astype(np.float32) for n in job["lengths"]]
    log.tail()
    res = dist.resample_batch(clips, in_rate, out_rate, quality, devices=[0])
    torch.cuda.synchronize()
    out["log_" + job["name"]] = np.array(log.tail().strip())
    out["x_" + job["name"]] = np.concatenate(clips)
    out["y_" + job["name"]] = np.concatenate([np.asarray(r).reshape(-1) for r in res])


def main():
    with open(sys.argv[1]) as f:
        jobs = json.load(f)
    log = Log(os.environ["HIPSOXR_DEBUG_LAUNCH_LOG"])
    plans, out = {}, {}
    for job in jobs:
        {"table": table_job, "py_ragged": py_ragged, "py_batch": py_batch}[job.get("kind", "table")](job, plans, log, out)
    np.savez(sys.argv[2], **out)
    print("RAGGED_TWO_STAGE_PROBE done: %d jobs" % len(jobs))


if __name__ == "__main__":
    main()
