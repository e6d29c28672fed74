"""Helper of tests/test_gpu_ragged_exact.py: runs ragged FORWARD jobs (hipsoxr_run_device with a clip_table) on the GPU
under the process's HIPSOXR_* environment — the debug-switch build with HIPSOXR_DEBUG_LAUNCH_LOG — and writes what it ran
and what came out to an .npz:

    python tests/_ragged_exact_probe.py JOBS.json RESULTS.npz

JOBS.json is a list of jobs.  A job without "kind" is a raw table job
    {"name", "case": [in_rate, out_rate, quality], "dtype": "f32" | "f64" | "i32" | "i16", "ch", "kernel", "seed",
     "clips": [[a, b, c, cut, t], ...], "cap": bool, "layout": "packed" | "odd" | "al4" | "split" | "strided",
     "table_dev": bool, "dither": bool, "dither_seed", "data": "normal" | "square", "counter": bool,
     "solo": "clip" | "class" | "none", "pilot": selector of the one-clip job below (default: the job's own)}
A clip is to have a pb Lc + b Lc + c + t BIG outputs — Lc the replicated period and pb the periods per slab of the tiled
kernel, which only the launcher knows: they are read from the launch log of a one-clip ragged job of the same plan, type,
channel count and selector, and checked against the log of the job itself (the float32 planar kernel chooses pb by the
job's size: where it chose another, the lengths are made again with that one).  BIG = max(16 Lc, 4096), the least output
count at which AUTO takes a tile kernel; "cap" caps every clip at BIG - 1.  A plan without tile tables logs Lc = pb = 0.
in_frames is the least count whose output length reaches that; out_frames = the count - cut (cut > 0: a truncated clip).

Layouts (elements; S = the sentinel every buffer is pre-filled with): out always has ONE spare frame behind every clip.
    packed   clips back to back, frames of interleaved channels     odd / al4   the same, every clip's input offset moved
    split    channel planes [ch][sum frames], frame stride 1                    up to the next odd number / multiple of 4
    strided  input frames two frames apart (S in between)

Per job: `table_<name>` [clips, 4] as passed, `geom_<name>` = (Lc, pb, BIG, in frame stride, in channel stride, out frame
stride, out channel stride), `x_<name>` and `y_<name>` the whole buffers as they lay in memory, `log_<name>` the launch
log's lines of the job, `count_<name>` (ragged clip counter, sum of the counters of every clip run alone with its own out_frames) and `solo_<name>`: every clip's
first out_frames frames [out_frames, ch] of device.resample_tensor(..., kernel=KERNEL_EXACT) on the clip alone, concatenated
("class": the clips of one length as one equal-length batch, mono jobs).

Jobs with "kind" go through the Python surface (see each function below).  Nothing is compared here."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "python-soxr_amd"))
import torch  # noqa: E402
import ctypes as C  # noqa: E402
from soxr_amd import _native, device as dev, dist  # noqa: E402

DTYPE = {"f32": torch.float32, "f64": torch.float64, "i32": torch.int32, "i16": torch.int16}
SENTINEL = {"f32": 12345.0, "f64": 12345.0, "i32": 1234567, "i16": 12345}
EXACT_KERNELS = ("tile_mfma_p", "tile_mfma64_p", "tile_mfma", "tile", "gather")


class Log:
    def __init__(self, path):
        self.path, self.pos = path, 0

    def tail(self):
        if not os.path.exists(self.path):
            return ""
        with open(self.path) as f:
            f.seek(self.pos)
            txt = f.read()
        self.pos += len(txt)
        return txt


def fields(line):
    return dict(tok.split("=", 1) for tok in line.split())


def run_table(plan, in_ptr, out_ptr, dtype, ch, table, in_s, out_s, kernel, table_dev=None, dither=False, seed=0, counter=None):
    """hipsoxr_run_device on a clip table; strides = (frame, channel) in elements"""
    t = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 4)
    j = _native.Job()
    j.in_, j.out, j.elem, j.kernel = in_ptr, out_ptr, dev._torch_elem(dtype), kernel
    j.n_clips, j.n_channels = t.shape[0], ch
    j.in_frame_stride, j.in_chan_stride = in_s
    j.out_frame_stride, j.out_chan_stride = out_s
    j.in_abs0, j.out_k0 = 0, 0
    j.in_frames, j.out_frames = int(t[:, 1].max()), int(t[:, 3].max())
    j.clip_table, j.clip_table_dev = t.ctypes.data, table_dev
    j.dither, j.dither_seed = int(bool(dither)), int(seed)
    j.clip_counter = counter
    _native.check(_native.lib.hipsoxr_run_device(plan.handle, C.byref(j), torch.cuda.current_stream().cuda_stream))


def in_frames_for(plan, n_out):
    if n_out <= 0:
        return 0
    n = max(0, n_out * plan.M // plan.L - 2)
    while plan.out_len(n) < n_out:
        n += 1
    return n


def make_data(kind, rng, n, ch, dtype):
    if kind == "square":  # full-scale square wave: the filter's overshoot saturates an integer output
        k = np.arange(n)[:, None] + 7 * np.arange(ch)[None, :]
        v = np.where((k // 40) % 2 == 0, 1.0, -1.0)
    else:
        v = rng.standard_normal((n, ch)) * 0.25
    if dtype == torch.int16:
        return torch.from_numpy(np.clip(np.rint(v * 32767), -32768, 32767).astype(np.int16))
    if dtype == torch.int32:
        return torch.from_numpy(np.clip(np.rint(v * 2147483647), -2147483648, 2147483647).astype(np.int32))
    return torch.from_numpy(v).to(dtype)


def table_job(job, plans, pilots, log, out):
    name, case, ch, dtype, kernel = job["name"], tuple(job["case"]), int(job["ch"]), DTYPE[job["dtype"]], int(job["kernel"])
    plan = plans.setdefault(case, dev.Plan(*case))
    pilot_kernel = int(job.get("pilot", kernel))  # (a job that forces k_gather on long clips takes its units from the tile kernel's log)
    key = (case, job["dtype"], ch, pilot_kernel)
    if key not in pilots:  # one clip of 60 000 frames (a tile kernel's where the plan has one): Lc and a first pb
        x = torch.zeros((60000, ch), dtype=dtype, device="cuda")
        y = torch.zeros((plan.out_len(60000), ch), dtype=dtype, device="cuda")
        log.tail()
        run_table(plan, x.data_ptr(), y.data_ptr(), dtype, ch, [[0, 60000, 0, y.shape[0]]], (ch, 1), (ch, 1), pilot_kernel)
        torch.cuda.synchronize()
        f = fields(log.tail().strip())  # (no Lc there: the job is not the ragged exact launcher's — lengths are given outright)
        pilots[key] = (int(f.get("Lc", 0)), int(f.get("pb", 0)))
    lc, pb = pilots[key]
    big = max(16 * lc, 4096)
    sent, layout = SENTINEL[job["dtype"]], job.get("layout", "packed")
    for attempt in range(2):
        want = [a * pb * lc + b * lc + c + t * big for a, b, c, _, t in job["clips"]]
        if job.get("cap"):
            want = [min(w, big - 1) for w in want]
        n_in = [in_frames_for(plan, w) for w in want]
        n_out = [w - cl[3] for w, cl in zip(want, job["clips"])]
        assert min(n_out) >= 0 and all(o <= plan.out_len(i) for o, i in zip(n_out, n_in)), (name, lc, pb, n_out)
        rng = np.random.default_rng(int(job["seed"]))
        data = [make_data(job.get("data", "normal"), rng, n, ch, dtype) for n in n_in]
        out_fr = np.concatenate([[0], np.cumsum(np.array(n_out) + 1)[:-1]]).astype(np.int64)
        in_fr = np.concatenate([[0], np.cumsum(n_in)[:-1]]).astype(np.int64)
        si, so = max(int(sum(n_in)), 1), int(sum(n_out)) + len(n_out)
        if layout == "split":
            in_s, out_s, in_off, out_off, in_len, out_len = (1, si), (1, so), in_fr, out_fr, ch * si, ch * so
        elif layout == "strided":
            in_s, out_s, in_off, out_off, in_len, out_len = (2 * ch, 1), (ch, 1), 2 * ch * in_fr, ch * out_fr, 2 * ch * si, ch * so
        else:
            in_s, out_s, out_off, out_len = (ch, 1), (ch, 1), ch * out_fr, ch * so
            in_off, pos = [], 0
            for n in n_in:
                while (layout == "odd" and pos % 2 == 0) or (layout == "al4" and pos % 4):
                    pos += 1
                in_off.append(pos)
                pos += n * ch
            in_off, in_len = np.array(in_off, np.int64), max(pos, 1)
        x = torch.full((in_len,), sent, dtype=dtype)
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
        got = [int(fields(ln).get("pb", 0)) for ln in lines.split("\n") if ln]
        if not got or got[0] == pb or got[0] == 0:
            break
        assert attempt == 0, "the launcher's pb did not settle: %r" % lines
        pb = got[0]
    out["table_" + name] = table
    out["geom_" + name] = np.array([lc, pb, big, in_s[0], in_s[1], out_s[0], out_s[1]], np.int64)
    out["x_" + name], out["y_" + name], out["log_" + name] = x.cpu().numpy(), y.cpu().numpy(), np.array(lines)
    solo, solo_count = job.get("solo", "clip"), torch.zeros(1, dtype=torch.int64, device="cuda")
    kw = dict(kernel=_native.KERNEL_EXACT, dither=job.get("dither", False), dither_seed=job.get("dither_seed", 0))
    if counter is not None:  # the per-clip counts: each clip alone as a job of its own out_frames (a truncated clip's cut outputs are not made)
        for d, o, n in zip(data, n_out, n_in):
            if o:
                xd, yd = d.cuda(), torch.empty((o, ch), dtype=dtype, device="cuda")
                plan.run(xd.data_ptr(), yd.data_ptr(), dev._torch_elem(dtype), 1, ch, n, o, (0, ch, 1), (0, ch, 1),
                         stream=torch.cuda.current_stream().cuda_stream, kernel=_native.KERNEL_EXACT, clip_counter=solo_count.data_ptr(),
                         dither=kw["dither"], dither_seed=kw["dither_seed"])
                torch.cuda.synchronize()
    if solo == "clip":
        parts = [dev.resample_tensor(plan, d.cuda(), **kw)[:o] for d, o, n in zip(data, n_out, n_in) if n]
        parts = iter(parts)
        full = [next(parts) if n else torch.zeros((0, ch), dtype=dtype, device="cuda") for n in n_in]
        out["solo_" + name] = torch.cat([p.reshape(-1) for p in full]).cpu().numpy()
    elif solo == "class":
        assert ch == 1 and layout == "packed"
        flat = torch.zeros(int(sum(n_out)), dtype=dtype, device="cuda")
        start = torch.from_numpy(np.concatenate([[0], np.cumsum(n_out)[:-1]]).astype(np.int64)).cuda()
        t = torch.from_numpy(table).cuda()
        for ni, no in sorted(set(zip(n_in, n_out))):
            if no == 0:
                continue
            idx = torch.nonzero((t[:, 1] == ni) & (t[:, 3] == no))[:, 0]
            batch = x[t[idx, 0][:, None] + torch.arange(ni, device="cuda")[None, :]]   # [clips of the class, n_in]
            res = dev.resample_tensor(plan, batch[:, :, None], **kw)                     # one equal-length job
            flat[start[idx][:, None] + torch.arange(no, device="cuda")[None, :]] = res[:, :no, 0]
        out["solo_" + name] = flat.cpu().numpy()
    torch.cuda.synchronize()
    out["count_" + name] = np.array([int(counter.item()) if counter is not None else -1, int(solo_count.item())], np.int64)


def py_forward(job, plans, log, out):
    """dist.resample_ragged(plan, clips, kernel): the packed result, the per-clip results, the log"""
    case, dtype, ch = tuple(job["case"]), DTYPE[job["dtype"]], int(job["ch"])
    plan = plans.setdefault(case, dev.Plan(*case))
    rng = np.random.default_rng(int(job["seed"]))
    clips = [make_data("normal", rng, n, ch, dtype).cuda() for n in job["lengths"]]
    if ch == 1:
        clips = [c[:, 0] for c in clips]
    torch.cuda.synchronize()
    log.tail()
    ys = dist.resample_ragged(plan, clips, kernel=int(job["kernel"]))
    torch.cuda.synchronize()
    out["log_" + job["name"]] = np.array(log.tail().strip())
    out["y_" + job["name"]] = torch.cat([y.reshape(-1) for y in ys]).cpu().numpy()
    solo = [dev.resample_tensor(plan, c, kernel=_native.KERNEL_EXACT) if c.shape[0] else c[:0] for c in clips]
    out["solo_" + job["name"]] = torch.cat([y.reshape(-1) for y in solo]).cpu().numpy()
    out["x_" + job["name"]] = torch.cat([c.reshape(-1) for c in clips]).cpu().numpy()


def py_grad(job, plans, log, out):
    """gradcheck of dist.resample_ragged on float64, and the launches of a double backward"""
    case = tuple(job["case"])
    plan = plans.setdefault(case, dev.Plan(*case))
    rng = np.random.default_rng(int(job["seed"]))
    clips = [torch.from_numpy(rng.standard_normal(n)).cuda().requires_grad_(True) for n in job["lengths"]]

    def f(*cs):
        return torch.cat(dist.resample_ragged(plan, list(cs), kernel=_native.KERNEL_EXACT))
    out["gradcheck_" + job["name"]] = np.array(bool(torch.autograd.gradcheck(f, clips, eps=1e-6, atol=1e-8, rtol=1e-6, raise_exception=False)))
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


def py_batch(job, plans, log, out):
    """dist.resample_batch on a host corpus (several blocks of the staging ring): results, the block count, the log"""
    in_rate, out_rate, quality = job["case"]
    rng = np.random.default_rng(int(job["seed"]))
    ch = int(job["ch"])
    clips = [make_data("normal", rng, n, ch, torch.int16).numpy() for n in job["lengths"]]
    if ch == 1:
        clips = [c[:, 0] for c in clips]
    n_in = [int(c.shape[0]) for c in clips]
    blocks = dist._PipeRun(n_in, n_in, ch, 2, int(job["block_bytes"]), 3).blocks
    log.tail()
    res = dist.resample_batch(clips, in_rate, out_rate, quality, devices=[0], block_bytes=int(job["block_bytes"]))
    torch.cuda.synchronize()
    out["log_" + job["name"]] = np.array(log.tail().strip())
    out["blocks_" + job["name"]] = np.array([len(b) for b in blocks], np.int64)
    out["y_" + job["name"]] = np.concatenate([np.asarray(r).reshape(-1) for r in res])
    out["x_" + job["name"]] = np.concatenate([c.reshape(-1) for c in clips])


def main():
    with open(sys.argv[1]) as f:
        jobs = json.load(f)
    log = Log(os.environ["HIPSOXR_DEBUG_LAUNCH_LOG"])
    plans, pilots, out = {}, {}, {}
    for job in jobs:
        kind = job.get("kind", "table")
        if kind == "table":
            table_job(job, plans, pilots, log, out)
        elif kind == "py_forward":
            py_forward(job, plans, log, out)
        elif kind == "py_grad":
            py_grad(job, plans, log, out)
        elif kind == "py_batch":
            py_batch(job, plans, log, out)
        else:
            raise ValueError(kind)
    np.savez(sys.argv[2], **out)
    print("RAGGED_EXACT_PROBE done: %d jobs" % len(jobs))


if __name__ == "__main__":
    main()
