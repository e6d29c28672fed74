"""Helper of tests/test_gpu_vr_ragged.py: runs ragged VARIABLE-RATE jobs (hipsoxr_run_device_vr_ragged: a clip table on a
variable-rate plan, an io ratio per clip) on the GPU under the process's HIPSOXR_* environment — the debug-switch build with
HIPSOXR_DEBUG_LAUNCH_LOG — and writes what it ran and what came out to an .npz:

    python tests/_vr_ragged_probe.py JOBS.json RESULTS.npz

JOBS.json is a list of jobs.  A job without "kind" is a raw table job
    {"name", "case": [in_rate, out_rate, quality], "dtype": "f32" | "f64" | "i32" | "i16", "ch", "kernel", "seed",
     "unit": 256 | 32 | "KO", "clips": [[m, add, cut] | ["in", n_in, cut], ...], "ratios": [io ratio per clip],
     "layout": "packed" | "split" | "strided", "table_dev": bool, "dither": bool, "dither_seed", "data": "normal" | "square",
     "counter": bool, "ref": bool}
A clip [m, add, cut] is to have m U + add outputs — U the outputs of one column per workgroup of the kernel form the job is to
reach: 256 (k_interp), 32 (k_interp_wave), or "KO" (k_interp_tile), which only the launcher's cost model knows: the lengths
are first made with KO = 30 P, and made again ONCE with the KO the job's own log line shows where that differs.  in_frames is
the least count whose Plan.vr_out_len at the clip's ratio reaches m U + add; out_frames = that - cut (cut > 0: a truncated
clip).  ["in", n_in, cut]: n_in input frames outright, out_frames = vr_out_len - cut.

Buffers: every one is pre-filled with a sentinel.  ONE spare frame lies behind every clip of the output, and one behind every
clip of the input (a read past a clip's end meets it).  Layouts as in tests/_ragged_exact_probe.py (packed / split / strided).

Per job: `table_<name>`, `ratios_<name>`, `geom_<name>` = (U, in frame stride, in channel stride, out frame stride, out
channel stride), `x_<name>` and `y_<name>` the whole buffers as they lay in memory, `log_<name>` the launch log's lines of the
job, `count_<name>` = (the job's clip counter or -1, the sum of the per-clip streams' num_clips(), the counter of the same
clips run once more with every out_frames = vr_out_len — `full_<name>`, packed: a stream counts all of its frames), and reference A —
`refa_<name>`: what a fresh TensorStream(..., vr=True) with the job's dither and seed returns after set_io_ratio(r, 1.0) when it
is fed each clip with last=True, concatenated (all of its frames), `refa_len_<name>` its frame count per clip.

Jobs with "kind": "guard" (a constant-rate ragged job of an interpolated-phase plan and a variable-rate TensorStream run:
what they return, to be asked before and after the jobs above), "fold" (65536 mono clips of 3 frames: one job, and the same
table as two jobs) and "py" (the Python surface).  Nothing is compared here."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ragged_exact_probe import DTYPE, SENTINEL, Log, fields, make_data, run_table  # noqa: E402
import torch  # noqa: E402
from soxr_amd import _native, device as dev, dist  # noqa: E402


def in_frames_for(plan, n_out, ratio):
    """the least input length whose output length at `ratio` reaches n_out"""
    if n_out <= 0:
        return 0
    n = max(0, int(n_out * ratio) - 2)
    while plan.vr_out_len(n, ratio) < n_out:
        n += 1
    return n


def stream_of(case, ch, dtype, dither, seed, ratio):
    ts = dev.TensorStream(case[0], case[1], ch, dtype, case[2], vr=True, dither=dither, dither_seed=seed)
    ts.set_io_ratio(ratio, 1.0)
    return ts


def table_job(job, plans, log, out):
    name, case, ch, dtype, kernel = job["name"], tuple(job["case"]), int(job["ch"]), DTYPE[job["dtype"]], int(job["kernel"])
    plan = plans.setdefault(case, dev.Plan(*case, vr=True))
    ratios = [float(r) for r in job["ratios"]]
    assert len(ratios) == len(job["clips"])
    unit = job.get("unit", 0)
    u = 30 * plan.phases if unit == "KO" else int(unit)
    sent, layout = SENTINEL[job["dtype"]], job.get("layout", "packed")
    dither, seed = bool(job.get("dither", False)), int(job.get("dither_seed", 0))
    for attempt in range(2):
        n_in, n_out = [], []
        for (m, add, cut), r in zip(job["clips"], ratios):
            if m == "in":
                n_in.append(int(add))
                n_out.append(plan.vr_out_len(int(add), r) - cut)
            else:
                n_in.append(in_frames_for(plan, m * u + add, r))
                n_out.append(m * u + add - cut)
        assert min(n_out) >= 0 and all(o <= plan.vr_out_len(i, r) for o, i, r in zip(n_out, n_in, ratios)), (name, u, n_out)
        rng = np.random.default_rng(int(job["seed"]))
        data = [make_data(job.get("data", "normal"), rng, n, ch, dtype) for n in n_in]
        out_fr = np.concatenate([[0], np.cumsum(np.array(n_out) + 1)[:-1]]).astype(np.int64)
        in_fr = np.concatenate([[0], np.cumsum(np.array(n_in) + 1)[:-1]]).astype(np.int64)
        si, so = int(sum(n_in)) + len(n_in), int(sum(n_out)) + len(n_out)
        if layout == "split":
            in_s, out_s, in_off, out_off, in_len, out_len = (1, si), (1, so), in_fr, out_fr, ch * si, ch * so
        elif layout == "strided":
            in_s, out_s, in_off, out_off, in_len, out_len = (2 * ch, 1), (ch, 1), 2 * ch * in_fr, ch * out_fr, 2 * ch * si, ch * so
        else:
            in_s, out_s, in_off, out_off, in_len, out_len = (ch, 1), (ch, 1), ch * in_fr, ch * out_fr, ch * si, ch * so
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
        plan.run_vr_ragged(x.data_ptr(), y.data_ptr(), dev._torch_elem(dtype), ch, table, ratios, in_s, out_s,
                           stream=torch.cuda.current_stream().cuda_stream, kernel=kernel,
                           table_dev=table_dev.data_ptr() if table_dev is not None else None,
                           clip_counter=counter.data_ptr() if counter is not None else None, dither=dither, dither_seed=seed)
        torch.cuda.synchronize()
        lines = log.tail().strip()
        got = [int(fields(ln).get("KO", 0)) for ln in lines.split("\n") if ln]
        if unit != "KO" or not got or got[0] == u or got[0] == 0:
            break
        assert attempt == 0, "the launcher's KO did not settle: %r" % lines
        u = got[0]
    out["table_" + name], out["ratios_" + name] = table, np.array(ratios, np.float64)
    out["geom_" + name] = np.array([u, in_s[0], in_s[1], out_s[0], out_s[1]], np.int64)
    out["x_" + name], out["y_" + name], out["log_" + name] = x.cpu().numpy(), y.cpu().numpy(), np.array(lines)
    stream_count = 0
    if job.get("ref", True):  # reference A: the product's own variable-rate stream, clip by clip
        parts, lens = [], []
        for d, r in zip(data, ratios):
            ts = stream_of(case, ch, dtype, dither, seed, r)
            v = ts.resample_chunk(d.cuda() if ch > 1 else d[:, 0].cuda(), last=True)
            torch.cuda.synchronize()
            parts.append(v.reshape(-1).cpu().numpy())
            lens.append(int(v.shape[0]))
            if counter is not None:
                stream_count += ts.num_clips()
        out["refa_" + name], out["refa_len_" + name] = np.concatenate(parts), np.array(lens, np.int64)
    full_count = -1
    if counter is not None:  # a stream counts ALL its frames: the same clips once more with out_frames = vr_out_len, nothing cut
        n_full = [plan.vr_out_len(n, r) for n, r in zip(n_in, ratios)]
        fo = np.concatenate([[0], np.cumsum(n_full)[:-1]]).astype(np.int64)
        so = max(int(sum(n_full)), 1)
        full_s, full_off = ((1, so), fo) if layout == "split" else ((ch, 1), ch * fo)
        t_full = np.ascontiguousarray(np.stack([in_off, n_in, full_off, n_full], axis=1), dtype=np.int64)
        y_full, c_full = torch.empty(ch * so, dtype=dtype, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        plan.run_vr_ragged(x.data_ptr(), y_full.data_ptr(), dev._torch_elem(dtype), ch, t_full, ratios, in_s, full_s,
                           stream=torch.cuda.current_stream().cuda_stream, kernel=kernel, clip_counter=c_full.data_ptr(),
                           dither=dither, dither_seed=seed)
        torch.cuda.synchronize()
        log.tail()
        full_count = int(c_full.item())
        out["full_" + name] = y_full.cpu().numpy()
    out["count_" + name] = np.array([int(counter.item()) if counter is not None else -1, stream_count, full_count], np.int64)


def guard_job(job, plans, log, out):
    """what existed before: a constant-rate ragged job on an interpolated-phase plan (EXACT: the RAGGED forms of the same
    kernels, whose argument structs grew) and a variable-rate stream with a slew (the VR forms)"""
    name = job["name"]
    rng = np.random.default_rng(int(job["seed"]))
    plan = plans.setdefault(("const",) + tuple(job["case"]), dev.Plan(*job["case"]))
    assert plan.phases != 0
    n_in = [int(n) for n in job["lengths"]]
    n_out = [plan.out_len(n) for n in n_in]
    x = torch.from_numpy(rng.standard_normal(sum(n_in)).astype(np.float32) * 0.25).cuda()
    y = torch.full((sum(n_out) + 1,), 12345.0, dtype=torch.float32, device="cuda")
    in_off = np.concatenate([[0], np.cumsum(n_in)[:-1]])
    out_off = np.concatenate([[0], np.cumsum(n_out)[:-1]])
    table = np.ascontiguousarray(np.stack([in_off, n_in, out_off, n_out], axis=1), dtype=np.int64)
    log.tail()
    run_table(plan, x.data_ptr(), y.data_ptr(), torch.float32, 1, table, (1, 1), (1, 1), _native.KERNEL_EXACT)
    torch.cuda.synchronize()
    out["log_" + name] = np.array(log.tail().strip())
    out["ragged_" + name] = y.cpu().numpy()
    solo = [dev.resample_tensor(plan, x[o:o + n], kernel=_native.KERNEL_EXACT) for o, n in zip(in_off, n_in)]
    out["solo_" + name] = torch.cat(solo).cpu().numpy()
    ts = dev.TensorStream(44100, 16000, 1, torch.int16, "HQ", vr=True, dither=True, dither_seed=3)
    xs = torch.from_numpy((rng.standard_normal(9000) * 5000).astype(np.int16)).cuda()
    a = ts.resample_chunk(xs[:5000])
    ts.set_io_ratio(2.0, 1.0, 700)
    b = ts.resample_chunk(xs[5000:], last=True)
    torch.cuda.synchronize()
    out["stream_" + name] = torch.cat([a, b]).cpu().numpy()


def fold_job(job, plans, log, out):
    name, case = job["name"], tuple(job["case"])
    plan = plans.setdefault(case, dev.Plan(*case, vr=True))
    n, frames = int(job["n_clips"]), int(job["frames"])
    ratios = np.array([job["ratios"][i % len(job["ratios"])] for i in range(n)], np.float64)
    n_out = np.array([plan.vr_out_len(frames, r) for r in job["ratios"]], np.int64)[np.arange(n) % len(job["ratios"])]
    rng = np.random.default_rng(int(job["seed"]))
    x = torch.from_numpy(rng.standard_normal(n * frames).astype(np.float32) * 0.25).cuda()
    in_off = np.arange(n, dtype=np.int64) * frames
    out_off = np.concatenate([[0], np.cumsum(n_out + 1)[:-1]]).astype(np.int64)
    table = np.ascontiguousarray(np.stack([in_off, np.full(n, frames), out_off, n_out], axis=1), dtype=np.int64)
    total = int(n_out.sum()) + n
    st = torch.cuda.current_stream().cuda_stream
    y = torch.full((total,), 12345.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    log.tail()
    plan.run_vr_ragged(x.data_ptr(), y.data_ptr(), _native.F32, 1, table, ratios, (1, 1), (1, 1), stream=st, kernel=_native.KERNEL_EXACT)
    torch.cuda.synchronize()
    out["log_" + name] = np.array(log.tail().strip())
    y2 = torch.full((total,), 12345.0, dtype=torch.float32, device="cuda")
    h = int(job["cut"])
    for lo, hi in ((0, h), (h, n)):
        plan.run_vr_ragged(x.data_ptr(), y2.data_ptr(), _native.F32, 1, table[lo:hi], ratios[lo:hi], (1, 1), (1, 1), stream=st,
                           kernel=_native.KERNEL_EXACT)
    torch.cuda.synchronize()
    out["log2_" + name] = np.array(log.tail().strip())
    out["y_" + name], out["y2_" + name], out["table_" + name] = y.cpu().numpy(), y2.cpu().numpy(), table
    # ... and a few clips against the stream, so that the two equal results are the right ones
    picks = [0, 1, 2, 3, 65534, 65535, n - 1]
    ref = []
    for c in picks:
        ts = stream_of(case, 1, torch.float32, True, 0, float(ratios[c]))
        ref.append(ts.resample_chunk(x[c * frames:(c + 1) * frames], last=True).cpu().numpy())
    out["picks_" + name], out["pickref_" + name] = np.array(picks, np.int64), np.concatenate(ref)
    out["pickref_len_" + name] = np.array([len(r) for r in ref], np.int64)


def py_job(job, plans, log, out):
    """dist.resample_varispeed and dist.RaggedJob(io_ratios=...) on clips that are views of ONE buffer, the job on a second
    torch stream; reference A per clip"""
    name, case, ch = job["name"], tuple(job["case"]), int(job["ch"])
    dtype = DTYPE[job["dtype"]]
    plan = plans.setdefault(case, dev.Plan(*case, vr=True))
    rng = np.random.default_rng(int(job["seed"]))
    lengths, ratios = [int(n) for n in job["lengths"]], [float(r) for r in job["ratios"]]
    buf = make_data("normal", rng, sum(lengths) + 3 * len(lengths), ch, dtype).cuda()
    buf = buf if ch > 1 else buf[:, 0]
    clips, pos = [], 0
    for n in lengths:
        clips.append(buf[pos + 3:pos + 3 + n])
        pos += n + 3
    log.tail()
    ys = dist.resample_varispeed(plan, clips, ratios, dither=job.get("dither"), dither_seed=int(job.get("dither_seed", 0)))
    torch.cuda.synchronize()
    out["log_" + name] = np.array(log.tail().strip())
    side = torch.cuda.Stream()
    jb = dist.RaggedJob(plan, clips, kernel=_native.KERNEL_EXACT, stream=side, dither=job.get("dither"),
                        dither_seed=int(job.get("dither_seed", 0)), io_ratios=ratios)
    jb.launch()
    side.synchronize()
    torch.cuda.synchronize()
    out["inplace_" + name] = np.array([k.data_ptr() == c.data_ptr() for k, c in zip(jb._keep, clips) if c.shape[0]])
    out["lens_" + name] = np.array([int(y.shape[0]) for y in ys], np.int64)
    out["vs_" + name] = torch.cat([y.reshape(-1) for y in ys]).cpu().numpy()
    out["job_" + name] = torch.cat([y.reshape(-1) for y in jb.outputs()]).cpu().numpy()
    dith = (dtype == torch.int16) if job.get("dither") is None else bool(job["dither"])
    parts, lens = [], []
    for c, r in zip(clips, ratios):
        v = stream_of(case, ch, dtype, dith, int(job.get("dither_seed", 0)), r).resample_chunk(c, last=True)
        parts.append(v.reshape(-1).cpu().numpy())
        lens.append(int(v.shape[0]))
    out["refa_" + name], out["refa_len_" + name] = np.concatenate(parts), np.array(lens, np.int64)
    why = ""
    if dtype in (torch.float32, torch.float64):
        try:
            dist.resample_varispeed(plan, [clips[0].clone().requires_grad_(True)], ratios[:1])
        except RuntimeError as e:
            why = str(e)
    out["grad_" + name] = np.array(why)


def main():
    with open(sys.argv[1]) as f:
        jobs = json.load(f)
    log = Log(os.environ["HIPSOXR_DEBUG_LAUNCH_LOG"])
    plans, out = {}, {}
    kinds = {"table": table_job, "guard": guard_job, "fold": fold_job, "py": py_job}
    for job in jobs:
        kinds[job.get("kind", "table")](job, plans, log, out)
    np.savez(sys.argv[2], **out)
    print("VR_RAGGED_PROBE done: %d jobs" % len(jobs))


if __name__ == "__main__":
    main()
