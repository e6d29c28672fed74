"""Helper of tests/test_gpu_ragged_strided.py: runs clip tables of INTERLEAVED and STRIDED clips on the GPU under the process's
HIPSOXR_* environment — the debug-switch build with HIPSOXR_DEBUG_LAUNCH_LOG — and writes what it ran and what came out to an
.npz:

    python tests/_ragged_strided_probe.py JOBS.json RESULTS.npz

Jobs by "kind":
  "fft"       an exact-bank plan, the frequency-domain engine BY NAME: {"name", "case", "dtype": "f32" | "f64" | "i16", "ch",
              "kernel", "seed", "layout": "packed" ([frames, ch] interleaved) | "col2" (ch == 1: each clip column 0 of a 2-wide
              buffer, frame stride 2), "dither", "dither_seed", "data": "normal" | "square", "counter"}.  Nine clips in units
              of the job's own hop_out H (read from a pilot launch's log line, and made again where the job's own line shows
              another): out frames H+1, 0, 19H+5 (the longest, 20 blocks), 1, 3H+3 truncated by 7 below out_len, H-1, 2H+1, H, 2H.
              An int16 job also runs the float32 KERNEL_FFT job of the same table (`yf_`), whose values the test quantises.
  "anchor"    five equal-length clips at a constant distance, as a table and as one equal-length batch job with that clip
              stride: `y_` and `yeq_`, `log_` and `logeq_`.
  "refusal"   an int16 stereo table whose second clip's input offset is odd: `err_` the error text, `y_` the untouched output.
  "twostage"  an interpolated-phase plan under KERNEL_AUTO, interleaved channels: the nine clips of
              tests/_ragged_two_stage_probe.py (admitted and short ones mixed, in units of the polyphase tile).
  "py_ragged" dist.resample_ragged(plan, stereo clips); "py_batch" dist.resample_batch on a stereo float32 host corpus by name.
Every output buffer is pre-filled with a sentinel, with ONE spare frame behind every clip, and returned as it lay in memory.
Per table job: `table_`, `geom_` = (H or U, m, in frame stride, in channel stride, out frame stride, out channel stride),
`x_`, `y_`, `log_`, `count_` (device counter or -1).  Nothing is compared here."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ragged_exact_probe import DTYPE, SENTINEL, Log, fields, in_frames_for, make_data, run_table  # noqa: E402
from _ragged_two_stage_probe import clip_lengths  # noqa: E402
import torch  # noqa: E402
from soxr_amd import _native, device as dev, dist  # noqa: E402

FFT = _native.KERNEL_FFT


def hop_of(lines, what):
    got = [int(fields(ln)["hop_out"]) for ln in lines.split("\n") if ln.startswith("form=strided2")]
    assert got, "%s: no strided launch in %r" % (what, lines)
    return got[0]


def lay_out(layout, ch, n_in, n_out, odd_clip=None):
    """-> (in strides, out strides, in offsets, out offsets, in elements, out elements): clips end to end, one spare frame
    behind every output clip"""
    w = 2 if layout == "col2" else ch
    in_fr = np.concatenate([[0], np.cumsum(n_in)[:-1]]).astype(np.int64)
    out_fr = np.concatenate([[0], np.cumsum(np.array(n_out) + 1)[:-1]]).astype(np.int64)
    in_off, out_off = w * in_fr, w * out_fr
    in_len = w * max(int(sum(n_in)), 1) + 2
    if odd_clip is not None:
        in_off[odd_clip:] += 1
    return (w, 1), (w, 1), in_off, out_off, in_len, w * (int(sum(n_out)) + len(n_out))


def fill(x, data, in_off, n_in, ch, in_s):
    for d, off, n in zip(data, in_off, n_in):
        torch.as_strided(x, (n, ch), in_s, int(off)).copy_(d)


def fft_lengths(plan, h):
    want = [h + 1, 0, 19 * h + 5, 1, 3 * h + 3, h - 1, 2 * h + 1, h, 2 * h]
    cut = [0, 0, 0, 0, 7, 0, 0, 0, 0]
    n_in = [in_frames_for(plan, w) for w in want]
    n_out = [w - c for w, c in zip(want, cut)]
    assert all(o <= plan.out_len(i) for i, o in zip(n_in, n_out))
    return n_in, n_out


def fft_job(job, plans, pilots, log, out):
    name, case, ch, dtype, kernel = job["name"], tuple(job["case"]), int(job["ch"]), DTYPE[job["dtype"]], int(job["kernel"])
    plan = plans.setdefault(case, dev.Plan(*case))
    layout, sent = job.get("layout", "packed"), SENTINEL[job["dtype"]]
    key = (case, job["dtype"], ch, kernel, layout)
    if key not in pilots:  # one clip of 60 000 frames: a first H
        in_s, out_s, in_off, out_off, in_len, out_len = lay_out(layout, ch, [60000], [plan.out_len(60000)])
        x = torch.zeros(in_len, dtype=dtype, device="cuda")
        y = torch.zeros(out_len, dtype=dtype, device="cuda")
        log.tail()
        run_table(plan, x.data_ptr(), y.data_ptr(), dtype, ch, [[0, 60000, 0, plan.out_len(60000)]], in_s, out_s, kernel)
        torch.cuda.synchronize()
        pilots[key] = hop_of(log.tail().strip(), name)
    h = pilots[key]
    for attempt in range(4):
        n_in, n_out = fft_lengths(plan, h)
        rng = np.random.default_rng(int(job["seed"]))
        data = [make_data(job.get("data", "normal"), rng, n, ch, dtype) for n in n_in]
        in_s, out_s, in_off, out_off, in_len, out_len = lay_out(layout, ch, n_in, n_out)
        x = torch.full((in_len,), sent, dtype=dtype)
        fill(x, data, in_off, n_in, ch, in_s)
        x = x.cuda()
        y = torch.full((out_len,), sent, dtype=dtype, device="cuda")
        table = np.ascontiguousarray(np.stack([in_off, n_in, out_off, n_out], axis=1), dtype=np.int64)
        counter = torch.zeros(1, dtype=torch.int64, device="cuda") if job.get("counter") else None
        torch.cuda.synchronize()
        log.tail()
        run_table(plan, x.data_ptr(), y.data_ptr(), dtype, ch, table, in_s, out_s, kernel, dither=job.get("dither", False),
                  seed=job.get("dither_seed", 0), counter=counter.data_ptr() if counter is not None else None)
        torch.cuda.synchronize()
        lines = log.tail().strip()
        got = hop_of(lines, name)
        if got == h:
            break
        assert attempt < 3, "the launcher's block size did not settle: %r" % lines
        h = got
    out["table_" + name] = table
    out["geom_" + name] = np.array([h, 0, in_s[0], in_s[1], out_s[0], out_s[1]], np.int64)
    out["x_" + name], out["y_" + name], out["log_" + name] = x.cpu().numpy(), y.cpu().numpy(), np.array(lines)
    out["count_" + name] = np.array([int(counter.item()) if counter is not None else -1], np.int64)
    if dtype == torch.int16:  # the float32 job of the same table, by name: what the int16 job's output stage is fed
        xf = x.float()
        yf = torch.full((out_len,), SENTINEL["f32"], dtype=torch.float32, device="cuda")
        run_table(plan, xf.data_ptr(), yf.data_ptr(), torch.float32, ch, table, in_s, out_s, FFT)
        torch.cuda.synchronize()
        out["yf_" + name], out["logf_" + name] = yf.cpu().numpy(), np.array(log.tail().strip())


def anchor_job(job, plans, log, out):
    """the same five clips as a table and as an equal-length batch at the table's constant distance"""
    name, case, ch, dtype = job["name"], tuple(job["case"]), int(job["ch"]), DTYPE[job["dtype"]]
    plan = plans.setdefault(case, dev.Plan(*case))
    n_in, n_clips = int(job["frames"]), 5
    n_out = plan.out_len(n_in)
    d_in, d_out = ch * (n_in + 3), ch * (n_out + 1)
    rng = np.random.default_rng(int(job["seed"]))
    x = torch.full((n_clips * d_in,), SENTINEL[job["dtype"]], dtype=dtype)
    for c in range(n_clips):
        torch.as_strided(x, (n_in, ch), (ch, 1), c * d_in).copy_(make_data("normal", rng, n_in, ch, dtype))
    x = x.cuda()
    y = torch.full((n_clips * d_out,), SENTINEL[job["dtype"]], dtype=dtype, device="cuda")
    yeq = y.clone()
    table = np.array([[c * d_in, n_in, c * d_out, n_out] for c in range(n_clips)], np.int64)
    torch.cuda.synchronize()
    log.tail()
    run_table(plan, x.data_ptr(), y.data_ptr(), dtype, ch, table, (ch, 1), (ch, 1), FFT)
    torch.cuda.synchronize()
    out["log_" + name] = np.array(log.tail().strip())
    plan.run(x.data_ptr(), yeq.data_ptr(), dev._torch_elem(dtype), n_clips, ch, n_in, n_out, (d_in, ch, 1), (d_out, ch, 1),
             stream=torch.cuda.current_stream().cuda_stream, kernel=FFT)
    torch.cuda.synchronize()
    out["logeq_" + name] = np.array(log.tail().strip())
    out["table_" + name], out["x_" + name], out["y_" + name], out["yeq_" + name] = table, x.cpu().numpy(), y.cpu().numpy(), yeq.cpu().numpy()


def refusal_job(job, plans, log, out):
    name, case = job["name"], tuple(job["case"])
    plan = plans.setdefault(case, dev.Plan(*case))
    n_in = [9000, 7001, 5000]
    n_out = [plan.out_len(n) for n in n_in]
    in_s, out_s, in_off, out_off, in_len, out_len = lay_out("packed", 2, n_in, n_out, odd_clip=1)
    x = torch.zeros(in_len, dtype=torch.int16, device="cuda")
    y = torch.full((out_len,), SENTINEL["i16"], dtype=torch.int16, device="cuda")
    table = np.ascontiguousarray(np.stack([in_off, n_in, out_off, n_out], axis=1), dtype=np.int64)
    assert table[1, 0] % 2 == 1
    torch.cuda.synchronize()
    log.tail()
    err = ""
    try:
        run_table(plan, x.data_ptr(), y.data_ptr(), torch.int16, 2, table, in_s, out_s, _native.KERNEL_FFT_PCM, dither=True, seed=3)
    except RuntimeError as e:
        err = str(e)
    torch.cuda.synchronize()
    out["err_" + name], out["y_" + name], out["log_" + name] = np.array(err), y.cpu().numpy(), np.array(log.tail().strip())


def twostage_job(job, plans, log, out):
    name, case, ch, dtype = job["name"], tuple(job["case"]), int(job["ch"]), DTYPE[job["dtype"]]
    plan = plans.setdefault(case, dev.Plan(*case))
    assert plan.phases != 0, "an interpolated-phase plan"
    sent, u = SENTINEL[job["dtype"]], 512
    for attempt in range(6):
        m, lens = clip_lengths(plan, u)
        n_in, n_out = [a for a, _ in lens], [b for _, b in lens]
        rng = np.random.default_rng(int(job["seed"]))
        data = [make_data("normal", rng, n, ch, dtype) for n in n_in]
        in_s, out_s, in_off, out_off, in_len, out_len = lay_out("packed", ch, n_in, n_out)
        x = torch.full((in_len,), sent, dtype=dtype)
        fill(x, data, in_off, n_in, ch, in_s)
        x = x.cuda()
        y = torch.full((out_len,), sent, dtype=dtype, device="cuda")
        table = np.ascontiguousarray(np.stack([in_off, n_in, out_off, n_out], axis=1), dtype=np.int64)
        torch.cuda.synchronize()
        log.tail()
        run_table(plan, x.data_ptr(), y.data_ptr(), dtype, ch, table, in_s, out_s, _native.KERNEL_AUTO)
        torch.cuda.synchronize()
        lines = log.tail().strip()
        got = [int(fields(ln)["R"]) for ln in lines.split("\n") if ln.startswith("kernel=poly")]
        if not got or 256 * got[0] == u:
            break
        assert attempt < 5, "the launcher's R did not settle: %r" % lines
        u = 256 * got[0]
    out["table_" + name] = table
    out["geom_" + name] = np.array([u, m, in_s[0], in_s[1], out_s[0], out_s[1]], np.int64)
    out["x_" + name], out["y_" + name], out["log_" + name] = x.cpu().numpy(), y.cpu().numpy(), np.array(lines)
    short = [dev.resample_tensor(plan, d.cuda(), kernel=_native.KERNEL_EXACT)[:o].reshape(o, ch).cpu().numpy()
             for d, n, o in zip(data, n_in, n_out) if o > 0 and min(n, o) < 8192]
    out["short_" + name] = np.concatenate([s.reshape(-1) for s in short])
    torch.cuda.synchronize()


def py_ragged(job, plans, log, out):
    """dist.resample_ragged(plan, stereo clips) under defaults"""
    case, name = tuple(job["case"]), job["name"]
    plan = plans.setdefault(case, dev.Plan(*case))
    rng = np.random.default_rng(int(job["seed"]))
    clips = [torch.from_numpy((rng.standard_normal((n, 2)) * 0.25).astype(np.float32)).cuda() for n in job["lengths"]]
    torch.cuda.synchronize()
    log.tail()
    ys = dist.resample_ragged(plan, clips)
    torch.cuda.synchronize()
    out["log_" + name] = np.array(log.tail().strip())
    out["x_" + name] = torch.cat([c.reshape(-1) for c in clips]).cpu().numpy()
    out["y_" + name] = torch.cat([y.reshape(-1) for y in ys]).cpu().numpy()
    out["nout_" + name] = np.array([int(y.shape[0]) for y in ys], np.int64)
    solo = [dev.resample_tensor(plan, c, kernel=_native.KERNEL_EXACT) if c.shape[0] else c[:0] for c in clips]
    out["exact_" + name] = torch.cat([y.reshape(-1) for y in solo]).cpu().numpy()


def py_batch(job, plans, log, out):
    """dist.resample_batch on a stereo float32 host corpus with kernel=KERNEL_FFT (several blocks of the staging ring)"""
    in_rate, out_rate, quality = job["case"]
    rng = np.random.default_rng(int(job["seed"]))
    clips = [(rng.standard_normal((n, 2)) * 0.25).astype(np.float32) for n in job["lengths"]]
    n_in = [int(c.shape[0]) for c in clips]
    blocks = dist._PipeRun(n_in, n_in, 2, 4, int(job["block_bytes"]), 3).blocks
    log.tail()
    res = dist.resample_batch(clips, in_rate, out_rate, quality, devices=[0], kernel=FFT, block_bytes=int(job["block_bytes"]))
    torch.cuda.synchronize()
    out["log_" + job["name"]] = np.array(log.tail().strip())
    out["blocks_" + job["name"]] = np.array([len(b) for b in blocks], np.int64)
    out["x_" + job["name"]] = np.concatenate([c.reshape(-1) for c in clips])
    out["y_" + job["name"]] = np.concatenate([np.asarray(r).reshape(-1) for r in res])
    out["nout_" + job["name"]] = np.array([int(np.asarray(r).shape[0]) for r in res], np.int64)


def main():
    with open(sys.argv[1]) as f:
        jobs = json.load(f)
    log = Log(os.environ["HIPSOXR_DEBUG_LAUNCH_LOG"])
    plans, pilots, out = {}, {}, {}
    for job in jobs:
        kind = job["kind"]
        if kind == "fft":
            fft_job(job, plans, pilots, log, out)
        elif kind == "anchor":
            anchor_job(job, plans, log, out)
        elif kind == "refusal":
            refusal_job(job, plans, log, out)
        elif kind == "twostage":
            twostage_job(job, plans, log, out)
        elif kind == "py_ragged":
            py_ragged(job, plans, log, out)
        elif kind == "py_batch":
            py_batch(job, plans, log, out)
        else:
            raise ValueError(kind)
    np.savez(sys.argv[2], **out)
    print("RAGGED_STRIDED_PROBE done: %d jobs" % len(jobs))


if __name__ == "__main__":
    main()
