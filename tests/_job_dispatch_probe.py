"""Helper of tests/test_gpu_job_dispatch.py and tests/golden/make_job_dispatch_golden.py: runs the jobs of
tests/job_dispatch_cases.py that belong to one environment on the GPU, under the process's HIPSOXR_* environment — the
debug-switch build with HIPSOXR_DEBUG_LAUNCH_LOG — and writes what each was answered:

    python tests/_job_dispatch_probe.py ENV RECORDS.json [RESULTS.npz]

RECORDS.json: {case name: {"error": text} | {"lines": summarize(the job's launch-log lines)}}.  RESULTS.npz (when asked for),
per served case: y_<name> the whole output buffer, ref_<name> the same job on the reference path — KERNEL_EXACT for float32 /
float64 / int16 jobs, the float32 job of the same selector on the widened values rounded once for float16 jobs — and for
the case with "cut": cut_<name>, the job run as the given clip ranges one by one.  Nothing is compared here."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "python-soxr_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from soxr_amd import _native, device as dev  # noqa: E402
from job_dispatch_cases import CASES, EXACT, summarize  # noqa: E402

DTYPE = {"f32": torch.float32, "f64": torch.float64, "i16": torch.int16, "f16": torch.float16}


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


def in_frames_for(plan, n_out):
    if n_out <= 0:
        return 0
    n = max(0, n_out * plan.M // plan.L - 2)
    while plan.out_len(n) < n_out:
        n += 1
    return n


def make_data(rng, shape, dtype):
    v = rng.standard_normal(shape) * 0.25
    if dtype == torch.int16:
        return torch.from_numpy((v * 20000).astype(np.int16))
    return torch.from_numpy(v).to(dtype)


def launch(plan, job):
    err = _native.lib.hipsoxr_run_device(plan.handle, C.byref(job), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (err.decode() if isinstance(err, bytes) else str(err)) if err else None


def plain_job(case, plan, x, y, kernel, clips=None):
    """[clips, frames, channels] contiguous; clips = (first, end): that range alone"""
    n_clips, n_in, ch = x.shape
    n_out = y.shape[1]
    a, b = clips or (0, n_clips)
    j = _native.Job()
    j.in_, j.out = x.data_ptr() + a * n_in * ch * x.element_size(), y.data_ptr() + a * n_out * ch * y.element_size()
    j.elem, j.kernel, j.n_clips, j.n_channels = dev._torch_elem(x.dtype), kernel, b - a, ch
    j.in_clip_stride, j.in_frame_stride, j.in_chan_stride = n_in * ch, ch, 1
    j.out_clip_stride, j.out_frame_stride, j.out_chan_stride = n_out * ch, ch, 1
    j.in_abs0, j.out_k0, j.in_frames, j.out_frames = int(case.get("in_abs0", 0)), int(case.get("out_k0", 0)), n_in, n_out
    j.dither, j.dither_seed = int(bool(case.get("dither"))), 77
    return launch(plan, j)


def table_job(case, plan, x, y, table, kernel):
    ch = int(case["ch"])
    j = _native.Job()
    j.in_, j.out, j.elem, j.kernel = x.data_ptr(), y.data_ptr(), dev._torch_elem(x.dtype), kernel
    j.n_clips, j.n_channels = table.shape[0], ch
    j.in_frame_stride, j.in_chan_stride, j.out_frame_stride, j.out_chan_stride = ch, 1, ch, 1
    j.in_abs0, j.out_k0 = int(case.get("in_abs0", 0)), int(case.get("out_k0", 0))
    j.in_frames, j.out_frames = int(table[:, 1].max()) + int(case.get("job_in", 0)), int(table[:, 3].max()) + int(case.get("job_out", 0))
    j.clip_table, j.clip_table_dev = table.ctypes.data, None
    return launch(plan, j)


def run_case(case, plans, log, records, arrays):
    name, dtype, kernel = case["name"], DTYPE[case["dtype"]], int(case["kernel"])
    plan = plans.setdefault(tuple(case["plan"]), dev.Plan(*case["plan"]))
    rng = np.random.default_rng(len(name) + sum(map(ord, name)))
    is_half = dtype == torch.float16
    if "table" in case:
        ch, n_out = int(case["ch"]), list(case["table"])
        n_in = [in_frames_for(plan, o) for o in n_out]
        in_off = np.concatenate([[0], np.cumsum(n_in)[:-1]]) * ch
        out_off = np.concatenate([[0], np.cumsum(n_out)[:-1]]) * ch
        table = np.ascontiguousarray(np.stack([in_off, n_in, out_off, n_out], axis=1), dtype=np.int64)
        x = make_data(rng, (max(int(sum(n_in)), 1), ch), dtype).cuda()
        if "bad" in case:
            clip, field, value = case["bad"]
            table[clip, field] = plan.out_len(int(table[clip, 1])) + 1 if value == "plan+1" else int(value)
        y = torch.zeros((max(int(sum(n_out)), 1) + 1, ch), dtype=dtype, device="cuda")

        def run(xx, yy, k):
            return table_job(case, plan, xx, yy, table, k)
    else:
        n_clips, n_out, ch = case["shape"]
        n_in = int(case["in_frames"]) if "in_frames" in case else in_frames_for(plan, n_out)
        n_out = n_out or plan.out_len(n_in)
        x = make_data(rng, (n_clips, n_in, 1 if case.get("same_channels") else ch), dtype)
        x = x.expand(n_clips, n_in, ch).contiguous().cuda()
        y = torch.zeros((n_clips, n_out, ch), dtype=dtype, device="cuda")

        def run(xx, yy, k, clips=None):
            return plain_job(case, plan, xx, yy, k, clips)
    torch.cuda.synchronize()
    log.tail()
    err = run(x, y, kernel)
    text = log.tail()
    if err is not None:
        records[name] = {"error": err}
        return
    records[name] = {"lines": summarize(text)}
    if arrays is None:
        return
    arrays["y_" + name] = y.cpu().view(torch.int16).numpy() if is_half else y.cpu().numpy()
    if is_half:  # the identity of tests/test_gpu_half.py: the float32 job of the same selector, rounded once
        yf = torch.zeros(y.shape, dtype=torch.float32, device="cuda")
        assert run(x.float(), yf, kernel) is None
        arrays["ref_" + name] = yf.cpu().to(dtype).view(torch.int16).numpy()
    elif kernel != EXACT:
        ye = torch.zeros_like(y)
        assert run(x, ye, EXACT) is None
        arrays["ref_" + name] = ye.cpu().numpy()
    if "cut" in case:
        yc = torch.zeros_like(y)
        for a, b in case["cut"]:
            assert run(x, yc, kernel, (a, b)) is None
        arrays["cut_" + name] = yc.cpu().numpy()
    log.tail()


def main():
    env, records_path = sys.argv[1], sys.argv[2]
    arrays = {} if len(sys.argv) > 3 else None
    log = Log(os.environ["HIPSOXR_DEBUG_LAUNCH_LOG"])
    plans, records = {}, {}
    for case in CASES:
        if case["env"] == env:
            run_case(case, plans, log, records, arrays)
    with open(records_path, "w") as f:
        json.dump(records, f, indent=1, sort_keys=True)
    if arrays is not None:
        np.savez(sys.argv[3], **arrays)
    print("JOB_DISPATCH_PROBE done: %d jobs under %s" % (len(records), env))


if __name__ == "__main__":
    main()
