"""Helper of tests/test_gpu_tile_forms.py: runs the exact-engine jobs of a JSON file (written by the test) on the GPU under the
process's HIPSOXR_* environment — the debug-switch build with HIPSOXR_DEBUG_LAUNCH_LOG, and whatever form switches the test
sets for this child — and writes the results to an .npz:

    python tests/_tile_forms_probe.py JOBS.json RESULTS.npz

A job is {"name", "case": [in_rate, out_rate, quality], "dtype", "frames", "ch", "seed", "kernel", "dither", "dither_seed", "k0",
"windows": [[first, count], ...]}.  Its input is make_input(dtype, frames, ch, seed) — the test makes the same array for the
oracle — as one clip [frames, channels]; k0 != 0 runs the window of outputs [k0, out_len) through Plan.run.  Per job: the
SHA-256 of the whole result's bytes (`h_<name>`), its shape (`shape_<name>`), the windows of it one after the other
(`w_<name>`: [sum of counts, channels]) and the launch log's lines of the job (`log_<name>`).  Nothing is compared here."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_input(dtype, frames, ch, seed):
    """white noise of RMS 0.25 (of full scale / 1.6 for int16, / 2 for int32), [frames, ch]"""
    x = np.random.default_rng(seed).standard_normal((frames, ch)) * 0.25
    return {"float32": x.astype(np.float32), "float64": x, "int16": (x * 20000).astype(np.int16), "int32": (x * 2 ** 30).astype(np.int32)}[dtype]


def log_tail(path, pos):
    if not os.path.exists(path):
        return "", pos
    with open(path) as f:
        f.seek(pos)
        txt = f.read()
    return txt, pos + len(txt)


def main():
    sys.path.insert(0, os.path.join(ROOT, "python-soxr_amd"))
    import torch
    from soxr_amd import device as dev

    with open(sys.argv[1]) as f:
        jobs = json.load(f)
    log_path, pos = os.environ["HIPSOXR_DEBUG_LAUNCH_LOG"], 0
    plans, out = {}, {}
    for job in jobs:
        name, case = job["name"], tuple(job["case"])
        if case not in plans:
            plans[case] = dev.Plan(*case)
        plan, frames, ch, k0 = plans[case], job["frames"], job["ch"], job["k0"]
        x = torch.from_numpy(make_input(job["dtype"], frames, ch, job["seed"])).cuda()
        _, pos = log_tail(log_path, pos)
        if k0 == 0:
            y = dev.resample_tensor(plan, x, kernel=job["kernel"], dither=job["dither"], dither_seed=job["dither_seed"])
        else:  # outputs [k0, out_len) of the same signal: a window job (b_first != 0 in the tile kernels)
            n = plan.out_len(frames) - k0
            y = torch.empty((n, ch), dtype=x.dtype, device="cuda")
            plan.run(x.data_ptr(), y.data_ptr(), dev._torch_elem(x.dtype), 1, ch, frames, n, (0, ch, 1), (0, ch, 1),
                     stream=torch.cuda.current_stream().cuda_stream, kernel=job["kernel"], out_k0=k0, dither=job["dither"], dither_seed=job["dither_seed"])
        torch.cuda.synchronize()
        lines, pos = log_tail(log_path, pos)
        yh = np.ascontiguousarray(y.cpu().numpy())
        out["h_" + name] = np.array(hashlib.sha256(yh.tobytes()).hexdigest())
        out["shape_" + name] = np.array(yh.shape)
        out["w_" + name] = np.concatenate([yh[a:a + n] for a, n in job["windows"]]) if job["windows"] else yh[:0]
        out["log_" + name] = np.array(lines.strip())
        del x, y
    np.savez(sys.argv[2], **out)
    print("TILE_FORMS_PROBE done: %d jobs" % len(jobs))


if __name__ == "__main__":
    main()
