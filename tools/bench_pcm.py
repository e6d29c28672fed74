#!/usr/bin/env python3
"""Integer device jobs, exact engine against the frequency-domain engine (HIPSOXR_KERNEL_FFT_PCM), launch time.

    python tools/bench_pcm.py --out pcm.json [--base-tree DIR] [--rounds 3]

Shapes: the 60 s mono clip and the 128 x 10 s batch, 48 kHz -> 44.1 kHz VHQ.  Legs: int16 / int32 KERNEL_EXACT, float32
KERNEL_FFT (the same transform on twice the bytes), int16 / int32 KERNEL_FFT_PCM where the build has it.
--base-tree: a built checkout of ANOTHER commit (its python-soxr_amd/ is imported instead of this one's) — the baseline
the new selector is held against is the exact engine of the commit before it.  The two trees are measured alternately,
`--rounds` times each, every measurement in a fresh child process under its own time limit; the first failing child
ends the run.  A leg's figure is the median over HIP-event windows (every window the same launches, buffer sets rotated
so that no launch finds its input in a cache, all shapes warmed up first), as bench.py's kernel legs; the spread
reported is that of the per-round medians.  One JSON record per (tree, round, leg) line in --out, a table on stdout."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN_RATE, OUT_RATE, QUALITY = 48000, 44100, "VHQ"
SHAPES = {"mono_60s": (1, 60 * IN_RATE, 1), "batch_128x10s": (128, 10 * IN_RATE, 1)}
HBM_BYTES_PER_S = 8e12


def worker(tree, windows, out_path, tag, rnd):
    sys.path.insert(0, os.path.join(tree, "python-soxr_amd"))
    import torch
    torch.cuda.init()
    torch.zeros(1, device="cuda").cpu()          # torch's HIP context first (see tests/conftest.py)
    from soxr_amd import _native, device as dev
    plan = dev.Plan(IN_RATE, OUT_RATE, QUALITY)
    pcm = getattr(_native, "KERNEL_FFT_PCM", None)
    legs = [("int16_exact", torch.int16, _native.KERNEL_EXACT), ("int32_exact", torch.int32, _native.KERNEL_EXACT),
            ("float32_fft", torch.float32, _native.KERNEL_FFT)]
    if pcm is not None:
        legs += [("int16_fft_pcm", torch.int16, pcm), ("int32_fft_pcm", torch.int32, pcm)]
    torch.manual_seed(0)
    prepared = []
    for sname, shape in SHAPES.items():
        clips, frames, ch = shape
        n_out = plan.out_len(frames)
        for lname, dtype, kernel in legs:
            es = torch.empty(0, dtype=dtype).element_size()
            sets = max(2, min(8, int(1.2e9 // (clips * frames * es * 2))))   # > the 256 MB last-level cache in flight
            jobs = []
            for _ in range(sets):
                v = torch.randn(shape, device="cuda")
                x = (v * 0.25 if dtype == torch.float32 else torch.round(v * (5000 if dtype == torch.int16 else 2.0 ** 27))).to(dtype)
                y = torch.empty((clips, n_out, ch), dtype=dtype, device="cuda")
                jobs.append(dev.PreparedJob(plan, x, y, kernel=kernel))
            win = 40 if clips == 1 else 10
            prepared.append((sname, lname, jobs, win, clips * ch * (frames + n_out) * es, clips * ch * n_out))
    for _, _, jobs, win, _, _ in prepared:           # warm-up of every shape and leg before any timing
        for i in range(2 * len(jobs)):
            jobs[i % len(jobs)].launch()
    torch.cuda.synchronize()
    with open(out_path, "a") as f:
        for sname, lname, jobs, win, nbytes, nout in prepared:
            per = []
            for w in range(windows):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(win):
                    jobs[(w * win + i) % len(jobs)].launch()
                e1.record()
                e1.synchronize()
                per.append(e0.elapsed_time(e1) * 1e3 / win)
            per.sort()
            rec = {"tree": tag, "round": rnd, "shape": sname, "leg": lname, "us": per[len(per) // 2], "us_min": per[0],
                   "us_p90": per[int(0.9 * (len(per) - 1))], "windows": windows, "launches_per_window": win,
                   "algorithmic_bytes": nbytes, "bytes_per_output": nbytes / nout, "version": _native.version()}
            f.write(json.dumps(rec) + "\n")
            f.flush()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True)
    ap.add_argument("--base-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--windows", type=int, default=30)
    ap.add_argument("--child-timeout", type=int, default=150)
    ap.add_argument("--worker", nargs=3, metavar=("TREE", "TAG", "ROUND"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.worker[0], a.windows, a.out, a.worker[1], int(a.worker[2]))
        return 0
    open(a.out, "w").close()
    trees = ([("base", os.path.abspath(a.base_tree))] if a.base_tree else []) + [("this", ROOT)]
    for rnd in range(a.rounds):
        for tag, tree in trees:
            cmd = [sys.executable, os.path.abspath(__file__), "--out", a.out, "--windows", str(a.windows), "--worker", tree, tag, str(rnd)]
            try:
                rc = subprocess.run(cmd, timeout=a.child_timeout).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:     # nothing more is started on the GPU after a failure
                print(f"child ({tag}, round {rnd}) ended with status {rc}: stopping", file=sys.stderr)
                return 1
    recs = [json.loads(l) for l in open(a.out)]
    print(f"{'shape':14s} {'tree':5s} {'leg':14s} {'median us':>10s} {'rounds (us)':>28s} {'spread':>7s} {'B/out':>6s} {'of 8 TB/s':>9s}")
    for key in sorted({(r["shape"], r["tree"], r["leg"]) for r in recs}):
        v = sorted(r["us"] for r in recs if (r["shape"], r["tree"], r["leg"]) == key)
        r0 = next(r for r in recs if (r["shape"], r["tree"], r["leg"]) == key)
        med = v[len(v) // 2]
        print(f"{key[0]:14s} {key[1]:5s} {key[2]:14s} {med:10.2f} {' '.join('%.2f' % x for x in v):>28s} {100 * (v[-1] - v[0]) / med:6.1f}% "
              f"{r0['bytes_per_output']:6.3f} {100 * r0['algorithmic_bytes'] / (med * 1e-6) / HBM_BYTES_PER_S:8.1f}%")
    return 0


if __name__ == "__main__":
    sys.exit(main())
