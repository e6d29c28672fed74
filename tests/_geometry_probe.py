"""Helper of tests/test_gpu_fft_geometry.py: float32 unit-stride jobs of the frequency-domain engine at 48k <-> 44.1k —
the jobs whose block size the one-round rule chooses (csrc/fft.hip, kOneRoundCost) — under the process's HIPSOXR_*
environment (HIPSOXR_DEBUG_FFT_K with the debug-switch build: every such job on blocks of k periods; k < 0: the rule off).
Prints one JSON line: relative RMS errors against the oracle's float64 direct form on its own bank (mode "ref"),
determinism flags, and digests of jobs whose path must not depend on the rule."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "python-soxr_amd"))
import torch  # noqa: E402
from soxr_amd import device as dev  # noqa: E402
from soxr_amd import dist as sdist  # noqa: E402
from oracle import oracle as o  # noqa: E402

FFT, FFT_PCM = dev._n.KERNEL_FFT, dev._n.KERNEL_FFT_PCM


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2))) if a.shape == b.shape and a.size else 9.0


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def in_len_for(plan, n_out, guess):
    """An input length whose output length is n_out (out_len is monotone in the input length)."""
    n = guess
    while plan.out_len(n) < n_out:
        n += 1
    while plan.out_len(n) > n_out:
        n -= 1
    assert plan.out_len(n) == n_out
    return n


rng = np.random.default_rng(1420)
out = {}
for name, (fi, fo, L, M) in {"down": (48000, 44100, 147, 160), "up": (44100, 48000, 160, 147)}.items():
    plan = dev.Plan(fi, fo, "VHQ")
    # a block of k periods keeps k - 2 of them: the kept run of a PAIR of blocks is 2 (k - 2) L outputs.  Lengths that end
    # one output before / on / one output behind the end of the first and of the second pair's run, and on the last
    # element of the following run's first 16-byte granule (4 floats) — for both new block sizes, whatever k is forced
    for k in (14, 20):
        run = 2 * (k - 2) * L
        for pairs in (1, 2):
            for d in (-1, 0, 1, 4):
                n_out = pairs * run + d
                n = in_len_for(plan, n_out, n_out * M // L)
                x = (rng.standard_normal(n) * 0.25).astype(np.float32)
                y = dev.resample_tensor(plan, torch.from_numpy(x).cuda(), kernel=FFT).cpu().numpy()
                out[f"{name}_k{k}_pairs{pairs}_{d:+d}"] = rel(y, o.resample(x, fi, fo, "VHQ", mode="ref"))
    # the 60 s clip (AUTO, as the benchmark runs it), twice
    x = (rng.standard_normal(fi * 60) * 0.25).astype(np.float32)
    xt = torch.from_numpy(x).cuda()
    y1 = dev.resample_tensor(plan, xt).cpu().numpy()
    y2 = dev.resample_tensor(plan, xt).cpu().numpy()
    out[f"{name}_clip60"] = rel(y1, o.resample(x, fi, fo, "VHQ", mode="ref"))
    out[f"{name}_clip60_deterministic"] = bool(np.array_equal(y1, y2))
    out[f"{name}_clip60_sha"] = sha(y1)
    # two planar columns (frame stride 1, channel stride = the column's length), 25 s
    xp = (rng.standard_normal((2, fi * 25)) * 0.25).astype(np.float32)
    xpt = torch.from_numpy(xp).cuda().T                                     # [frame, channel]
    yp = torch.empty((2, plan.out_len(fi * 25)), device="cuda").T
    dev.resample_tensor(plan, xpt, out=yp)
    yp1 = yp.cpu().numpy()
    out[f"{name}_planar2"] = max(rel(yp1[:, c], o.resample(xp[c], fi, fo, "VHQ", mode="ref")) for c in range(2))
    dev.resample_tensor(plan, xpt, out=yp)
    out[f"{name}_planar2_deterministic"] = bool(np.array_equal(yp1, yp.cpu().numpy()))
    # a ragged batch through the clip table: lengths from nothing to many pairs, every clip where it lies
    lens = [0, 1, 5, 3000, 24 * M + 7, 52345, 300007, 77777]
    clips = [torch.from_numpy((rng.standard_normal(n) * 0.25).astype(np.float32)).cuda() for n in lens]
    job = sdist.RaggedJob(plan, clips, kernel=FFT)
    job.y.fill_(7.0)                                                        # anything not written would show
    job.launch()
    torch.cuda.synchronize()
    outs = [t.cpu().numpy().reshape(-1) for t in job.outputs()]
    out[f"{name}_ragged"] = max([rel(outs[i], o.resample(clips[i].cpu().numpy(), fi, fo, "VHQ", mode="ref")) for i in range(len(lens)) if lens[i]] +
                                [0.0 if outs[0].size == 0 else 9.0])
    job.launch()
    torch.cuda.synchronize()
    out[f"{name}_ragged_deterministic"] = all(np.array_equal(a, t.cpu().numpy().reshape(-1)) for a, t in zip(outs, job.outputs()))
    # ---- jobs whose path the rule must not move: digests, compared across environments by the test ----
    g = torch.Generator(device="cpu").manual_seed(99)
    xb = (torch.randn((128, fi * 10, 1), generator=g) * 0.25).cuda()       # the 128 x 10 s batch shape
    out[f"{name}_batch128_sha"] = sha(dev.resample_tensor(plan, xb).cpu().numpy())
    del xb
    x64 = torch.from_numpy(rng.standard_normal(fi * 20) * 0.25).cuda()      # float64, one clip of 20 s
    out[f"{name}_f64_sha"] = sha(dev.resample_tensor(plan, x64).cpu().numpy())
    xi = torch.from_numpy((rng.standard_normal(fi * 20) * 6000).astype(np.int16)).cuda()
    out[f"{name}_i16_pcm_sha"] = sha(dev.resample_tensor(plan, xi, kernel=FFT_PCM, dither=True, dither_seed=3).cpu().numpy())
print("GEOMETRY_PROBE " + json.dumps(out))
