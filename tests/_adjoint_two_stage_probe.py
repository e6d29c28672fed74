"""Child process of tests/test_gpu_adjoint_two_stage.py, on the debug-switch build with a launch log: one adjoint job of
HIPSOXR_KERNEL_ADJOINT_TWO_STAGE per (tap count of k_poly_adj, element width) that HQ / VHQ plans reach, at the smallest
admitted size, with the float64 exact adjoint of the same cotangent — and the launch log's lines of each job.

    python _adjoint_two_stage_probe.py OUT.npz        (HIPSOXR_LIBRARY, HIPSOXR_DEBUG_LAUNCH_LOG set by the parent)

Also imported by the test for the case lists and the arithmetic that says which instance a plan takes."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

TAPS = (8, 12, 16, 20, 24, 28, 32, 40, 48, 56)  # twostage.hip HIPSOXR_POLY_TAPS
MIN_FRAMES = 8192                               # poly_rules.h two_stage_admits
# the issue's rate pairs (VHQ; HQ on the first two) ...
PAIRS = [(48000, 44101, "VHQ"), (44101, 48000, "VHQ"), (44100, 16001, "VHQ"), (96000, 24001, "VHQ"), (8000, 44100.25, "VHQ"),
         (48000, 44101, "HQ"), (44101, 48000, "HQ")]
# ... two of which take 40 and 56 taps.  56 taps: poly_design gives the plan no two-stage form at all (its [128][57] table of
# 16-byte records is above the 100 KB it allows), AUTO == EXACT in both widths — replaced by the steepest 96000 -> pair of 48
# taps.  40 taps and more: the float64 table ([128][T2 + 1] records of 32 bytes: 168 KB and up) leaves LDS, the forward form
# does not take them in float64 — replaced in float64 by pairs of at most 32 taps.  Replaced, not skipped.
REPLACED = {"f32": {(96000, 24001, "VHQ"): (96000, 25401, "VHQ")},
            "f64": {(44100, 16001, "VHQ"): (44100, 19001, "VHQ"), (96000, 24001, "VHQ"): (44100, 22051, "VHQ")}}
F64_MAX_TAPS = 32
# every instance HQ / VHQ reach, once per width: the tap count by poly_design's arithmetic (poly_taps below)
COVER = {12: (48000, 44101, "HQ"), 16: (48000, 44101, "VHQ"), 20: (44101, 48000, "HQ"), 24: (44100, 19001, "HQ"), 28: (44101, 48000, "VHQ"),
         32: (44100, 19001, "VHQ"), 40: (44100, 16001, "VHQ"), 48: (96000, 25401, "VHQ")}
# 8 taps: down needs (att + 6 - 7.95) / (14.357 out/in) + 1 <= 8 with out/in < 1 — att <= 102 dB, below HQ's 128; up is fixed at
# 19 (HQ) / 26 (VHQ) taps.  No HQ / VHQ plan takes the 8-tap instance.
# 56 taps: the design lands there (VHQ, steeper than 3.79:1) but poly_design then refuses the table: the plan has no form.
UNREACHABLE = (8, 56)


def case_for(case, kind):
    return REPLACED[kind].get(case, case)


def poly_taps(plan):
    """twostage.hip poly_design: Kaiser's estimate for att + 6 dB over the stage's transition band, rounded up to an instance"""
    up = plan.out_rate > plan.in_rate
    width = 0.5 if up else plan.out_rate / plan.in_rate
    n = (plan.att_db + 6.0 - 7.95) / (2.285 * 2.0 * math.pi * width) + 1.0
    return next(t for t in TAPS if t >= math.ceil(n))


def smallest(plan):
    """the smallest n_x with both sides of the job at MIN_FRAMES or more"""
    n = MIN_FRAMES
    while plan.out_len(n) < MIN_FRAMES:
        n += max(1, int((MIN_FRAMES - plan.out_len(n)) * plan.in_rate / plan.out_rate))
    while n > MIN_FRAMES and plan.out_len(n - 1) >= MIN_FRAMES:
        n -= 1
    return n


def fields(line):
    return dict(tok.split("=", 1) for tok in line.split() if "=" in tok)


def main(out_path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "python-soxr_amd")]
    import torch
    from soxr_amd import device as dev
    log_path = os.environ["HIPSOXR_DEBUG_LAUNCH_LOG"]
    out = {}
    gen = torch.Generator(device="cuda").manual_seed(7)
    for taps, case in sorted(COVER.items()):
        plan = dev.Plan(*case)
        assert plan.phases and poly_taps(plan) == taps, (case, taps)
        n_x = smallest(plan)
        for kind, dt in (("f32", torch.float32), ("f64", torch.float64)):
            if kind == "f64" and taps > F64_MAX_TAPS:
                continue
            gy = torch.randn(plan.out_len(n_x), dtype=dt, device="cuda", generator=gen)
            ref = dev.resample_tensor_adjoint(plan, gy.double(), n_x, kernel=dev.KERNEL_ADJOINT)
            torch.cuda.synchronize()
            open(log_path, "w").close()
            got = dev.resample_tensor_adjoint(plan, gy, n_x, kernel=dev.KERNEL_ADJOINT_TWO_STAGE)
            torch.cuda.synchronize()
            with open(log_path) as f:
                out["log_%d_%s" % (taps, kind)] = f.read()
            out["got_%d_%s" % (taps, kind)] = got.cpu().numpy()
            out["ref_%d_%s" % (taps, kind)] = ref.cpu().numpy()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
