#!/usr/bin/env python
"""Randomised check of device streams on the frequency-domain engine (TensorStream(engine="fft")): random rate pair from
the paired-kernel schedule table, HQ / VHQ, dtype, channel count and chunk plan (0 .. 200 000 frames per call).  Per case:
every call returns the default stream's frame count and delay; float streams meet the engine's bar against the oracle's
float64 direct form globally and around every chunk seam; integer streams equal the float stream of their width pushed
through oracle.quantize, sample for sample, clip count included (tests/stream_fft_checks.py).
`python tests/fuzz/fuzz_stream_fft.py [cases] [seed]`"""
import os, random, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "python-soxr_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch
from soxr_amd import device as dev
from oracle import oracle
import stream_fft_checks as sc

n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 24
r = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
torch.zeros(1, device="cuda").cpu()
fails = 0
for case in range(n_cases):
    in_rate, out_rate = r.choice(sc.TABLE_RATES)
    q = r.choice(["VHQ", "HQ"])
    dtype = r.choice([np.float32, np.float32, np.float64, np.int16, np.int16, np.int32])
    ch = 1 if dtype == np.int32 else r.choice([1, 2, 4, 8]) if dtype == np.int16 else r.choice([1, 1, 2, 3, 5, 8])
    total = r.randint(1, 400000)
    sizes = sc.random_plan(r, total)
    for _ in range(r.randint(0, 2)):
        sizes.insert(r.randint(0, len(sizes)), 0)
    rng = np.random.default_rng(case)
    what = f"case {case}: {in_rate}->{out_rate} {q} {np.dtype(dtype).name} ch={ch} total={total} chunks={len(sizes)}"
    try:
        tdt = sc.torch_dtype(dtype)
        x = sc.signal(rng, total, ch, dtype, full_scale=(dtype == np.int16 and r.random() < 0.3))
        ts = dev.TensorStream(in_rate, out_rate, ch, dtype=tdt, quality=q, dither_seed=case, engine="fft")
        tw = dev.TensorStream(in_rate, out_rate, ch, dtype=tdt, quality=q, dither_seed=case)
        outs = sc.feed(ts, x, sizes, twin=tw)
        assert sum(len(o) for o in outs) == dev.Plan(in_rate, out_rate, q).out_len(total)
        if np.issubdtype(dtype, np.integer):
            sc.check_integer_identity(oracle, dev, in_rate, out_rate, q, x, sizes, r.random() < 0.7, case, what)
        elif total > 2000:  # (a reference of a few samples has no RMS to speak of)
            ref = oracle.resample(x.astype(np.float64), in_rate, out_rate, q, mode="ref")
            sc.check_values(outs, ref, dev.Plan(in_rate, out_rate, q).taps, sc.tolerance(dtype, q), what)
    except (AssertionError, RuntimeError) as e:
        fails += 1
        print(f"FAIL {what} sizes={sizes[:12]}: {e!r}"[:1500])
print(f"stream-fft fuzz: {fails} failures in {n_cases} cases")
sys.exit(1 if fails else 0)
