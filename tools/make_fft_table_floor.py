#!/usr/bin/env python3
"""Writes tests/golden/fft_table_floor.json: for every row of the paired-block table (csrc/fft.hip, fft_pairs) and the
recipes VHQ / HQ, what the float64 overlap-save model (oracle/overlap_save.py, blocks of the row's k periods) leaves
against the oracle's float64 direct form on the inputs of tests/test_gpu_fft_table.py — relative to rms(reference): the
whole-signal RMS error, the largest RMS error of a 2048-sample stretch, the largest pointwise error (CPU only, ~1 min).
The GPU test's per-stretch and pointwise bars of the float64 kernels are four times these figures.

    python tools/make_fft_table_floor.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _table_probe as tp  # noqa: E402
from oracle import oracle as o  # noqa: E402
from oracle import overlap_save as ovs  # noqa: E402

o.lib()
rows, _ = tp.parse_table()
floor = {}
for r in rows:
    floor[tp.row_name(r)] = {}
    for q in tp.QUALITIES:
        f = tp.model_floor(o, ovs, tp.row_key(r), q)
        floor[tp.row_name(r)][q] = f and {k: float("%.4g" % v) for k, v in f.items()}
        print(tp.row_name(r), q, floor[tp.row_name(r)][q], flush=True)
with open(tp.FLOOR_JSON, "w") as f:
    json.dump({"what": "float64 overlap-save model at each row's block size against the oracle's float64 direct form, relative to "
                       "rms(reference): whole-signal RMS, worst 2048-sample stretch RMS, worst sample; null: the row is not "
                       "admissible for the recipe (tools/make_fft_table_floor.py)",
               "floor": floor}, f, indent=1, sort_keys=True)
    f.write("\n")
