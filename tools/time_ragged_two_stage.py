#!/usr/bin/env python3
"""Ragged float batches on interpolated-phase plans under the default selector: what `dist.RaggedJob.launch()` costs for the
tables the two-stage form serves — one ragged polyphase launch, one ragged FFT-stage launch and one ragged launch of the exact
engine for the short clips (per range of columns), where the parent commit's library ran the two-stage form clip by clip inside
the same C call (one allocation, two launches and one free per clip).  The yardstick is the PARENT's library running the very
same calls, not a loop written here: run this tool once per library (HIPSOXR_LIBRARY selects it), each run a process of its own,
alternated, with --json; then merge the records into a table (tools/time_ragged_interp.py is the same tool for the exact engine).

Rows: float32 mono 48000 -> 44101 VHQ (down: polyphase stage first) and 44101 -> 48000 VHQ (up: FFT stage first), 64 and 1024
clips, lengths uniform (seeded) in 1 to 10 s and in 0.1 to 1 s — the latter mixes clips the form admits (8192 frames or more on
both sides) with clips it leaves to the exact engine; one float64 row.  Clips are views of one packed buffer.
Per repetition one `launch()` is timed between two HIP events on the current stream — host-side work between the launches
included — median over the repetitions (min-max in brackets).  The packed result is summed (float64) after the first launch and
after the last: the two sums of one library must be equal (the same job gives the same bits every time); the two LIBRARIES differ
in rounding on admitted mono float32 clips (k_poly here, the split form of k_poly2 there), so their sums are reported side by
side, not compared.  Also reported per row: clips by class and the intermediate's size (all columns; peak = the largest range).
Run on the debug-switch build with HIPSOXR_DEBUG_LAUNCH_LOG set (--shape F: one launch per row, no timing), the tool reads the
ragged polyphase launches' own log lines — grid, R, columns per range — and records two figures of the launch as it was:
the share of its workgroups that leave at the skip test (block index at or behind the column's own tile count), and the imbalance
between columns under the persistent walk (1 - mean / longest tile count: the share of the longest column's time the others' workgroups
have nothing left to do).  GPU only.

    HIPSOXR_LIBRARY=<parent build>/libhipsoxr.so python tools/time_ragged_two_stage.py --json parent1.json
    python tools/time_ragged_two_stage.py --json this1.json          (and once more each: parent2.json, this2.json)
    HIPSOXR_LIBRARY=<debug-switch build> HIPSOXR_DEBUG_LAUNCH_LOG=log python tools/time_ragged_two_stage.py --shape shape.json
    python tools/time_ragged_two_stage.py --merge parent1.json this1.json parent2.json this2.json --with-shape shape.json --out rows.md

--merge pools the repetitions of each library and states the acceptance per row: this tree's median must not exceed the
parent's median by more than the larger of the two min-max spreads."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "python-soxr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

# name, in rate, out rate, quality, dtype, (clip counts), (length ranges in seconds)
RANGES = [(1.0, 10.0), (0.1, 1.0)]
WORKLOADS = [("48000->44101 VHQ float32 mono", 48000, 44101, "VHQ", "float32", (64, 1024), RANGES),
             ("44101->48000 VHQ float32 mono", 44101, 48000, "VHQ", "float32", (64, 1024), RANGES),
             ("48000->44101 VHQ float64 mono", 48000, 44101, "VHQ", "float64", (64,), RANGES[:1])]


def merge(paths, out, shape_path=None):
    shape = None
    if shape_path:
        with open(shape_path) as f:
            shape = json.load(f)["rows"]
    recs = []
    for p in paths:
        with open(p) as f:
            recs.append(json.load(f))
    parents, these = recs[0::2], recs[1::2]
    lines = ["| workload | clip lengths, s | clips (two-stage / short) | frames in all | intermediate, MB (peak) | poly grid (x by columns per range) | workgroups that skip | imbalance between columns | parent (clip by clip), us | this tree, us | parent / this | accepted |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for i, rb in enumerate(these[0]["rows"]):
        pa = [t for r in parents for t in r["rows"][i]["ts"]]
        pb = [t for r in these for t in r["rows"][i]["ts"]]
        for r in parents + these:
            assert (r["rows"][i]["name"], r["rows"][i]["seconds"], r["rows"][i]["clips"], r["rows"][i]["frames"]) == (rb["name"], rb["seconds"], rb["clips"], rb["frames"])
            assert r["rows"][i]["checksum"] == r["rows"][i]["checksum_last"], "a library's result changed between repetitions: %r" % rb["name"]
        ma, mb = statistics.median(pa), statistics.median(pb)
        spread = max(max(pa) - min(pa), max(pb) - min(pb))
        ok = mb <= ma + spread
        sh = shape[i] if shape else None
        if sh:
            assert (sh["name"], sh["seconds"], sh["clips"], sh["frames"]) == (rb["name"], rb["seconds"], rb["clips"], rb["frames"])
        lines.append("| %s | %g-%g | %d (%d / %d) | %d | %.0f (%.0f) | %s | %s | %s | %.0f (%.0f-%.0f) | %.0f (%.0f-%.0f) | %.2f | %s |" % (
            rb["name"], rb["seconds"][0], rb["seconds"][1], rb["clips"], rb["two_stage"], rb["short"], rb["frames"], rb["mid_mb"], rb["mid_peak_mb"],
            sh["grids"] if sh else "n/a", "%.1f %%" % (100 * sh["skip_share"]) if sh else "n/a", "%.0f %%" % (100 * sh["imbalance"]) if sh else "n/a", ma, min(pa), max(pa), mb, min(pb), max(pb), ma / mb, "yes" if ok else "NO"))
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(text)


def shape_of(n_in, n_out, up, width, budget=1 << 30):
    """clips by class and the intermediate in bytes (all columns, largest range), with the rules of csrc/poly_rules.h restated
    roughly (pad and the 8-element rounding left out)"""
    adm = [(i, o) for i, o in zip(n_in, n_out) if min(i, o) >= 8192]
    mids = [2 * (i if up else o) for i, o in adm]
    peak, run = 0, 0
    for m in mids:
        if run and (run + m) * width > budget:
            peak, run = max(peak, run), 0
        run += m
    peak = max(peak, run)
    return len(adm), sum(1 for o in n_out if o) - len(adm), sum(mids) * width, peak * width


def launch_shape(log_text, n_in, n_out, up):
    """From the launch's own poly log lines (one per range: grid=, R=, n_out= of its longest column, ragged= its columns) and each
    column's tile count: (grids, share of workgroups that leave at the skip test, imbalance between columns).  Mono clips: a
    column is a clip.  A column's polyphase outputs are the clip's outputs (up) or its intermediate, 2 n_out + 2 pad (down; whole
    clips) — 2 pad read off the range's longest column."""
    lines = [dict(tok.split("=", 1) for tok in ln.split()) for ln in log_text.split("\n") if ln.startswith("kernel=poly")]
    assert lines and all("ragged" in f for f in lines), "no ragged polyphase launch in the log: %r" % log_text[:300]
    outs = [o for i, o in zip(n_in, n_out) if min(i, o) >= 8192]
    pos, grids, skipped, wgs, tiles_all = 0, [], 0, 0, []
    for f in lines:
        cols, tile = int(f["ragged"]), 256 * int(f["R"])
        gx, gy = (int(v) for v in f["grid"].split("x")[:2])
        mine = outs[pos:pos + cols]
        pos += cols
        assert gy == cols == len(mine)
        pad2 = 0 if up else int(f["n_out"]) - 2 * max(mine)
        assert 0 <= pad2 <= 512 and (up and int(f["n_out"]) == max(mine) or not up)
        tiles = [-(-(o if up else 2 * o + pad2) // tile) for o in mine]
        assert max(tiles) == int(f["tiles"])
        skipped += sum(max(0, gx - t) for t in tiles)
        wgs += gx * cols
        tiles_all += tiles
        grids.append("%dx%d R=%s" % (gx, cols, f["R"]))
    assert pos == len(outs)
    return ", ".join(grids), skipped / wgs, 1 - sum(tiles_all) / (max(tiles_all) * len(tiles_all))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", help="write this library's rows here")
    ap.add_argument("--merge", nargs="+", metavar="JSON", help="PARENT THIS [PARENT THIS ...] --json records -> a markdown table")
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shape", help="debug-switch build with HIPSOXR_DEBUG_LAUNCH_LOG: one launch per row, the launch's shape from its log -> this file")
    ap.add_argument("--with-shape", help="(--merge) a --shape record: fills the grid, skip and imbalance columns")
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out, args.with_shape)
    import torch
    assert torch.cuda.is_available(), "time_ragged_two_stage.py needs a GPU"
    from soxr_amd import _native, device as dev, dist

    rows = []
    for name, fi, fo, q, dtype, counts, ranges in WORKLOADS:
        plan = dev.Plan(fi, fo, q)
        assert plan.phases != 0, "an interpolated-phase plan"
        tdt = getattr(torch, dtype)
        for lo, hi in ranges:
            for n_clips in counts:
                rng = np.random.default_rng(n_clips)
                n_in = [int(v) for v in rng.integers(int(lo * fi), int(hi * fi) + 1, n_clips)]
                total = sum(n_in)
                g = torch.Generator(device="cuda").manual_seed(n_clips)
                packed = (torch.rand((total,), dtype=torch.float32, device="cuda", generator=g) - 0.5).to(tdt)
                clips = list(torch.split(packed, n_in))
                job = dist.RaggedJob(plan, clips)
                log_path, log_pos = os.environ.get("HIPSOXR_DEBUG_LAUNCH_LOG"), 0
                if args.shape:
                    assert log_path, "--shape reads HIPSOXR_DEBUG_LAUNCH_LOG (debug-switch build)"
                    log_pos = os.path.getsize(log_path) if os.path.exists(log_path) else 0
                job.launch()
                torch.cuda.synchronize()
                if args.shape:
                    with open(log_path) as fh:
                        fh.seek(log_pos)
                        grids, skip, imb = launch_shape(fh.read(), n_in, job.n_out, fo > fi)
                    rows.append(dict(name=name, seconds=[lo, hi], clips=n_clips, frames=total, grids=grids, skip_share=skip, imbalance=imb))
                    print("%-32s %4g-%-4g s %5d clips  grid %s  skip %.1f %%  imbalance %.0f %%" % (name, lo, hi, n_clips, grids, 100 * skip, 100 * imb), flush=True)
                    del job, clips, packed
                    torch.cuda.empty_cache()
                    continue
                checksum = float(job.y.to(torch.float64).sum().item())
                for _ in range(2):
                    job.launch()
                torch.cuda.synchronize()
                ts = []
                for _ in range(args.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    job.launch()
                    e1.record()
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1) * 1e3)  # us
                torch.cuda.synchronize()
                last = float(job.y.to(torch.float64).sum().item())
                two, short, mid, peak = shape_of(n_in, job.n_out, fo > fi, packed.element_size())
                rows.append(dict(name=name, seconds=[lo, hi], clips=n_clips, frames=total, checksum=checksum, checksum_last=last, ts=ts, two_stage=two, short=short,
                                 mid_mb=mid / 1e6, mid_peak_mb=peak / 1e6))
                print("%-32s %4g-%-4g s %5d clips (%d two-stage, %d short)  %10d frames  %.0f us (%.0f-%.0f)  sums %s" % (
                    name, lo, hi, n_clips, two, short, total, statistics.median(ts), min(ts), max(ts), "equal" if checksum == last else "DIFFER"), flush=True)
                del job, clips, packed
                torch.cuda.empty_cache()
    if args.shape:
        args.json = args.shape
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(dict(library=_native.LIB_PATH, rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
