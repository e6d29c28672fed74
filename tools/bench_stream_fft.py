#!/usr/bin/env python3
"""Device streams, default (canonical-order) engine against engine="fft" (HIPSOXR_STREAM_FFT), time per call.

    python tools/bench_stream_fft.py --out stream_fft.json [--alternations 5]

ONE build, one process: the default stream IS the behaviour of the commit before the flag.  Configurations: 48 kHz ->
44.1 kHz VHQ float32 mono and stereo, int16 stereo; 44.1 kHz -> 16 kHz VHQ float32 8 channels.  Chunk lengths 0.1 s, 1 s,
10 s, 60 s.  Per configuration and chunk length one stream of either kind is kept alive and fed through the C entry
(hipsoxr_stream_process_device, preallocated result buffer, input buffers rotated); the two kinds are measured
alternately, `--alternations` times each: a measurement is one HIP-event window around `calls` back-to-back calls (the
chunk's device-to-device copy into the ring included — a stream call has it, a one-shot job does not), reported per
call.  The first window of every stream is warm-up (ring allocation, table build) and is not recorded.  Median and
spread (max - min over the alternations, in % of the median) per leg; the crossover is the shortest chunk length from
which engine="fft" stays ahead.  One JSON record per line in --out, a table on stdout."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-soxr_amd"))
CONFIGS = [("f32_mono_48k_44k1", 48000, 44100, 1, "float32"), ("f32_stereo_48k_44k1", 48000, 44100, 2, "float32"),
           ("i16_stereo_48k_44k1", 48000, 44100, 2, "int16"), ("f32_8ch_44k1_16k", 44100, 16000, 8, "float32")]
SECONDS = [0.1, 1.0, 10.0, 60.0]
CALLS = {0.1: 40, 1.0: 20, 10.0: 6, 60.0: 3}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True)
    ap.add_argument("--alternations", type=int, default=5)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    torch.zeros(1, device="cuda").cpu()          # torch's HIP context first (see tests/conftest.py)
    from soxr_amd import _native as _n, device as dev
    fn = _n.lib.hipsoxr_stream_process_device
    stream = torch.cuda.current_stream().cuda_stream
    torch.manual_seed(0)
    recs = []
    with open(a.out, "w") as f:
        for name, in_rate, out_rate, ch, dt in CONFIGS:
            dtype = getattr(torch, dt)
            for sec in SECONDS:
                frames, calls = int(sec * in_rate), CALLS[sec]
                cap = int(frames * out_rate / in_rate) + 4096
                shape = (frames, ch) if ch > 1 else (frames,)
                xs = []
                for _ in range(3):
                    v = torch.randn(shape, device="cuda")
                    xs.append((v * 0.25).to(dtype) if dtype.is_floating_point else torch.round(v * 5000).to(dtype))
                out = torch.empty((cap, ch) if ch > 1 else (cap,), dtype=dtype, device="cuda")
                done = C.c_size_t(0)
                streams = {e: dev.TensorStream(in_rate, out_rate, ch, dtype=dtype, quality="VHQ", engine=e) for e in ("exact", "fft")}
                per = {"exact": [], "fft": []}
                for alt in range(a.alternations + 1):   # (alternation 0: warm-up)
                    for eng in ("exact", "fft"):
                        h = streams[eng]._h
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for i in range(calls):
                            _n.check(fn(h, xs[i % 3].data_ptr(), frames, out.data_ptr(), cap, C.byref(done), stream))
                        e1.record()
                        e1.synchronize()
                        if alt:
                            per[eng].append(e0.elapsed_time(e1) * 1e3 / calls)
                for eng, v in per.items():
                    v.sort()
                    med = v[len(v) // 2]
                    rec = {"config": name, "chunk_s": sec, "engine": eng, "us_per_call": med, "us_min": v[0], "us_max": v[-1],
                           "spread_pct": 100 * (v[-1] - v[0]) / med, "alternations": a.alternations, "calls_per_window": calls,
                           "version": _n.version()}
                    recs.append(rec)
                    f.write(json.dumps(rec) + "\n")
                    f.flush()
                del streams, xs, out
    print(f"{'configuration':22s} {'chunk':>6s} {'exact us':>10s} {'spread':>7s} {'fft us':>10s} {'spread':>7s} {'exact/fft':>9s}")
    for name, *_ in CONFIGS:
        def leg(sec, eng):
            return next(r for r in recs if r["config"] == name and r["chunk_s"] == sec and r["engine"] == eng)
        cross = None
        for sec in reversed(SECONDS):   # the shortest chunk length from which engine="fft" stays ahead
            if leg(sec, "fft")["us_per_call"] >= leg(sec, "exact")["us_per_call"]:
                break
            cross = sec
        for sec in SECONDS:
            ex, ff = leg(sec, "exact"), leg(sec, "fft")
            print(f"{name:22s} {sec:5.1f}s {ex['us_per_call']:10.2f} {ex['spread_pct']:6.1f}% {ff['us_per_call']:10.2f} {ff['spread_pct']:6.1f}% "
                  f"{ex['us_per_call'] / ff['us_per_call']:9.2f}")
        print(f"{name:22s} crossover: " + (f"engine=\"fft\" ahead from {cross} s chunks up" if cross is not None
                                           else "engine=\"fft\" is not ahead at the longest chunk"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
