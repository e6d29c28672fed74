#!/usr/bin/env python
"""bench.py — headline benchmark of the hot path (BASELINE.json: "Msamples/sec VHQ 48k->44.1k
float32; achieved HBM GB/s vs roofline @1/2/4/8 GPU").

    python bench.py --gpus N --steps K --warmup W          (N > 1: starts its own N ranks through torch.distributed.run)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W        (the driver's form: WORLD_SIZE must equal N)
    python bench.py ... --full                  (also every context leg below: batch, configs[2], other engines and
                                                 precisions, roofline probes, host API, CPU baseline, full record)
    python bench.py ... --dump-outputs DIR      (after the timed steps: the last step's output as DIR/resampled.npy)

A plain run (no --full) does what the headline needs and nothing else: plan, input, W warm-up launches, the K timed
launches, the line.  Its `roofline.launch_us` is then the timed steps' own wall time per step; --full takes it from
HIP-event windows around the timed region instead, and adds the legs described below.

A "step" is one pass of the hot path (one hipsoxr_run_device launch) over one batch of synthetic
input that is already resident in HBM.  Workload (config.workload):
  * default: BASELINE.json configs[1] — VHQ 48000->44100 float32, 60 s mono, per GPU;
  * the same JSON line also carries `batch_shard`: the per-GPU shard of configs[3]
    (1024 independent 10 s clips over 8 GPUs = 128 clips per GPU), timed the same way.
Multi-GPU: the path shards by independent clips — every rank resamples its own clips, no data-path
collective; the only collective is the RCCL broadcast of the shared filter bank from rank 0 at plan
time (outside the timed region).  Per-GPU work is fixed as N grows -> "scaling": "weak".

Msamples/s = input samples consumed per second.  `roofline` is computed from the
ALGORITHMIC bytes of one launch (4 B in + 4 B out per sample: 8.354 B per output sample at
48k->44.1k) divided by the average launch duration measured with HIP events on the launch stream.
`cpu_baseline` times the oracle (single-thread C restatement, kind "port" — libsoxr itself is not
available in this image) on rank 0 over a bounded sample of the same workload; `cpu_baseline.fft_overlap_save` is
the same filter applied the way libsoxr's sharp stages work (FFT overlap-save, scipy.fft), 1 core and all cores.

Buffers: the 60 s clip (22 MB) re-runs on one input / output pair — it lives in the 256 MB Infinity Cache whatever
is done, and the line says so.  The batch lines ROTATE through several input / output sets (>= 1.4 GB in all) so that
nothing a launch reads was left in a cache by the launch before: the figure is HBM traffic, not cache traffic
(`buffer_sets`; with one set the non-temporal result stores of round 4 leave the 246 MB input cache-resident from
launch to launch and the launch looks 8 % faster than it is on fresh data — profiles/r04_ab_experiments.txt §5).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "python-soxr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

IN_RATE, OUT_RATE, QUALITY = 48000, 44100, "VHQ"
KERNEL_NAMES = {0: "k_fft_pair2<.., float> (AUTO: frequency-domain engine, paired-block kernel, for large float32 device jobs)",
                1: "k_gather<float,float>", 2: "k_tile_mfma_p<float>", 3: "k_tile<float,float,16,true>",
                4: "k_tile_mfma_p<float>", 5: "k_fft_pair2<.., float>", 6: "k_tile_mfma_p<float> (EXACT: canonical-order engine)"}
# HBM traffic and VALU wave-instructions per launch come from rocprofv3 PMC passes (bench.py cannot collect counters
# itself): profiles/<TRAFFIC_FILE> records them TOGETHER WITH the SHA-256 of the kernel sources they were taken on.
# `measured_counters()` hands a figure out only while that hash still matches the sources in this checkout — a stale
# constant is reported as null with the reason, never silently.
TRAFFIC_FILE = "r06_traffic.json"
KERNEL_SOURCES = ("python-soxr_amd/csrc/fft.hip", "python-soxr_amd/csrc/fft_dev.h", "python-soxr_amd/csrc/fftwave.hip", "python-soxr_amd/csrc/kernels.hip",
                  "python-soxr_amd/csrc/kernels_interp.h", "python-soxr_amd/csrc/kernels_chain.h", "python-soxr_amd/csrc/kernels_tile.h",
                  "python-soxr_amd/csrc/twostage.hip")


def kernel_sources_sha16():
    import hashlib
    h = hashlib.sha256()
    for rel in KERNEL_SOURCES:
        with open(os.path.join(ROOT, rel), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def measured_counters(workload):
    """-> (traffic_bytes | None, valu_wave_insts | None, provenance dict)"""
    path = os.path.join(ROOT, "profiles", TRAFFIC_FILE)
    here = kernel_sources_sha16()
    try:
        with open(path) as f:
            rec = json.load(f)
    except (OSError, ValueError):
        return None, None, {"traffic_source": None, "why": f"profiles/{TRAFFIC_FILE} absent", "kernel_sources_sha16": here}
    prov = {"traffic_source": f"profiles/{TRAFFIC_FILE}", "taken_on_kernel_sources_sha16": rec.get("kernel_sources_sha16"),
            "kernel_sources_sha16": here}
    if rec.get("kernel_sources_sha16") != here:
        prov["why"] = "stale: the kernel sources changed since the counters were collected (re-run tools/prof_bench.sh)"
        return None, None, prov
    w = rec.get("workloads", {}).get(workload)
    if not w:
        prov["why"] = "no record for this workload"
        return None, None, prov
    if w.get("rocprof_avg_us") is not None:   # the kernel's average duration in the committed rocprofv3 kernel trace
        prov["rocprof_avg_us"] = w["rocprof_avg_us"]
    return w.get("traffic_bytes"), w.get("valu_wave_insts"), prov


VALU_SLOTS_PER_S = 256 * 4 * 2.4e9 / 2
HBM_PEAK_GBS = 8000.0      # MI355X HBM3E spec (MI355X_MICROARCH.md)
VALU_PEAK_TFLOPS = 157.3   # fp32 vector peak


def shard(n_units, world, rank):
    """soxr_amd.dist.shard (the product owns the partition rule; kept here as the name older tools import)."""
    from soxr_amd import dist as sdist
    return sdist.shard(n_units, world, rank)


def broadcast_bank(plan, rank, world, device):
    """soxr_amd.dist.broadcast_bank over torch's communicator (RCCL over xGMI for backend nccl)."""
    from soxr_amd import dist as sdist
    if world > 1:
        sdist.broadcast_bank(plan, device=device)


def gather_rank_info(plan, rank, world, device, backend):
    from soxr_amd import dist as sdist
    return sdist.rank_info(plan, device=device)


def time_workload(plan, x, steps, warmup, world, device, kernel=0, windows=50, min_window=0):
    """W warm-up launches, then exactly K timed launches bracketed by barrier + synchronize (the contract region).
    Returns (wall seconds for K steps [max over ranks], launch duration from HIP events [s], output).
    x: one tensor, or a LIST of equally shaped tensors — buffer sets a step rotates through (step i runs on set
    i mod len(x), each with its own output), so that no launch finds its input in a cache.
    The launch duration is the MEDIAN over `windows` event windows of max(K, min_window) launches each (HIP events on
    the launch stream): at the driver's K = 20 the contract region of the 60 s clip lasts 0.3 ms, too short for one
    window to be a measurement, and a window of a handful of launches also counts the gaps between them (round 3: 5-launch
    windows of the batch read 131 us where rocprofv3 and the 3 s sustained leg said 122.5).  Half of the windows run
    BEFORE the contract region (they are warm-up as far as the contract is concerned) and half AFTER it, so that both
    figures are taken at the same clock state of the chip.  A step is the same thing in every window."""
    import torch
    import torch.distributed as dist
    from soxr_amd import device as dev
    xs = list(x) if isinstance(x, (list, tuple)) else [x]
    ys = [dev.resample_tensor(plan, xi, kernel=kernel) for xi in xs]
    jobs = [dev.PreparedJob(plan, xi, yi, kernel=kernel) for xi, yi in zip(xs, ys)]  # descriptor built once; a step = one C call = one launch
    nj = len(jobs)
    turn = [0]

    def launch(n):
        t = turn[0]
        for i in range(n):
            jobs[(t + i) % nj].launch()
        turn[0] = (t + n) % nj

    launch(warmup)
    torch.cuda.synchronize(device)
    per = []
    win = max(steps, min_window)

    def event_windows(n):
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch(win)
            e1.record()
            e1.synchronize()
            per.append(e0.elapsed_time(e1) * 1e-3 / win)

    event_windows(windows // 2)
    torch.cuda.synchronize(device)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize(device)
    # The contract region holds the K launches and nothing else: the HIP events of the kernel timing (two more
    # packets on the stream, ~0.4 us per step at the driver's K = 20) are recorded in the windows around it.
    t0 = time.perf_counter()
    launch(steps)
    torch.cuda.synchronize(device)
    wall = time.perf_counter() - t0  # this rank's K steps; the MAX over ranks is taken below, behind the closing bracket
    if world > 1:                    # (a collective's own latency is tens of us: not part of K x 12 us steps)
        dist.barrier()
    torch.cuda.synchronize(device)
    event_windows(windows - windows // 2)
    kern = wall / steps
    if per:
        per.sort()
        kern = per[len(per) // 2]
    if world > 1:
        t = torch.tensor([wall], dtype=torch.float64, device=device if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall = float(t.item())
    return wall, kern, ys[0]


class _SmiSampler:
    """Board power and shader clock from `rocm-smi`, sampled in a thread beside a run (rank 0).  The batch launch runs
    AT the board's power cap: time = energy / cap, and the line should say at what power and clock it was taken."""

    def __init__(self):
        import threading
        self.samples, self._stop = [], False
        self._t = threading.Thread(target=self._run, daemon=True)

    def _run(self):
        import re
        import subprocess
        while not self._stop:
            try:
                out = subprocess.run(["rocm-smi", "--showpower", "--showclocks"], capture_output=True, text=True, timeout=5).stdout
            except Exception:
                return
            pw = re.findall(r"Power \(W\): ([0-9.]+)", out)
            sc = re.findall(r"sclk clock level: \w+: \((\d+)Mhz\)", out)
            if pw and sc:
                self.samples.append((float(pw[0]), sum(map(int, sc)) / len(sc)))

    def __enter__(self):
        self._t.start()
        return self

    def __exit__(self, *a):
        self._stop = True
        self._t.join(timeout=10)

    def summary(self):
        mid = self.samples[len(self.samples) // 3:] or self.samples   # (the first samples see the clock ramp)
        if not mid:
            return {"power_W": None, "sclk_MHz": None, "smi_samples": 0}
        return {"power_W": sum(p for p, _ in mid) / len(mid), "sclk_MHz": sum(c for _, c in mid) / len(mid), "smi_samples": len(self.samples)}


def sustained_leg(plan, x, seconds, device, kernel=0, sample_power=False):
    """The batch workload launched back to back for `seconds` of wall time (>= 3 s), rotating through the buffer sets of
    `x` (a list): long enough for an outside observer (the driver's gpu_busy sampler, rocm-smi) to see the GPU busy and
    to corroborate the per-launch time, and for rocm-smi to report the power and clock the launches ran at."""
    import torch
    from soxr_amd import device as dev
    xs = list(x) if isinstance(x, (list, tuple)) else [x]
    jobs = [dev.PreparedJob(plan, xi, dev.resample_tensor(plan, xi, kernel=kernel), kernel=kernel) for xi in xs]
    torch.cuda.synchronize(device)
    smi = _SmiSampler() if sample_power else None
    if smi:
        smi.__enter__()
    n, t0 = 0, time.perf_counter()
    while True:
        for i in range(200):
            jobs[(n + i) % len(jobs)].launch()
        n += 200
        torch.cuda.synchronize(device)
        if time.perf_counter() - t0 >= seconds:
            break
    dt = time.perf_counter() - t0
    power = {}
    if smi:
        smi.__exit__()
        power = smi.summary()
    return n, dt, power


def cpu_baseline(seconds_in=60, budget_s=10.0):
    """Oracle (float64 CPU restatement, one thread) on the same 60 s mono workload, repeated for
    ~budget_s seconds.  Two context numbers ride along (CPU side): the same oracle over
    independent clips on all host threads (the reference's scaling model, tests/gil_bench.py:22-56),
    and scipy.signal.resample_poly with the same prototype as an independent third-party figure."""
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor
    from oracle import oracle
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(IN_RATE * seconds_in) * 0.25).astype(np.float32)
    x64 = x.astype(np.float64)
    pl = oracle.plan(IN_RATE, OUT_RATE, QUALITY)
    oracle.resample_channel(pl, x64[:48000], "ref")  # warm up
    t0 = time.perf_counter()
    n = 0
    while True:
        oracle.resample_channel(pl, x.astype(np.float64), "ref")
        n += 1
        if time.perf_counter() - t0 > budget_s:
            break
    dt = (time.perf_counter() - t0) / n
    live = live_libsoxr_timing(x)
    if live is not None:  # a real libsoxr on this box: it is the baseline (kind "reference"), the oracle rides along
        live["port"] = {"value": len(x) / dt / 1e6, "unit": "Msamples/s", "cores": 1,
                        "sample": f"oracle/soxr_oracle.c, {seconds_in} s mono x{n} passes"}
        live["host_cpus"] = os.cpu_count()
        return live
    out = {"value": len(x) / dt / 1e6, "unit": "Msamples/s", "cores": 1, "kind": "port", "libsoxr": "absent",
           "sample": f"{seconds_in} s mono float32 48k->44.1k VHQ x{n} passes, float64 accumulate, "
                     f"oracle/soxr_oracle.c (libsoxr itself is absent from this image)",
           "host_cpus": os.cpu_count()}
    ncpu = usable_cpus()
    out["usable_cpus"] = ncpu
    try:  # all usable host threads over independent 10 s clips (the reference's scaling model, tests/gil_bench.py:22-56):
        # the C function called straight through ctypes (GIL released) on preallocated buffers — no per-call allocation or
        # conversion in Python, and as many threads as the container may really run (cgroup quota / affinity, not
        # os.cpu_count(): round 3's 128 threads on a capped container measured the cap, 12.7x, not the cores)
        threads = max(1, min(ncpu, 128))
        clip = np.ascontiguousarray(x64[:IN_RATE * 10])
        n_out = pl.out_len(len(clip))
        bank = np.ascontiguousarray(pl.bank, np.float64)
        outs = [np.empty(n_out, np.float64) for _ in range(threads)]
        fn = oracle.lib().oracle_resample_ref
        reps = 2

        def one(t):
            for _ in range(reps):
                fn(bank.ctypes.data, pl.L, pl.M, pl.T, clip.ctypes.data, 0, len(clip), outs[t].ctypes.data, 0, n_out)

        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(one, range(threads)))       # warm up: threads started, pages touched
            t0 = time.perf_counter()
            list(ex.map(one, range(threads)))
            dt_mt = time.perf_counter() - t0
        out["all_threads"] = {"value": threads * reps * len(clip) / dt_mt / 1e6, "unit": "Msamples/s",
                              "threads": threads, "speedup_over_1": threads * reps * len(clip) / dt_mt / 1e6 / out["value"],
                              "sample": f"{threads * reps} independent 10 s clips, {threads} threads"}
    except Exception as e:  # context only
        out["all_threads"] = {"error": str(e)}
    try:  # the same filter the way libsoxr's sharp stages work: FFT overlap-save (oracle/overlap_save.py, scipy.fft)
        from oracle import overlap_save as ols
        fp = ols.Plan(pl, 256)
        y_ols = ols.resample(fp, x64[:IN_RATE * 2])
        y_ref = oracle.resample_channel(pl, x64[:IN_RATE * 2], "ref")
        err = float(np.sqrt(np.mean((y_ols - y_ref) ** 2)) / np.sqrt(np.mean(y_ref ** 2)))
        t0 = time.perf_counter()
        n1 = 0
        while time.perf_counter() - t0 < 3.0:
            ols.resample(fp, x64)
            n1 += 1
        v1 = n1 * len(x64) / (time.perf_counter() - t0) / 1e6
        threads = max(1, min(ncpu, 128))
        clip = x64[:IN_RATE * 10]
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(lambda _: ols.resample(fp, clip), range(threads)))
            t0 = time.perf_counter()
            list(ex.map(lambda _: ols.resample(fp, clip), range(threads * 2)))
            dtm = time.perf_counter() - t0
        out["fft_overlap_save"] = {"value": v1, "unit": "Msamples/s", "cores": 1, "rel_rms_vs_direct_form": err,
                                   "all_threads": {"value": threads * 2 * len(clip) / dtm / 1e6, "threads": threads},
                                   "sample": f"60 s mono float64 x{n1} passes, blocks of 256 periods (40960 -> 37632 points), scipy.fft (pocketfft); "
                                             f"all_threads: {threads * 2} independent 10 s clips",
                                   "note": "libsoxr's algorithm class for its sharp stages (SURVEY.md §A.4, unverified); the oracle's own prototype"}
    except Exception as e:
        out["fft_overlap_save"] = {"error": str(e)}
    try:
        from scipy.signal import resample_poly
        g = np.zeros(pl.L * pl.T)
        for ph in range(pl.L):
            g[pl.L * (pl.T - 1 - np.arange(pl.T)) + ph] = pl.bank[ph]
        clip = x64[:IN_RATE * 10]
        resample_poly(clip[:4800], pl.L, pl.M, window=g)
        t0 = time.perf_counter()
        reps = 0
        while time.perf_counter() - t0 < 4.0:
            resample_poly(clip, pl.L, pl.M, window=g)
            reps += 1
        out["scipy_resample_poly"] = {"value": reps * len(clip) / (time.perf_counter() - t0) / 1e6,
                                      "unit": "Msamples/s", "cores": 1,
                                      "sample": "10 s mono float64, same prototype (scipy.signal.upfirdn)"}
    except Exception as e:
        out["scipy_resample_poly"] = {"error": str(e)}
    return out


def usable_cpus():
    """CPUs this process may really use: the smaller of its affinity mask and its cgroup's CPU quota (a container on a
    256-thread host is usually capped well below os.cpu_count())."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as f:
                txt = f.read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                q = int(txt[0])
                if q > 0:
                    with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                        n = min(n, max(1, int(q / int(f.read()))))
            break
        except (OSError, ValueError, IndexError):
            continue
    return n


def live_libsoxr_timing(x):
    """If a real libsoxr is importable / loadable at run time: time it the way the
    reference's own harness does (tests/bench.py:42-53: timeit, best of N) on the 60 s mono VHQ clip, and
    report the GPU path's parity against it.  None when absent (this image: always)."""
    try:
        from oracle import live_libsoxr
        live = live_libsoxr.probe()
    except Exception:
        return None
    if live is None:
        return None
    import timeit
    import numpy as np
    live.resample(x[:48000], IN_RATE, OUT_RATE, QUALITY)
    best = min(timeit.repeat(lambda: live.resample(x, IN_RATE, OUT_RATE, QUALITY), number=1, repeat=10))
    out = {"value": len(x) / best / 1e6, "unit": "Msamples/s", "cores": 1, "kind": "reference",
           "libsoxr": live.version, "how": live.how,
           "sample": "60 s mono float32 48k->44.1k VHQ, timeit best of 10 (tests/bench.py:42-53 method)"}
    try:
        import soxr_amd
        ref = np.asarray(live.resample(x, IN_RATE, OUT_RATE, QUALITY), np.float64)
        got = soxr_amd.resample(x, IN_RATE, OUT_RATE, quality=QUALITY).astype(np.float64)
        n = min(len(ref), len(got))
        out["parity_rel_rms_white_noise"] = float(np.sqrt(np.mean((got[:n] - ref[:n]) ** 2)) / np.sqrt(np.mean(ref[:n] ** 2)))
        out["parity_len_equal"] = len(ref) == len(got)
    except Exception as e:
        out["parity_error"] = str(e)
    return out


def configs4_stream(seconds=20):
    """BASELINE configs[4]: ResampleStream 44100->16000 int16, chunked input, state carried across
    launches (host-pointer surface: every call is H2D + kernel + D2H).  us per resample_chunk call and
    Msamples/s for the chunk sizes SURVEY.md §8d names: constant rate (synchronous calls; synchronous calls served
    by the resident kernel — no HIP call per chunk; deferred output — each call returns the previous call's
    frames, no GPU round trip inside the call) and variable rate."""
    import numpy as np
    import soxr_amd as soxr
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(44100 * seconds) * 5000).astype(np.int16)
    out = {"workload": f"BASELINE configs[4]: ResampleStream 44100->16000 int16 VHQ mono, {seconds} s, chunked "
                       f"(host numpy in/out per call, state on device)"}
    for vr, deferred, resident in ((False, False, False), (False, False, True), (False, False, "auto"), (False, True, False), (True, False, False)):
        for chunk in (441, 4410, 96000):
            if resident and chunk == 96000:
                continue  # (beyond what the resident kernel serves: same as the synchronous leg)
            if resident == "auto" and chunk != 441:
                continue
            rs = soxr.ResampleStream(44100, 16000, 1, dtype="int16", quality="VHQ", vr=vr, deferred=deferred,
                                     resident=resident)
            rs.resample_chunk(x[:chunk])  # warm up: buffers, plan tables
            rs.clear()
            n_calls = 0
            t0 = time.perf_counter()
            for a in range(0, len(x), chunk):
                if vr and n_calls == 8:
                    rs.set_io_ratio(44100, 22050, 1000)  # one ratio change with a slew, mid-stream
                rs.resample_chunk(x[a:a + chunk], last=(a + chunk >= len(x)))
                n_calls += 1
            dt = time.perf_counter() - t0
            key = f"{'vr' if vr else 'cr_deferred' if deferred else 'cr_auto_resident' if resident == 'auto' else 'cr_resident' if resident else 'cr'}_chunk{chunk}"
            out[key] = {"us_per_call": dt / n_calls * 1e6, "calls": n_calls, "Msamples_per_s": len(x) / dt / 1e6}
            if chunk == 441 and not vr:
                # a real-time caller feeds a chunk every 10 ms: time spent INSIDE the call when calls are spaced
                # (here 300 us apart), i.e. the latency the caller sees rather than the back-to-back rate
                rs.clear()
                inside = 0.0
                for a in range(0, 441 * 300, chunk):
                    t1 = time.perf_counter()
                    rs.resample_chunk(x[a:a + chunk])
                    t2 = time.perf_counter()
                    inside += t2 - t1
                    while time.perf_counter() - t2 < 300e-6:
                        pass
                out[key]["us_in_call_when_spaced"] = inside / 300 * 1e6
    # the same stream with the chunks already in HBM (soxr_amd.device.TensorStream): pending input stays on the device,
    # a call is one asynchronous launch on the current stream — no PCIe, no host synchronisation inside the call
    try:
        import torch
        from soxr_amd import device as dev
        xd = torch.from_numpy(x).cuda()
        for chunk in (441, 4410, 96000):
            ts = dev.TensorStream(44100, 16000, 1, dtype=torch.int16, quality="VHQ")
            for a in range(0, min(len(x), 300 * chunk), chunk):   # warm up: module load, allocator, clocks (a 20 ms leg sees the ramp otherwise)
                ts.resample_chunk(xd[a:a + chunk])
            ts.clear()
            torch.cuda.synchronize()
            n_calls = 0
            t0 = time.perf_counter()
            for a in range(0, len(x), chunk):
                ts.resample_chunk(xd[a:a + chunk], last=(a + chunk >= len(x)))
                n_calls += 1
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out[f"device_chunk{chunk}"] = {"us_per_call": dt / n_calls * 1e6, "calls": n_calls, "Msamples_per_s": len(x) / dt / 1e6,
                                           "note": "chunks and results are device tensors; one sync after the last call"}
        # many live streams in lock step are the CHANNELS of one handle (channels are independent columns): 128 of them,
        # 10 ms chunks each, one copy kernel and one launch per call for all
        nch = 128
        xm = (torch.randn((441 * 400, nch), device="cuda") * 5000).to(torch.int16)
        ts = dev.TensorStream(44100, 16000, nch, dtype=torch.int16, quality="VHQ")
        ts.resample_chunk(xm[:441])
        ts.clear()
        torch.cuda.synchronize()
        n_calls = 0
        t0 = time.perf_counter()
        for a in range(0, xm.shape[0], 441):
            ts.resample_chunk(xm[a:a + 441], last=(a + 441 >= xm.shape[0]))
            n_calls += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out["device_chunk441_x128_streams"] = {"us_per_call": dt / n_calls * 1e6, "calls": n_calls, "streams": nch,
                                               "Msamples_per_s": xm.numel() / dt / 1e6,
                                               "note": "128 lock-step mono streams as the channels of one handle, 441-frame chunks"}
        # ... and N INDEPENDENT handles (different phases and pending counts: every stream is fed a prefix of its own length
        # first) served by ONE launch per call: soxr_amd.device.TensorStreamGroup / hipsoxr_streams_process_device
        grp = dev.TensorStreamGroup(nch, 44100, 16000, 1, dtype=torch.int16, quality="VHQ", dither_seeds=list(range(nch)))
        for i, s in enumerate(grp.streams):
            s.resample_chunk(xm[: 7 * i, 0].contiguous())
        xg = xm.t().contiguous()                       # [streams, frames]
        grp.resample_chunks(xg[:, :441].contiguous())
        torch.cuda.synchronize()
        chunks = [xg[:, a:a + 441].contiguous() for a in range(441, xg.shape[1], 441)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for c in chunks:
            grp.resample_chunks(c)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out["device_chunk441_x128_independent_handles"] = {"us_per_call": dt / len(chunks) * 1e6, "calls": len(chunks), "streams": nch,
                                                           "Msamples_per_s": nch * 441 * len(chunks) / dt / 1e6,
                                                           "note": "128 independent stream handles (own phases, pending counts, dither seeds), 441-frame chunks each, one launch per call"}
    except Exception as e:  # noqa: BLE001
        out["device_stream"] = {"error": str(e)}
    return out


def dtype_matrix(plan, device, seconds, steps):
    """The other three I/O dtypes as device-resident jobs on the configs[1] shape (60 s mono): float64 and
    int32 run the f64 engine, int16 the f32 engine (exact engine for all; AUTO = what a caller gets)."""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(77)
    n_in = IN_RATE * seconds
    base = torch.randn(n_in, device=device, dtype=torch.float64, generator=g) * 0.25
    out = {}
    for name, x in (("float64", base), ("int32", (base * 2 ** 30).to(torch.int32)), ("int16", (base * 2 ** 14).to(torch.int16))):
        _, k, y = time_workload(plan, x, max(5, steps // 4), 3, 1, device, kernel=0, windows=10)
        nbytes = x.element_size() * (x.numel() + y.numel())
        out[name] = {"launch_us": k * 1e6, "Msamples_per_s": n_in / k / 1e6,
                     "hbm_frac": nbytes / k / 1e9 / HBM_PEAK_GBS, "direct_form_equiv_tflops": 2.0 * plan.taps * y.numel() / k / 1e12}
        del x, y
    return out


def host_api_timings():
    """PCIe-inclusive figures of the drop-in surface (numpy in, numpy out) — never the headline
    `value`.  configs[0] is the case the reference's README quotes (10 s, 48k->44.1k: soxr HQ 10.8 ms,
    VHQ 14.5 ms on an unspecified Colab CPU, README.md:97-99)."""
    import numpy as np
    import soxr_amd as soxr
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(IN_RATE * 60) * 0.25).astype(np.float32)
    out = {}
    for key, arr, q in (("configs0_10s_HQ", x[:IN_RATE * 10], "HQ"), ("10s_VHQ", x[:IN_RATE * 10], "VHQ"),
                        ("configs1_60s_VHQ", x, "VHQ")):
        soxr.resample(arr, IN_RATE, OUT_RATE, quality=q)
        best = 1e9
        for _ in range(10):
            t0 = time.perf_counter()
            soxr.resample(arr, IN_RATE, OUT_RATE, quality=q)
            best = min(best, time.perf_counter() - t0)
        out[key] = {"ms_per_call": best * 1e3, "Msamples_per_s": len(arr) / best / 1e6}
    out["note"] = ("soxr_amd.resample on host numpy arrays, best of 10 (H2D + kernel + D2H + bit-exact engine); "
                   "published for the reference on other hardware: HQ 10.8 ms, VHQ 14.5 ms per 10 s clip")
    return out


def _host_link_rate(block=16 << 20, n=24):
    """GB/s per direction of pinned <-> device copies of 64 MB blocks, both directions at once on two streams (the
    traffic shape of dist._HostPipe): what the link of THIS box delivers, beside the 63 GB/s of the spec."""
    import torch
    pin = [torch.empty(block, dtype=torch.float32, pin_memory=True) for _ in range(2)]
    dev = [torch.empty(block, dtype=torch.float32, device="cuda") for _ in range(2)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    best = 1e9
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _k in range(n):
            with torch.cuda.stream(s1):
                dev[0].copy_(pin[0], non_blocking=True)
            with torch.cuda.stream(s2):
                pin[1].copy_(dev[1], non_blocking=True)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return block * 4 * n / best / 1e9


def host_batch(n_clips=1024, seed=11):
    """A host corpus end to end (the reference's scaling model: threads over independent HOST arrays,
    tests/gil_bench.py:22-56): `n_clips` ragged 5-15 s mono float32 clips as numpy arrays through
    soxr_amd.dist.resample_batch on the visible device — pinned staging ring, H2D / launch / D2H overlapped.  Msamples/s
    host to host and the fraction of the PCIe floor (63 GB/s per direction, both directions at once: the larger of
    input and output bytes)."""
    import numpy as np
    from soxr_amd import dist as sdist
    rng = np.random.default_rng(seed)
    lens = rng.integers(5 * IN_RATE, 15 * IN_RATE + 1, size=n_clips)
    pool = (rng.standard_normal(15 * IN_RATE + n_clips) * 0.25).astype(np.float32)
    clips = [pool[i:i + int(n)].copy() for i, n in enumerate(lens)]
    b_in = sum(c.nbytes for c in clips)
    res = {}
    for name, pinned in (("pinned_results", True), ("pageable_results", False)):
        outs = sdist.resample_batch(clips, IN_RATE, OUT_RATE, QUALITY, devices=[0], pinned_results=pinned)   # warm up: plan, rings, the host allocator's cache
        b_out = sum(o.nbytes for o in outs)
        best = 1e9
        for _ in range(3):
            outs = None                                                   # (the pinned buffers of the run before go back to the cache)
            t0 = time.perf_counter()
            outs = sdist.resample_batch(clips, IN_RATE, OUT_RATE, QUALITY, devices=[0], pinned_results=pinned)
            best = min(best, time.perf_counter() - t0)
        outs = None
        res[name] = best
    floor = max(b_in, b_out) / 63e9
    link = _host_link_rate()
    best = res["pinned_results"]
    return {"workload": f"{n_clips} ragged 5-15 s mono float32 host clips (numpy in, numpy out), VHQ 48k->44.1k, one device",
            "seconds": best, "Msamples_per_s": sum(len(c) for c in clips) / best / 1e6,
            "GB_in": b_in / 1e9, "GB_out": b_out / 1e9, "pcie_floor_s": floor, "frac_of_pcie_floor": floor / best,
            "seconds_with_pageable_results": res["pageable_results"], "frac_with_pageable_results": floor / res["pageable_results"],
            "link_GBs_per_direction_measured": link, "frac_of_measured_link_floor": max(b_in, b_out) / (link * 1e9) / best,
            "usable_cpus": usable_cpus(),
            "note": "best of 3; results as views of the pinned buffers the D2H copies land in (resample_batch's default up to 8 GiB per call); "
                    "floor = max(input, output bytes) / 63 GB/s (PCIe Gen5 x16 spec, both directions concurrently); link_GBs_per_direction_measured = pinned 64 MB "
                    "copies both ways at once on this box"}


def hbm_ceiling(device, n_bytes=1 << 30):
    """What this box's HBM delivers to plain streaming kernels, so that roofline fractions can also be read against
    the achievable rather than the spec peak: the probe kernels of tools/ubench/stream_probe.hip (16 bytes per lane,
    1 / 2 / 4 / 8 loads in flight per lane, temporal and non-temporal; read-only and write-only sweeps) over 1 GiB
    buffers — four times the 256 MiB Infinity Cache — and torch's copy_.  (Round 2 quoted a 4096-workgroup
    grid-stride copy at 4.7 TB/s, well below what the guide documents for a float4 copy, 6.29 TB/s.)"""
    import ctypes
    import torch
    path = os.path.join(ROOT, "tools", "ubench", "libstream_probe.so")
    try:
        probe = ctypes.CDLL(path)
    except OSError as e:
        return {"error": f"{path}: {e} (built by __graft_entry__.build())"}
    probe.stream_probe_run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    probe.stream_probe_name.restype = ctypes.c_char_p
    a = torch.empty(n_bytes // 4, dtype=torch.float32, device=device).normal_()
    b = torch.empty_like(a)
    st = torch.cuda.current_stream(device).cuda_stream
    res = {}
    legs = [(probe.stream_probe_name(m).decode(), (lambda m=m: probe.stream_probe_run(m, b.data_ptr(), a.data_ptr(), n_bytes, st)),
             probe.stream_probe_moves(m) * n_bytes) for m in range(9)]
    legs.append(("torch_copy", lambda: b.copy_(a), 2 * n_bytes))
    for name, fn, moved in legs:
        for _ in range(3):
            fn()
        torch.cuda.synchronize(device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            fn()
        e1.record()
        torch.cuda.synchronize(device)
        res[name + "_GBs"] = moved * 10 / (e0.elapsed_time(e1) * 1e-3) / 1e9
    res["best_copy_GBs"] = max(v for k, v in res.items() if k.startswith(("copy", "torch_copy")))
    res["best_read_GBs"] = max(v for k, v in res.items() if k.startswith("read"))
    res["note"] = "tools/ubench/stream_probe.hip kernels and torch copy_, 1 GiB buffers, HIP events, 10 launches each"
    return res


def spawn_ranks(n):
    """`python bench.py --gpus N` with no launcher around it: re-run this command line as N ranks of one node under
    torch.distributed.run (one process per GPU; rendezvous on 127.0.0.1, a free port) and hand its exit code back.
    Refuses when the box has fewer than N GPUs — unless BENCH_DIST_BACKEND=gloo asks for the harness test, where ranks
    share devices (never for numbers)."""
    import socket
    import subprocess
    import torch
    have = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if os.environ.get("BENCH_DIST_BACKEND", "nccl") == "nccl" and have < n:
        raise SystemExit(f"bench.py --gpus {n}: this box shows {have} HIP device(s); one rank per GPU needs {n} "
                         f"(BENCH_DIST_BACKEND=gloo runs the N-rank harness on fewer devices, for testing only)")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # (the host driver supports dmabuf IPC only: RCCL needs it)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def pattern_floor(device, grid_x, grid_y, hop_in, hop_out, wg_in, wg_out, in_col, out_col, in_len, out_len, lds, threads, sets=3):
    """The memory side of a block-transform launch on its own (tools/ubench/stream_probe.hip `k_pattern`): the same grid,
    LDS footprint and bytes per workgroup as the kernel, no arithmetic; rotating buffer sets.  us per launch, or None."""
    import ctypes
    import torch
    try:
        probe = ctypes.CDLL(os.path.join(ROOT, "tools", "ubench", "libstream_probe.so"))
        fn = probe.stream_probe_pattern
    except (OSError, AttributeError):
        return None
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                   ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p]
    n_in, n_out = max(in_col * grid_y, in_len), max(out_col * grid_y, out_len)
    xs = [torch.randn(int(n_in) + 16, device=device) for _ in range(sets)]
    ys = [torch.empty(int(n_out) + 16, device=device) for _ in range(sets)]
    st = torch.cuda.current_stream(device).cuda_stream

    def go(n):
        for i in range(n):
            fn(ys[i % sets].data_ptr(), xs[i % sets].data_ptr(), grid_x, grid_y, hop_in, hop_out, wg_in, wg_out, in_col, out_col,
               in_len, out_len, lds, threads, st)
    go(5)
    torch.cuda.synchronize(device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); go(60); e1.record()
    torch.cuda.synchronize(device)
    return e0.elapsed_time(e1) * 1e3 / 60


def launch_floor(device, n=400):
    """us per launch of an EMPTY kernel, back to back on the current stream: the floor under any one-kernel step."""
    import ctypes
    import torch
    try:
        probe = ctypes.CDLL(os.path.join(ROOT, "tools", "ubench", "libstream_probe.so"))
        fn = probe.stream_probe_empty
    except (OSError, AttributeError):
        return None
    fn.argtypes = [ctypes.c_void_p]
    st = torch.cuda.current_stream(device).cuda_stream
    for _ in range(20):
        fn(st)
    torch.cuda.synchronize(device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn(st)
    e1.record()
    torch.cuda.synchronize(device)
    return e0.elapsed_time(e1) * 1e3 / n


def power_leg(plan, xs, seconds, device, kernel, nbytes):
    """A short sustained leg of one workload with rocm-smi beside it -> power, clock and energy per launch."""
    n, dt, pw = sustained_leg(plan, xs, seconds, device, kernel, sample_power=True)
    us = dt / n * 1e6
    return {"us_per_launch": us, "frac": nbytes / (dt / n) / 1e9 / HBM_PEAK_GBS, **pw,
            "energy_mJ_per_launch": pw["power_W"] * dt / n * 1e3 if pw.get("power_W") else None}


# ---- the ONE line the driver keeps ---------------------------------------------------------------------------------------
# The driver's record holds the last ~8 KB of stdout + stderr; round 5's 12.4 KB line lost `configs2`, `batch_shard` and
# `batch_strong` that way.  The printed line is therefore a COMPACT form of the result (<= LINE_BUDGET bytes: numbers at
# five significant digits, strings <= 80 characters, prose dropped — it lives in DESIGN.md §6), with the roofline-bearing
# legs LAST; the full record goes to gpurun_out/bench_full.json (BENCH_FULL_JSON overrides the path).
LINE_BUDGET = 6144
_HEAD_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline")
_TAIL_KEYS = ("dtype_matrix", "arith_f64", "arbitrary_ratio", "exact_engine", "batch_up", "batch_strong", "configs2", "batch_shard", "throughput_roofline")
_DROP_KEYS = {"note", "launch_us_window", "smi_samples", "taken_on_kernel_sources_sha16", "usable_cpus", "host_cpus", "calls", "regime_note",
              "launch_us_le_step", "algorithmic_bytes_per_launch", "direct_form_equiv_tflops", "buffer_sets", "launches", "seconds", "frac_of_measured_copy"}
# context legs given up first (in this order) if a line still exceeds the budget
_SHED_ORDER = ("host_batch", "host_api", "configs4", "hbm_ceiling", "ranks", "dtype_matrix", "arith_f64")


def _compact(v, key=None):
    if isinstance(v, bool) or v is None or isinstance(v, int):
        return v
    if isinstance(v, float):
        return float("%.5g" % v) if v == v and abs(v) != float("inf") else None
    if isinstance(v, str):
        if key == "bank_sha256":
            return v[:16]
        return v if len(v) <= 80 else v[:77] + "..."
    if isinstance(v, (list, tuple)):
        return [_compact(e) for e in v]
    if isinstance(v, dict):
        # a leg of per-call timings: its us_per_call is the figure
        if "us_per_call" in v and key not in ("sustained",):
            keep = {k: v[k] for k in ("us_per_call", "us_in_call_when_spaced", "streams") if k in v}
            return _compact(keep["us_per_call"]) if len(keep) == 1 else {k: _compact(x) for k, x in keep.items()}
        return {k: _compact(x, k) for k, x in v.items() if k not in _DROP_KEYS}
    return str(v)[:80]


def compact_line(result, budget=LINE_BUDGET):
    """-> the JSON text bench.py prints: every contract key, `roofline` and `cpu_baseline` first, context legs in the
    middle, the roofline-bearing legs (`configs2`, `batch_shard`, `throughput_roofline`, ...) last; <= budget bytes."""
    c = {k: _compact(v, k) for k, v in result.items()}
    if isinstance(c.get("cpu_baseline"), dict):   # the contract's `sample` stays; the context figures' own samples live in the full record
        def strip(d):
            return {k: (strip(v) if isinstance(v, dict) else v) for k, v in d.items() if k != "sample"}
        c["cpu_baseline"] = {k: (strip(v) if isinstance(v, dict) else v) for k, v in c["cpu_baseline"].items()}
    order = [k for k in _HEAD_KEYS if k in c] + [k for k in c if k not in _HEAD_KEYS and k not in _TAIL_KEYS] + [k for k in _TAIL_KEYS if k in c]
    c = {k: c[k] for k in order}
    line = json.dumps(c, separators=(",", ":"))
    if len(line) > budget:   # second level: the ceiling probe's best figures only, per-call legs as bare numbers, shorter strings
        if isinstance(c.get("hbm_ceiling"), dict):
            c["hbm_ceiling"] = {k: v for k, v in c["hbm_ceiling"].items() if k.startswith("best_") or k in ("error", "skipped")}
        for leg in ("configs4", "host_api"):
            if isinstance(c.get(leg), dict):
                c[leg] = {k: (v["us_per_call"] if isinstance(v, dict) and "us_per_call" in v else v) for k, v in c[leg].items() if k != "workload"}

        def shorter(v):
            if isinstance(v, str):
                return v if len(v) <= 48 else v[:45] + "..."
            if isinstance(v, dict):
                return {k: shorter(x) for k, x in v.items()}
            return v
        c = {k: (shorter(v) if k not in ("metric", "config") else v) for k, v in c.items()}
        line = json.dumps(c, separators=(",", ":"))
    shed = []
    for k in _SHED_ORDER:
        if len(line) <= budget:
            break
        if k in c:
            del c[k]
            shed.append(k)
            c["shed_for_line_budget"] = shed   # (named, never silent: the full record still holds them)
            c = {k2: c[k2] for k2 in [x for x in c if x not in _TAIL_KEYS] + [x for x in _TAIL_KEYS if x in c]}
            line = json.dumps(c, separators=(",", ":"))
    return line


DUMP_BYTES = 63 * 10 ** 6   # --dump-outputs: under 64 MB in all, .npy headers included


def dump_outputs(dirname, y, rank, world, budget=DUMP_BYTES):
    """--dump-outputs DIR: what the timed path handed back in its last step (the resampled clip, float32) as
    DIR/resampled.npy; rank r > 0 of an N-GPU run writes DIR/resampled_rank<r>.npy.  An output larger than its share of
    the budget (a long --seconds) is written as every s-th sample from the first on, s the smallest stride that fits:
    the same positions in every run with the same arguments."""
    import numpy as np
    a = y.detach().cpu().numpy().reshape(-1)
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float32)
    stride = -(-a.nbytes // (budget // world))
    if stride > 1:
        a = np.ascontiguousarray(a[::stride])
    os.makedirs(dirname, exist_ok=True)
    path = os.path.join(dirname, "resampled.npy" if rank == 0 else f"resampled_rank{rank}.npy")
    np.save(path, a)
    return path


def write_full_record(result):
    path = os.environ.get("BENCH_FULL_JSON", os.path.join(ROOT, "gpurun_out", "bench_full.json"))
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(result, f, indent=1)
    except OSError:
        pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seconds", type=int, default=60, help="length of the mono clip (configs[1])")
    ap.add_argument("--batch-clips", type=int, default=1024, help="clips in the sharded batch (configs[3])")
    ap.add_argument("--batch-gpus", type=int, default=8, help="GPU count the batch is defined on")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-batch", action="store_true")
    ap.add_argument("--kernel", type=int, default=0)
    ap.add_argument("--strong", action="store_true", help="(kept for older command lines: the strong-scaling batch line is always timed now)")
    ap.add_argument("--windows", type=int, default=50, help="extra timing windows of K launches (median -> launch_us)")
    ap.add_argument("--sustained-s", type=float, default=3.0, help="wall seconds of the sustained batch leg")
    ap.add_argument("--no-sustained", action="store_true")
    ap.add_argument("--kernels-only", action="store_true", help="device-kernel legs only (profiling target: no host API / stream / CPU / ceiling legs)")
    ap.add_argument("--full", action="store_true",
                    help="run every context leg too (batch, configs[2], other engines and precisions, roofline probes, host API, "
                         "CPU baseline) and write the full record; without it only the headline workload is timed")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's output as DIR/resampled.npy (float32)")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(spawn_ranks(args.gpus))     # N ranks, one per GPU; rank 0 of them prints the line

    import torch
    import torch.distributed as dist
    from soxr_amd import device as dev

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks (the line would report the wrong N)")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (there is no CPU fallback)")
    # BENCH_DIST_BACKEND=gloo lets the N > 1 code path be exercised on a box with fewer GPUs than
    # ranks (ranks then share devices; for testing the harness, never for numbers)
    backend = os.environ.get("BENCH_DIST_BACKEND", "nccl")
    dev_index = local_rank if backend == "nccl" else local_rank % torch.cuda.device_count()
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    plan = dev.Plan(IN_RATE, OUT_RATE, QUALITY)
    broadcast_bank(plan, rank, world, device)
    rank_info = gather_rank_info(plan, rank, world, device, backend)
    # what an N-GPU line must have run on: N ranks, RCCL (unless the harness test asked for gloo), one bank everywhere,
    # N distinct devices — anything else is reported as a failure, not as a number
    if world > 1:
        want_backend = "nccl (RCCL)" if backend == "nccl" else backend
        devices_used = {r["device"] for r in rank_info["ranks"]}
        problems = [m for ok, m in ((rank_info["ranks_seen"] == world, f"ranks_seen {rank_info['ranks_seen']} != {world}"),
                                    (rank_info["backend"] == want_backend, f"backend {rank_info['backend']} != {want_backend}"),
                                    (rank_info["banks_identical"], "banks differ between ranks after the broadcast"),
                                    (backend != "nccl" or len(devices_used) == world, f"{len(devices_used)} distinct devices for {world} ranks")) if not ok]
        if problems:
            raise SystemExit("bench.py: multi-GPU run is not what the line would claim: " + "; ".join(problems))

    # ---- configs[1]: 60 s mono float32, one clip per GPU ------------------------------------
    g = torch.Generator(device=device)
    g.manual_seed(1000 + rank)
    n_in = IN_RATE * args.seconds
    x = torch.randn(n_in, device=device, dtype=torch.float32, generator=g) * 0.25
    # (a plain run: no HIP-event windows around the timed steps — launch_us is then the steps' own wall time per step)
    wall, kern, y = time_workload(plan, x, args.steps, args.warmup, world, device, args.kernel,
                                  windows=args.windows if args.full else 0)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, y, rank, world)
    n_out = y.shape[0]
    algo_bytes = 4.0 * (n_in + n_out)
    flops = 2.0 * plan.taps * n_out
    value = world * n_in * args.steps / wall / 1e6
    fft_kernel = args.kernel in (0, 5)
    c1_traffic, c1_valu, c1_prov = measured_counters("configs1") if (fft_kernel and args.seconds == 60) else (None, None, {})

    result = {
        "metric": "Msamples/sec VHQ 48k->44.1k float32 (input samples/s)",
        "value": value, "unit": "Msamples/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": wall / args.steps * 1e3, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"BASELINE configs[1]: VHQ 48000->44100 float32, {args.seconds} s mono, "
                               f"one clip per GPU, device-resident",
                   "quality": QUALITY, "in_rate": IN_RATE, "out_rate": OUT_RATE,
                   "taps_per_phase": plan.taps, "phases": plan.L, "frames_in": n_in, "frames_out": n_out,
                   "parallelism": f"independent clips per rank x{world}; RCCL bank broadcast at plan time"},
        "roofline": {"bound": "hbm", "achieved": algo_bytes / kern / 1e9, "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": algo_bytes / kern / 1e9 / HBM_PEAK_GBS,
                     "traffic": c1_traffic, "kernel": KERNEL_NAMES.get(args.kernel, "auto"), "launch_us": kern * 1e6,
                     "launch_us_le_step": bool(kern <= wall / args.steps),
                     "algorithmic_bytes_per_launch": algo_bytes,
                     "valu_issue_frac": c1_valu / (VALU_SLOTS_PER_S * kern) if c1_valu else None,
                     "direct_form_equiv_tflops": flops / kern / 1e12, **c1_prov},
        "full": args.full,
    }
    if not args.full:   # a plain run ends here: the line, no context legs, no full record
        if rank == 0:
            result["cpu_baseline"] = None
            result["ranks"] = rank_info
            print(compact_line(result))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return
    if rank == 0 and fft_kernel and args.seconds == 60 and not args.no_sustained:
        # what bounds THIS line: one 22 MB buffer pair re-launched — it lives in the 256 MB Infinity Cache, and its 643
        # workgroups are a single round on 1024 slots: latency (launch floor + one workgroup's six passes), not HBM traffic.
        # `throughput_roofline` (the batch, rotating buffers) is the HBM-roofline claim of this benchmark.
        r = result["roofline"]
        r["regime"] = "latency: Infinity-Cache resident (22 MB re-launched), one round of 643 workgroups; the HBM-roofline claim is throughput_roofline"
        r["launch_floor_us"] = launch_floor(device)
        # memory side alone, same grid / LDS / bytes per workgroup (k = 16 periods: 2560 -> 2352-point blocks, 14 kept periods)
        r["floor_us"] = pattern_floor(device, 643, 1, 2 * 2240, 2 * 2058, 2240 + 2560, 2 * 2058, 0, 0, n_in, n_out, 20480, 384, sets=1)
        r.update({k: v for k, v in power_leg(plan, [x], 1.5, device, args.kernel, algo_bytes).items()
                  if k in ("power_W", "sclk_MHz", "energy_mJ_per_launch", "smi_samples")})

    # ---- configs[3] shard: 1024 x 10 s clips over 8 GPUs -> 128 clips per GPU ----------------
    f64_tp = exact_tp = None
    if not args.no_batch:
        lo, hi = shard(args.batch_clips, args.batch_gpus, rank % args.batch_gpus)
        clips = hi - lo
        # buffer sets in rotation: >= 1.4 GB of signal in all, several times the 256 MB Infinity Cache
        b_set_bytes = 4.0 * clips * IN_RATE * 10 * (1 + OUT_RATE / IN_RATE)
        n_sets = max(1, min(6, int(-(-1.4e9 // b_set_bytes))))
        xbs = [torch.randn((clips, IN_RATE * 10, 1), device=device, dtype=torch.float32, generator=g) * 0.25 for _ in range(n_sets)]
        bsteps = max(5, args.steps // 10)
        bwall, bkern, yb = time_workload(plan, xbs, bsteps, max(2, args.warmup // 10), world, device,
                                         args.kernel, windows=max(6, args.windows // 4), min_window=50)
        b_traffic, b_valu, b_prov = measured_counters("batch_shard") if (fft_kernel and clips == 128) else (None, None, {})
        b_in, b_out = clips * IN_RATE * 10, clips * yb.shape[1]
        bbytes = 4.0 * (b_in + b_out)
        # the launch's memory side alone (k = 32 periods: 5120 -> 4704-point blocks, 30 kept periods; pairs of blocks)
        b_floor = pattern_floor(device, (yb.shape[1] + 8819) // 8820, clips, 9600, 8820, 4800 + 5120, 8820, IN_RATE * 10, yb.shape[1],
                                IN_RATE * 10, yb.shape[1], 40960, 384) if (rank == 0 and fft_kernel) else None
        bflops = 2.0 * plan.taps * b_out
        result["batch_shard"] = {
            "workload": f"BASELINE configs[3] shard: {clips} independent 10 s clips per GPU "
                        f"({args.batch_clips} clips / {args.batch_gpus} GPUs), VHQ 48k->44.1k float32",
            "buffer_sets": n_sets,
            "value": world * b_in * bsteps / bwall / 1e6, "unit": "Msamples/s", "steps": bsteps,
            "ms_per_step": bwall / bsteps * 1e3,
            "roofline": {"bound": "hbm", "achieved": bbytes / bkern / 1e9, "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": bbytes / bkern / 1e9 / HBM_PEAK_GBS,
                         "traffic": b_traffic, "valu_issue_frac": b_valu / (VALU_SLOTS_PER_S * bkern) if b_valu else None,
                         "read_frac": 4.0 * b_in / bkern / 1e9 / HBM_PEAK_GBS, "floor_us": b_floor,
                         "launch_us": bkern * 1e6, "launch_us_window": "median of HIP-event windows of >= 50 back-to-back launches",
                         "launch_us_le_step": bool(bkern <= bwall / bsteps),
                         "direct_form_equiv_tflops": bflops / bkern / 1e12, **b_prov}}
        # a sustained leg on the same workload: >= 3 s of back-to-back launches (rank 0's GPU; every rank runs it so the
        # ranks stay in step), with the board power and shader clock rocm-smi reports meanwhile
        if not args.no_sustained:
            sn, sdt, spower = sustained_leg(plan, xbs, args.sustained_s, device, args.kernel, sample_power=(rank == 0))
            result["batch_shard"]["sustained"] = {"seconds": sdt, "launches": sn, "us_per_launch": sdt / sn * 1e6,
                                                  "frac": bbytes / (sdt / sn) / 1e9 / HBM_PEAK_GBS, **spower,
                                                  "energy_mJ_per_launch": spower["power_W"] * sdt / sn * 1e3 if spower.get("power_W") else None,
                                                  "note": "back-to-back launches of the batch_shard job for >= %g s of wall time; power / clock: rocm-smi beside it "
                                                          "(the board's cap is 1400 W: at ~1370 W the launch is power-bound, time = energy / cap)" % args.sustained_s}
            # the same launches on ONE buffer set (what rounds 1-3 timed): with non-temporal result stores the 246 MB input
            # stays in the Infinity Cache from launch to launch — context, not the roofline figure
            if n_sets > 1:
                cn, cdt, _ = sustained_leg(plan, xbs[:1], min(1.0, args.sustained_s), device, args.kernel)
                result["batch_shard"]["one_buffer_set"] = {"us_per_launch": cdt / cn * 1e6, "frac": bbytes / (cdt / cn) / 1e9 / HBM_PEAK_GBS,
                                                           "note": "input re-read from the Infinity Cache: not HBM traffic"}
        # ... and the same batch at the arithmetic width libsoxr's VHQ recipe computes in (float32 I/O, float64 arithmetic):
        # the throughput figure of the `arith_f64` leg — rotating buffer sets, back to back, >= 1 s
        # ... and on the exact (canonical-order) engine: its THROUGHPUT figure — the 60 s clip of `exact_engine` is two rounds of
        # workgroups, a latency line like the headline (profiles/NOTES_r06.md §5)
        exact_tp = None
        if world == 1 and args.kernel == 0 and not args.no_sustained:
            try:
                en, edt, _ = sustained_leg(plan, xbs, min(1.0, args.sustained_s), device, 6)
                eflops = 2.0 * plan.taps * b_out
                exact_tp = {"workload": "batch_shard", "us_per_launch": edt / en * 1e6, "launches": en,
                            "mfma_tflops": eflops / (edt / en) / 1e12, "mfma_frac": eflops / (edt / en) / 1e12 / VALU_PEAK_TFLOPS,
                            "us_per_clip_minute": edt / en * 1e6 * (IN_RATE * 60.0) / b_in}
            except RuntimeError as e:
                exact_tp = {"error": str(e)}
        if world == 1 and args.kernel == 0 and not args.no_sustained:
            try:
                fn, fdt, _ = sustained_leg(plan, xbs, min(1.5, args.sustained_s), device, 8)
                f64_tp = {"workload": "batch_shard", "us_per_launch": fdt / fn * 1e6, "launches": fn,
                          "frac": bbytes / (fdt / fn) / 1e9 / HBM_PEAK_GBS, "read_frac": 4.0 * b_in / (fdt / fn) / 1e9 / HBM_PEAK_GBS}
            except RuntimeError as e:
                f64_tp = {"error": str(e)}
        del xbs, yb
        # the same batch in the UP direction (44.1k -> 48k): 8832 block pairs, which the product hands to the one-wave-per-pair
        # kernel (csrc/fftwave.hip, round 6) — context line: rotating buffer sets, HIP-event windows
        if world == 1 and args.kernel == 0:
            try:
                plan_up = dev.Plan(float(OUT_RATE), float(IN_RATE), QUALITY)
                xus = [torch.randn((clips, OUT_RATE * 10, 1), device=device, dtype=torch.float32, generator=g) * 0.25 for _ in range(min(n_sets, 3))]
                _, uk, yu = time_workload(plan_up, xus, bsteps, 2, world, device, 0, windows=6, min_window=50)
                ubytes = 4.0 * (clips * OUT_RATE * 10 + clips * yu.shape[1])
                u_traffic, _, u_prov = measured_counters("batch_up") if clips == 128 else (None, None, {})
                result["batch_up"] = {"workload": f"{clips} x 10 s clips, VHQ 44.1k->48k float32", "kernel": "k_fft_wave<3528 x 3840> (one wave per block pair)",
                                      "launch_us": uk * 1e6, "frac": ubytes / uk / 1e9 / HBM_PEAK_GBS, "traffic": u_traffic,
                                      "rocprof_avg_us": u_prov.get("rocprof_avg_us")}
                if not args.no_sustained:   # back to back >= 1 s with rocm-smi beside it: the power and clock this kernel runs at
                    un, udt, upower = sustained_leg(plan_up, xus, min(1.0, args.sustained_s), device, 0, sample_power=(rank == 0))
                    result["batch_up"]["sustained"] = {"us_per_launch": udt / un * 1e6, "frac": ubytes / (udt / un) / 1e9 / HBM_PEAK_GBS, **upower,
                                                       "energy_mJ_per_launch": upower["power_W"] * udt / un * 1e3 if upower.get("power_W") else None}
                del xus, yu, plan_up
            except RuntimeError as e:
                result["batch_up"] = {"error": str(e)}
        # the same batch partitioned over THIS job's ranks (strong scaling: 1024 clips in total whatever N is; at N = 1
        # all 1024 clips run on the one GPU — 3.8 GB of signal — which anchors the strong-scaling curve and exercises
        # configs[3] whole)
        slo, shi = shard(args.batch_clips, world, rank)
        xs = torch.randn((shi - slo, IN_RATE * 10, 1), device=device, dtype=torch.float32, generator=g) * 0.25
        swall, skern, ys = time_workload(plan, xs, bsteps, 2, world, device, args.kernel, windows=6)
        result["batch_strong"] = {
            "workload": f"BASELINE configs[3]: {args.batch_clips} x 10 s clips partitioned over {world} rank(s) "
                        f"(soxr_amd.dist.shard(n, world, rank): rank 0 holds clips [{slo}, {shi}))",
            "scaling": "strong", "value": args.batch_clips * IN_RATE * 10 * bsteps / swall / 1e6, "unit": "Msamples/s",
            "ms_per_step": swall / bsteps * 1e3, "launch_us_rank0": skern * 1e6,
            "hbm_frac_rank0": 4.0 * (xs.numel() + ys.numel()) / skern / 1e9 / HBM_PEAK_GBS}
        if world > 1:  # which clips every rank really held (a partition of [0, batch_clips): tests/test_gpu_multi.py)
            import torch.distributed as dist
            held = [None] * world
            dist.all_gather_object(held, [slo, shi])
            result["batch_strong"]["shards"] = held
        del xs, ys

    # ---- configs[2] (context line, not the headline): 60 s x 8 channels interleaved, 44.1k -> 16k VHQ
    if not args.no_batch and world == 1:
        try:
            plan2 = dev.Plan(44100, 16000, QUALITY)
            x2 = torch.randn((44100 * args.seconds, 8), device=device, dtype=torch.float32, generator=g) * 0.25
            w2, k2, y2 = time_workload(plan2, x2, max(5, args.steps // 10), 2, world, device, args.kernel, windows=20)
            bytes2 = 4.0 * (x2.numel() + y2.numel())
            c2_traffic, _, c2_prov = measured_counters("configs2") if (fft_kernel and args.seconds == 60) else (None, None, {})
            result["configs2"] = {"workload": f"BASELINE configs[2]: VHQ 44100->16000 float32, {args.seconds} s x 8 ch "
                                              f"interleaved [frames, 8], device-resident",
                                  "value": x2.numel() / k2 / 1e6, "unit": "Msamples/s", "launch_us": k2 * 1e6,
                                  "roofline": {"bound": "hbm", "achieved": bytes2 / k2 / 1e9, "peak": HBM_PEAK_GBS,
                                               "unit": "GB/s", "frac": bytes2 / k2 / 1e9 / HBM_PEAK_GBS,
                                               "traffic": c2_traffic, "kernel": "k_fft_strided2<4410x1600,float,channel pairs>", **c2_prov}}
            if fft_kernel and args.seconds == 60 and not args.no_sustained:
                r2 = result["configs2"]["roofline"]
                # memory side alone in the best access shape (whole frames, contiguous): 750 blocks of 4410 frames x 8 channels in
                # (hop 3528 frames), 1280 frames x 8 out.  The kernel's OWN shape — 8-byte words at the 32-byte frame stride, four
                # workgroups per line — takes 40 us by itself (tools/ubench/c2_probe.hip, profiles/NOTES_r05.md §3)
                r2["floor_us"] = pattern_floor(device, (y2.shape[0] + 1279) // 1280, 1, 3528 * 8, 1280 * 8, 4410 * 8, 1280 * 8, 0, 0,
                                               x2.numel(), y2.numel(), 0, 256)
                r2["floor_us_own_access_shape"] = 40.1
                x2s = [x2] + [torch.randn_like(x2) * 0.25 for _ in range(2)]    # (rotating: 3 x 115 MB > the Infinity Cache)
                r2["sustained"] = power_leg(plan2, x2s, 1.5, device, args.kernel, bytes2)
                del x2s
            del x2, y2, plan2
        except RuntimeError as e:  # context only
            result["configs2"] = {"error": str(e)}

    # ---- a ratio without an exact bank (reference tests/test_random.py:21-25 draws such rates): 48000 -> 44101 stereo 60 s
    #      as a float32 device job — the two-stage form (FFT engine at 2:1 + a short polyphase stage) against the exact engine
    if not args.no_batch and world == 1 and args.kernel == 0:
        try:
            plan3 = dev.Plan(48000, 44101, QUALITY)
            x3 = torch.randn((IN_RATE * args.seconds, 2), device=device, dtype=torch.float32, generator=g) * 0.25
            _, k3, y3 = time_workload(plan3, x3, max(5, args.steps // 10), 2, world, device, 0, windows=10)
            _, k3e, _ = time_workload(plan3, x3, 5, 2, world, device, 6, windows=4)
            bytes3 = 4.0 * (x3.numel() + y3.numel())
            result["arbitrary_ratio"] = {"workload": f"VHQ 48000->44101 float32, {args.seconds} s stereo interleaved, device-resident (interpolated-phase plan: {plan3.phases} intervals x {plan3.taps} taps)",
                                         "launch_us": k3 * 1e6, "kernel": "two-stage: k_poly2<T2, MQ> (interleaved channel pair per pass) + k_fft (2:1), two launches (csrc/twostage.hip)",
                                         "value": x3.numel() / k3 / 1e6, "unit": "Msamples/s", "hbm_frac": bytes3 / k3 / 1e9 / HBM_PEAK_GBS,
                                         "exact_engine_launch_us": k3e * 1e6, "speedup_over_exact": k3e / k3}
            # ... and the same ratio mono (round 5: the column's two halves run as the pair of k_poly2 / of k_interp_tile's lanes)
            x3m = x3[:, 0].contiguous()
            _, k3m, _ = time_workload(plan3, x3m, max(5, args.steps // 10), 2, world, device, 0, windows=10)
            _, k3me, _ = time_workload(plan3, x3m, 5, 2, world, device, 6, windows=4)
            result["arbitrary_ratio"].update({"mono_launch_us": k3m * 1e6, "mono_exact_engine_launch_us": k3me * 1e6})
            del x3, x3m, y3, plan3
        except RuntimeError as e:  # context only
            result["arbitrary_ratio"] = {"error": str(e)}

    # the canonical-order (bit-exact) engine on the same workloads, for reference
    if args.kernel == 0 and world == 1:
        ew, ek, _ = time_workload(plan, x, max(10, args.steps // 4), 5, world, device, kernel=6, windows=20)
        result["exact_engine"] = {"kernel": KERNEL_NAMES[6], "launch_us": ek * 1e6,
                                  "value": n_in / ek / 1e6, "unit": "Msamples/s",
                                  "hbm_frac": algo_bytes / ek / 1e9 / HBM_PEAK_GBS,
                                  "mfma_tflops": flops / ek / 1e12, "mfma_frac": flops / ek / 1e12 / VALU_PEAK_TFLOPS}
        if exact_tp is not None:
            result["exact_engine"]["throughput"] = exact_tp

    # the headline workload at the arithmetic width libsoxr's VHQ recipe itself computes in: float32 I/O on float64
    # arithmetic (HIPSOXR_KERNEL_FFT_F64; SURVEY.md §0.3, reference src/soxr_ext.cpp:74,228)
    if args.kernel == 0 and world == 1:
        try:
            fw, fk, _ = time_workload(plan, x, max(10, args.steps // 4), 5, world, device, kernel=8, windows=20)
            result["arith_f64"] = {"kernel": "k_fft_pair2<.., double, float> (float32 I/O, float64 arithmetic)", "dtype": "f64 arithmetic, f32 I/O",
                                   "launch_us": fk * 1e6, "value": n_in / fk / 1e6, "unit": "Msamples/s",
                                   "frac": algo_bytes / fk / 1e9 / HBM_PEAK_GBS, "read_frac": 4.0 * n_in / fk / 1e9 / HBM_PEAK_GBS}
        except RuntimeError as e:
            result["arith_f64"] = {"error": str(e)}
        if not args.no_batch and f64_tp is not None:
            result["arith_f64"]["throughput"] = f64_tp

    if rank == 0:
        ceil = hbm_ceiling(device) if not args.kernels_only else {"skipped": "--kernels-only"}
        result["hbm_ceiling"] = ceil
        # the north star words its target against the HBM *read* roofline: input bytes only
        result["roofline"]["read_frac"] = 4.0 * n_in / kern / 1e9 / HBM_PEAK_GBS
        if "best_copy_GBs" in ceil:
            result["roofline"]["frac_of_measured_copy"] = result["roofline"]["achieved"] / ceil["best_copy_GBs"]
            if "batch_shard" in result:
                result["batch_shard"]["roofline"]["frac_of_measured_copy"] = \
                    result["batch_shard"]["roofline"]["achieved"] / ceil["best_copy_GBs"]
    if rank == 0:
        result["ranks"] = rank_info
        if "batch_shard" in result:  # the line that is real HBM traffic (the 22 MB clip lives in the Infinity Cache)
            br = result["batch_shard"]["roofline"]
            # THE roofline fraction of this benchmark: rotating buffers (real HBM traffic), back-to-back launches, i.e. at the
            # clock the board's power cap allows — the sustained leg's figure when it ran, with that clock and energy beside it
            sus = result["batch_shard"].get("sustained") or {}
            result["throughput_roofline"] = {"workload": "batch_shard (configs[3] per-GPU shard), rotating buffer sets, back to back",
                                             "frac": sus.get("frac", br["frac"]), "frac_event_windows": br["frac"],
                                             "read_frac": br["read_frac"], "achieved_GBs": br["achieved"],
                                             "traffic": br["traffic"], "launch_us": sus.get("us_per_launch", br["launch_us"]),
                                             "floor_us": br.get("floor_us"), "sclk_MHz": sus.get("sclk_MHz"), "power_W": sus.get("power_W"),
                                             "energy_mJ_per_launch": sus.get("energy_mJ_per_launch"),
                                             "note": "a profiler spaces launches, the board then throttles less: rocprof_avg_us is expected 5-10 % below launch_us"}
    if rank == 0 and world == 1 and not args.no_batch:
        result["dtype_matrix"] = dtype_matrix(plan, device, args.seconds, args.steps)
        if not args.kernels_only:
            result["configs4"] = configs4_stream()
    if rank == 0 and world == 1 and not args.kernels_only:
        result["host_api"] = host_api_timings()
    if rank == 0 and world == 1 and not args.no_batch and not args.kernels_only:
        try:
            result["host_batch"] = host_batch()
        except Exception as e:  # context only
            result["host_batch"] = {"error": str(e)}
    if rank == 0 and world == 1 and not args.no_cpu and not args.kernels_only:
        result["cpu_baseline"] = cpu_baseline(args.seconds)
    elif rank == 0:
        result["cpu_baseline"] = None

    if rank == 0:
        write_full_record(result)
        print(compact_line(result))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
