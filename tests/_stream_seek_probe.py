"""Helper of tests/test_gpu_stream_positions.py.

As a program it runs the stream cases of a JSON file (written by the test) on the GPU under the process's HIPSOXR_*
environment — the debug-switch build, which exports hipsoxr_debug_stream_seek, with HIPSOXR_DEBUG_LAUNCH_LOG and whatever
form switches the test sets for this child — and writes the results to an .npz:

    python tests/_stream_seek_probe.py CASES.json RESULTS.npz

A case is {"name", "surface": "tensor" | "host" | "group", "rates": [in_rate, out_rate, quality], "vr", "engine", "dtype",
"ch", "dither", "seed" (group: one per stream), "loud", "sig_from", "sig_seed", "chunks", "events": {call: [in_rate, out_rate,
slew_len]}, "cap", "resident", "deferred", "seeks": {run: [in_frames, out_frames] or null}} (group: "seeks" is the LIST of
the streams' pairs).  Its input is make_signal of tests/_window_probe.py (sig_from: made in that type, then converted), fed
in `chunks`, then the end of input.  Every run of `seeks` is made twice on ONE handle, each after clear() and — where the run
names a pair — the seek: the run, and its repeat.  A call writes into the middle of a buffer of `cap` frames with GUARD frames
either side, all of it poison.  Per run r of case c: the frames of every call end to end (`y_c_r`), the frames per call, the
flush's calls included (`n_c_r`), delay() after every call (`d_c_r`), whether every element outside each call's result kept
the poison (`g_c_r`), num_clips() (`c_c_r`), the launch log (`log_c_r`), and of the repeat the SHA-256 per call and the
counts, delays, guards and clips (`hr_`, `nr_`, `dr_`, `gr_`, `cr_`).  A group case runs its streams in ONE call per chunk
(`y_c_g<i>`, ...) and then each stream alone (`y_c_s<i>`, ...).  The case named "refusals" records what the seek answers where it
must refuse.  Nothing is compared here.

As a module it holds what the test derives a case's position from: call_counts, periods, class_holds."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _window_probe as wp  # noqa: E402

GUARD, POISON = wp.GUARD, wp.POISON
POSITIONS = ("a_out_2p31", "b_out_2p32", "c_in_2p32", "d_2p40", "e_2p48", "f_2p50")
ODD = wp.ODD
NEAR = 2 ** 24  # classes (d)-(f): this close to the power of two (a period of the L = 4800037 plan is 2^22.2 outputs)


# ---- positions: Python integers, nothing here can wrap ---------------------------------------------------------------------
def avail(L, M, T, N):
    """outputs computable from the first N input frames: the k with floor(k M / L) + T/2 <= N - 1"""
    H = T // 2
    return 0 if N - 1 - H < 0 else ((N - H) * L - 1) // M + 1


def out_len(L, M, N):
    return (2 * N * L + M) // (2 * M)


def call_counts(L, M, T, chunks):
    """frames per call of a synchronous constant-rate stream fed `chunks` with room for everything due; last entry: the flush"""
    n = k = 0
    out = []
    for c in chunks:
        n += c
        a = max(avail(L, M, T, n), k)
        out.append(a - k)
        k = a
    out.append(out_len(L, M, n) - k)
    return out


def crosses_inside_a_call(out0, counts, p):
    """output index p is an output of some call, and not that call's first"""
    start = out0
    for c in counts:
        if start < p < start + c:
            return True
        start += c
    return False


def class_holds(in0, out0, counts, n_in, cls):
    """the statement of a position class for a run seeked to (in0, out0) that emits `counts` frames per call from n_in input frames"""
    total = sum(counts)
    if cls == "a_out_2p31":
        return crosses_inside_a_call(out0, counts, 2 ** 31)
    if cls == "b_out_2p32":
        return crosses_inside_a_call(out0, counts, 2 ** 32)
    if cls == "c_in_2p32":
        return in0 + 8 < 2 ** 32 < in0 + n_in - 8 and not out0 <= 2 ** 32 <= out0 + total
    if cls == "d_2p40":
        return 2 ** 40 < min(in0, out0) < 2 ** 40 + NEAR
    if cls == "e_2p48":
        return 2 ** 48 - NEAR < max(in0 + n_in, out0 + total) < 2 ** 48
    return 2 ** 50 < min(in0, out0) < 2 ** 50 + NEAR


def periods(L, M, counts, n_in, cls):
    """-> q, or None: the whole periods that put a constant-rate run of `counts` in class cls (seek: in q M, out q L).  None where
    no multiple of the period does — a plan whose period is longer than the run cannot straddle a given index."""
    total = sum(counts)
    if cls in ("a_out_2p31", "b_out_2p32"):
        q0 = (2 ** (31 if cls == "a_out_2p31" else 32) - total // 2) // L
    elif cls == "c_in_2p32":
        q0 = (2 ** 32 - n_in // 2) // M
    elif cls == "d_2p40":
        q0 = (2 ** 40 + ODD) // min(L, M) + 1
    elif cls == "e_2p48":
        q0 = (2 ** 48 - 2 ** 20) // max(L, M)
    else:
        q0 = (2 ** 50 + ODD) // min(L, M) + 1
    for dq in (0, 1, -1, 2, -2):
        if class_holds((q0 + dq) * M, (q0 + dq) * L, counts, n_in, cls):
            return q0 + dq
    return None


def clock_pair(counts, n_in, cls):
    """-> (in_frames, out_frames) of class cls for a variable-rate run (any integer pair is a legal clock)"""
    if cls in ("a_out_2p31", "b_out_2p32"):
        p = 2 ** (31 if cls == "a_out_2p31" else 32)
        j = max(range(len(counts) // 2 + 1), key=lambda i: (counts[i] >= 2, i))  # the middle call, or the last before it that emits two
        return 3 * p // 2 + ODD, p - sum(counts[:j]) - counts[j] // 2
    if cls == "c_in_2p32":
        return 2 ** 32 - n_in // 2, 2 ** 31 + 2 ** 30 + ODD
    if cls == "d_2p40":
        return 2 ** 40 + ODD, 2 ** 40 + 3 * ODD
    if cls == "e_2p48":
        return 2 ** 48 - 2 ** 22 - 5, 2 ** 48 - 2 ** 23 + 7
    return 2 ** 50 + ODD, 2 ** 50 + 2 * ODD + 1


def signal(case, stream=0):
    """the input of a case (group: of its stream `stream`): [frames, ch]"""
    total = sum(case["chunks"])
    x = wp.make_signal(case.get("sig_from") or case["dtype"], total, case["ch"], case["sig_seed"] + 977 * stream, case.get("loud", 0))
    return x.astype(wp_dtype(case["dtype"]))


def wp_dtype(name):
    return {"float32": np.float32, "float64": np.float64, "int16": np.int16, "int32": np.int32}[name]


# ---- the program -------------------------------------------------------------------------------------------------------------
def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


class Driver:
    """one handle of a case behind process(chunk or None) -> (frames [n, ch] as numpy, guards intact)"""

    def __init__(self, mods, case, seed):
        torch, dev, soxr, n = mods
        self.m, self.case, self.n = mods, case, n
        self.ch, self.cap, self.np_dt = case["ch"], case["cap"], wp_dtype(case["dtype"])
        rates, q = case["rates"][:2], case["rates"][2]
        if case["surface"] == "host":
            self.obj = soxr.ResampleStream(rates[0], rates[1], self.ch, dtype=case["dtype"], quality=q, vr=case["vr"], dither_seed=seed,
                                           deferred=case.get("deferred", False), resident=case.get("resident", False))
        else:
            self.t_dt = getattr(torch, case["dtype"])
            self.obj = dev.TensorStream(rates[0], rates[1], self.ch, dtype=self.t_dt, quality=q, vr=case["vr"], dither=case["dither"],
                                        dither_seed=seed, engine=case["engine"])
        self.h = self.obj._h
        self.done = C.c_size_t(0)

    def start(self, seek):
        n = self.n
        n.check(n.lib.hipsoxr_stream_clear(self.h))
        if seek is not None:
            n.check(n.lib.hipsoxr_debug_stream_seek(self.h, int(seek[0]), int(seek[1])))

    def set_io_ratio(self, ev):
        self.n.check(self.n.lib.hipsoxr_stream_set_io_ratio(self.h, float(ev[0]) / float(ev[1]), int(ev[2])))

    def process(self, chunk):
        torch, n = self.m[0], self.n
        frames = 0 if chunk is None else len(chunk)
        if self.case["surface"] == "host":
            buf = np.full((GUARD + self.cap + GUARD, self.ch), POISON, self.np_dt)
            optr = buf.ctypes.data + GUARD * self.ch * buf.itemsize
            x = None if chunk is None else np.ascontiguousarray(chunk)
            n.check(n.lib.hipsoxr_stream_process(self.h, None if x is None else x.ctypes.data, frames, optr, self.cap, C.byref(self.done)))
            got = buf
        else:
            buf = torch.full((GUARD + self.cap + GUARD, self.ch), POISON, dtype=self.t_dt, device="cuda")
            optr = buf.data_ptr() + GUARD * self.ch * buf.element_size()
            st = torch.cuda.current_stream().cuda_stream
            n.check(n.lib.hipsoxr_stream_process_device(self.h, None if chunk is None else chunk.data_ptr(), frames, optr, self.cap, C.byref(self.done), st))
            torch.cuda.synchronize()
            got = buf.cpu().numpy()
        k = int(self.done.value)
        return got[GUARD:GUARD + k].copy(), bool((got[:GUARD] == POISON).all() and (got[GUARD + k:] == POISON).all())

    def delay(self):
        return float(self.n.lib.hipsoxr_stream_delay(self.h))

    def clips(self):
        return int(self.n.lib.hipsoxr_stream_num_clips(self.h))


def run_stream(drv, x, chunks, events, seek):
    """one run: clear, seek, the chunks, the flush -> (frames per call, delays, guards)"""
    drv.start(seek)
    parts, delays, guards, pos = [], [], True, 0
    for i, c in enumerate(chunks):
        if str(i) in events:
            drv.set_io_ratio(events[str(i)])
        y, g = drv.process(x[pos:pos + c])
        pos += c
        parts.append(y); delays.append(drv.delay()); guards &= g
    while True:  # the flush, until the stream is dry
        y, g = drv.process(None)
        guards &= g
        delays.append(drv.delay())
        if len(y) == 0:
            break
        parts.append(y)
    return parts, delays, guards


def record(out, key, parts, delays, guards, clips, log, repeat):
    if repeat:
        out["hr_" + key] = np.array([_sha(p) for p in parts] or [""])
        out["nr_" + key], out["dr_" + key], out["gr_" + key], out["cr_" + key] = np.array([len(p) for p in parts]), np.array(delays), np.array(guards), np.array(clips)
    else:
        out["y_" + key] = np.concatenate(parts) if parts else np.zeros(0)
        out["n_" + key], out["d_" + key], out["g_" + key], out["c_" + key] = np.array([len(p) for p in parts]), np.array(delays), np.array(guards), np.array(clips)
        out["log_" + key] = np.array(log.strip())


def main():
    sys.path.insert(0, os.path.join(ROOT, "python-soxr_amd"))
    import torch
    import soxr_amd as soxr
    from soxr_amd import device as dev, _native as n
    n.lib.hipsoxr_debug_stream_seek.restype = C.c_char_p  # (no header declares it: the debug-switch build's own export)
    n.lib.hipsoxr_debug_stream_seek.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    mods = (torch, dev, soxr, n)
    with open(sys.argv[1]) as f:
        cases = json.load(f)
    log_path, lpos = os.environ["HIPSOXR_DEBUG_LAUNCH_LOG"], 0
    out = {}
    keep = []  # every handle lives until the process ends: a deleted stream hands its ring to the next one (engine.cpp's pool), and when a
    #            run moves its ring would then depend on the cases in front of it

    def on_device(case, x):
        return x if case["surface"] == "host" else torch.from_numpy(np.ascontiguousarray(x)).cuda()

    for case in cases:
        name = case["name"]
        if case["surface"] == "refusals":
            drv = Driver(mods, dict(case, surface="tensor"), 0)
            x = on_device(dict(case, surface="tensor"), signal(case))
            q, (L, M) = case["q"], case["LM"]
            seek = n.lib.hipsoxr_debug_stream_seek
            ans = {"fresh_whole": seek(drv.h, q * M, q * L), "cleared": None, "off_period": None, "fed": None, "ended": None, "null": seek(None, 0, 0)}
            n.check(n.lib.hipsoxr_stream_clear(drv.h))
            ans["off_period"] = seek(drv.h, q * M + 1, q * L)
            ans["off_period_out"] = seek(drv.h, q * M, q * L + 1)
            ans["range"] = seek(drv.h, 2 ** 62, 2 ** 62)
            drv.process(x[:case["chunks"][0]])
            ans["fed"] = seek(drv.h, q * M, q * L)
            n.check(n.lib.hipsoxr_stream_clear(drv.h))
            ans["cleared"] = seek(drv.h, q * M, q * L)
            ans["twice"] = seek(drv.h, q * M, q * L)  # (seeked, not fed: its counters are no longer at zero)
            drv.process(None)
            ans["ended"] = seek(drv.h, q * M, q * L)
            n.check(n.lib.hipsoxr_stream_clear(drv.h))
            keep.append(drv)
            out["refusals"] = np.array(json.dumps({k: (v.decode() if v else None) for k, v in ans.items()}))
            continue
        if case["surface"] == "group":
            k = len(case["seeks"])
            drvs = [Driver(mods, dict(case, surface="tensor"), case["seed"][i]) for i in range(k)]
            xs = [on_device(dict(case, surface="tensor"), signal(case, i)) for i in range(k)]
            handles = (C.c_void_p * k)(*[d.h.value for d in drvs])
            cap, ch, es = case["cap"], case["ch"], xs[0].element_size()
            for rep in (False, True):
                for d, sk in zip(drvs, case["seeks"]):
                    d.start(sk)
                _, lpos = wp.log_tail(log_path, lpos)
                parts, delays, guards, pos = [[] for _ in drvs], [[] for _ in drvs], [True] * k, 0
                for c in case["chunks"]:
                    buf = torch.full((k, GUARD + cap + GUARD, ch), POISON, dtype=xs[0].dtype, device="cuda")
                    ins = np.array([x.data_ptr() + pos * ch * es for x in xs], np.uint64)
                    outs = np.array([buf[i].data_ptr() + GUARD * ch * es for i in range(k)], np.uint64)
                    ilens, olens, dones = np.full(k, c, np.uint64), np.full(k, cap, np.uint64), np.zeros(k, np.uint64)
                    n.check(n.lib.hipsoxr_streams_process_device(handles, k, ins.ctypes.data, ilens.ctypes.data, outs.ctypes.data, olens.ctypes.data,
                                                                 dones.ctypes.data, torch.cuda.current_stream().cuda_stream))
                    torch.cuda.synchronize()
                    got = buf.cpu().numpy()
                    pos += c
                    for i in range(k):
                        m = int(dones[i])
                        parts[i].append(got[i, GUARD:GUARD + m].copy())
                        guards[i] &= bool((got[i, :GUARD] == POISON).all() and (got[i, GUARD + m:] == POISON).all())
                        delays[i].append(drvs[i].delay())
                log, lpos = wp.log_tail(log_path, lpos)
                for i, d in enumerate(drvs):  # the flush: handle by handle
                    while True:
                        y, g = d.process(None)
                        guards[i] &= g
                        delays[i].append(d.delay())
                        if len(y) == 0:
                            break
                        parts[i].append(y)
                    record(out, "%s_g%d" % (name, i), parts[i], delays[i], guards[i], d.clips(), log, rep)
            for i, d in enumerate(drvs):  # each stream alone, the same seek and signal
                _, lpos = wp.log_tail(log_path, lpos)
                parts, delays, guards = run_stream(d, xs[i], case["chunks"], {}, case["seeks"][i])
                log, lpos = wp.log_tail(log_path, lpos)
                record(out, "%s_s%d" % (name, i), parts, delays, guards, d.clips(), log, False)
            keep.append(drvs)
            continue
        drv = Driver(mods, case, case["seed"])
        x = on_device(case, signal(case))
        for run, seek in case["seeks"].items():
            for rep in (False, True):
                _, lpos = wp.log_tail(log_path, lpos)
                parts, delays, guards = run_stream(drv, x, case["chunks"], case.get("events", {}), seek)
                log, lpos = wp.log_tail(log_path, lpos)
                record(out, name + "_" + run, parts, delays, guards, drv.clips(), log, rep)
        # after clear() the handle is a fresh stream again
        _, lpos = wp.log_tail(log_path, lpos)
        parts, delays, guards = run_stream(drv, x, case["chunks"], case.get("events", {}), None)
        out["hc_" + name] = np.array([_sha(p) for p in parts] or [""])
        keep.append(drv)
    np.savez(sys.argv[2], **out)
    print("STREAM_SEEK_PROBE done: %d cases" % len(cases))


if __name__ == "__main__":
    main()
