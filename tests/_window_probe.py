"""Helper of tests/test_gpu_window_positions.py (and, for the position rules alone, of tests/test_window_oracle.py).

As a program it runs the window jobs of a JSON file (written by the test) on the GPU under the process's HIPSOXR_*
environment — the debug-switch build with HIPSOXR_DEBUG_LAUNCH_LOG, and whatever form switches the test sets for this
child — and writes the results to an .npz:

    python tests/_window_probe.py JOBS.json RESULTS.npz

A job is {"name", "case": [in_rate, out_rate, quality], "dtype", "ch", "seed", "kernel", "k0", "n_out", "in_abs0", "n_in",
"lead", "total", "q", "loud", "dither", "dither_seed", "counter"}.  Its input is frames [lead, lead + n_in) of make_signal(dtype, total,
ch, seed, loud) — the test cuts the same array for the oracle — placed at absolute input index in_abs0; the outputs asked for are
[k0, k0 + n_out).  It is run TWICE through Plan.run: as it stands, and moved down by q whole periods — outputs from k0 - q L,
input at in_abs0 - q M — each into a buffer with GUARD frames of poison either side, the payload pre-filled with NaN (integers: a
sentinel).  Per job: the guarded buffer of the run at the job's own position (`y_<name>`), the SHA-256 of the payload's bytes of
both runs (`h_<name>`, `hs_<name>`), whether the twin's guard frames are untouched (`gs_<name>`), the launch
log's lines of each run (`log_<name>`, `logs_<name>`) and, where "counter" is set, the clip counts (`clips_<name>`: [own, twin]).
Nothing else is compared here.

As a module it holds what both tests derive a job's position from: first_tap, span, position, PLACEMENTS."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, POISON = 8, 12345
INT_SENT = {"int16": -12345, "int32": -123456789}

# ---- positions -------------------------------------------------------------------------------------------------------------
# Output k of an L/M plan with T taps reads inputs [first_tap(k), first_tap(k) + T): the product of k and M is formed in
# Python's integers here, so nothing in this file can wrap.
POSITIONS = ("a_out_2p31", "b_out_2p32", "c_in_2p32", "d_2p40", "e_2p47", "f_2p50")
PLACEMENTS = ("exact", "history5", "late3", "short2")
ODD = 1000003  # how far above the power of two classes (d)-(f) sit


def first_tap(L, M, T, k):
    return k * M // L - (T // 2 - 1)


def span(L, M, T, k0, n_out):
    """input frames that outputs [k0, k0 + n_out) read, from first_tap(k0) on"""
    return first_tap(L, M, T, k0 + n_out - 1) + T - first_tap(L, M, T, k0)


def position(L, M, T, n_out, cls):
    """-> (k0, q): k0 = q L + r of position class cls for a window of n_out outputs, with r no multiple of L (the phase of
    the first output is not 0), r large enough that the window moved down by q periods still has 5 frames of history at
    non-negative input indices, and first_tap(k0) a multiple of 4 (the tile kernels stage an input window that starts there
    in 16-byte words, one that starts 5 frames earlier or 3 later sample by sample)."""
    r_lo = ((T // 2 + 8) * L) // M + 2
    if cls == "a_out_2p31":
        target = 2 ** 31 - n_out // 2
    elif cls == "b_out_2p32":
        target = 2 ** 32 - n_out // 2
    elif cls == "c_in_2p32":  # the middle of the input span at 2^32
        target = ((2 ** 32 - (n_out * M // L + T) // 2 + T // 2) * L) // M
    else:
        target = 2 ** {"d_2p40": 40, "e_2p47": 47, "f_2p50": 50}[cls] + ODD
    q = (target - r_lo) // L
    r = target - q * L
    while r % L == 0 or first_tap(L, M, T, q * L + r) % 4 != 0:
        r += 1
    return q * L + r, q


def class_holds(L, M, T, k0, n_out, cls):
    """the statement of a position class, for the tests to assert"""
    n0, n = first_tap(L, M, T, k0), span(L, M, T, k0, n_out)
    out_straddles = lambda p: k0 < p < k0 + n_out - 1  # noqa: E731
    if cls == "a_out_2p31":
        return out_straddles(2 ** 31)
    if cls == "b_out_2p32":
        return out_straddles(2 ** 32)
    if cls == "c_in_2p32":
        return n0 + 8 < 2 ** 32 < n0 + n - 8 and not k0 <= 2 ** 32 <= k0 + n_out
    p = 2 ** {"d_2p40": 40, "e_2p47": 47, "f_2p50": 50}[cls]
    return p < k0 < p + 2 * ODD + 8 * L


def placement(L, M, T, k0, n_out, how):
    """-> (in_abs0, n_in, lead): the input window of a job, and where it starts in the signal make_signal gives for the
    job — span + 5 frames whose frame 5 is the first tap of output k0."""
    n0, n = first_tap(L, M, T, k0), span(L, M, T, k0, n_out)
    return {"exact": (n0, n, 5),           # exactly what the outputs read
            "history5": (n0 - 5, n + 5, 0),  # spare history, an odd base
            "late3": (n0 + 3, n - 3, 8),    # the first outputs read zeros in front of the window
            "short2": (n0, n - 2, 5)}[how]  # the last outputs read zeros behind it


def make_signal(dtype, frames, ch, seed, loud=0):
    """white noise [frames, ch] of RMS 0.25 — int16: 5000 LSB, or `loud` LSB (clipped to the type: the test picks a level at which
    about one output in a hundred saturates); int32: 2^28"""
    x = np.random.default_rng(seed).standard_normal((frames, ch)) * 0.25
    return {"float32": lambda: x.astype(np.float32), "float64": lambda: x,
            "int16": lambda: np.clip(np.rint(x * (4 * loud if loud else 20000)), -32768, 32767).astype(np.int16),
            "int32": lambda: np.rint(x * 2 ** 30).astype(np.int32)}[dtype]()


# ---- the program -------------------------------------------------------------------------------------------------------------
def log_tail(path, pos):
    if not os.path.exists(path):
        return "", pos
    with open(path) as f:
        f.seek(pos)
        txt = f.read()
    return txt, pos + len(txt)


def guards_hold(buf, n_out):
    """the guard frames either side of the payload untouched"""
    return bool((buf[:GUARD] == POISON).all() and (buf[GUARD + n_out:] == POISON).all())


def main():
    sys.path.insert(0, os.path.join(ROOT, "python-soxr_amd"))
    import torch
    from soxr_amd import device as dev

    with open(sys.argv[1]) as f:
        jobs = json.load(f)
    log_path, pos = os.environ["HIPSOXR_DEBUG_LAUNCH_LOG"], 0
    plans, out = {}, {}
    st = torch.cuda.current_stream().cuda_stream
    for job in jobs:
        name, case, dtype = job["name"], tuple(job["case"]), job["dtype"]
        if case not in plans:
            plans[case] = dev.Plan(*case)
        plan, ch, n_out, n_in = plans[case], job["ch"], job["n_out"], job["n_in"]
        sig = make_signal(dtype, job["total"], ch, job["seed"], job.get("loud", 0))
        x = torch.from_numpy(np.ascontiguousarray(sig[job["lead"]:job["lead"] + n_in])).cuda()
        counter = torch.zeros(1, dtype=torch.int64, device="cuda") if job.get("counter") else None
        counts = []
        for tag, shift in (("", 0), ("s", job["q"])):
            buf = torch.full((n_out + 2 * GUARD, ch), POISON, dtype=x.dtype, device="cuda")
            view = buf[GUARD:GUARD + n_out]
            view[:] = INT_SENT.get(dtype, float("nan"))
            if counter is not None:
                counter.zero_()
            _, pos = log_tail(log_path, pos)
            plan.run(x.data_ptr(), view.data_ptr(), dev._torch_elem(x.dtype), 1, ch, n_in, n_out, (0, ch, 1), (0, ch, 1), stream=st,
                     kernel=job["kernel"], in_abs0=job["in_abs0"] - shift * plan.M, out_k0=job["k0"] - shift * plan.L,
                     clip_counter=None if counter is None else counter.data_ptr(), dither=job["dither"], dither_seed=job["dither_seed"])
            torch.cuda.synchronize()
            lines, pos = log_tail(log_path, pos)
            yh = buf.cpu().numpy()
            out["h" + tag + "_" + name] = np.array(hashlib.sha256(np.ascontiguousarray(yh[GUARD:GUARD + n_out]).tobytes()).hexdigest())
            out["log" + tag + "_" + name] = np.array(lines.strip())
            if tag == "":
                out["y_" + name] = yh
            else:
                out["gs_" + name] = np.array(guards_hold(yh, n_out))
            if counter is not None:
                counts.append(int(counter.item()))
            del buf, view
        if counter is not None:
            out["clips_" + name] = np.array(counts)
        del x
    np.savez(sys.argv[2], **out)
    print("WINDOW_PROBE done: %d jobs" % len(jobs))


if __name__ == "__main__":
    main()
