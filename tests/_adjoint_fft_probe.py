"""Helper of tests/test_gpu_adjoint_fft.py: runs adjoint jobs with kernel=KERNEL_ADJOINT_FFT on the GPU under the process's
HIPSOXR_* environment — the debug-switch build with HIPSOXR_DEBUG_LAUNCH_LOG — and writes cotangents, results and launch-log
lines to an .npz:

    python tests/_adjoint_fft_probe.py RESULTS.npz

The lengths of the parity jobs depend on the row of the schedule table the engine takes for the transposed plan, so they are
made here: per (case, type) a first job of 3000 frames names the row in the log (k, hop_out), and the lengths are placed
around the kept run of ONE work item of it (a pair of blocks: 2 hop_out frames) — `lengths()`.  Every job is run twice into
a buffer with 8 guard elements either side of every column, pre-filled with NaN; `same_<name>` says whether both runs gave
the same bytes.  Nothing is compared with a reference here."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "python-soxr_amd"))

GUARD, POISON = 8, 12345.0
torch = dev = dist = K = None  # (loaded by main(): the test module imports this file for its tables and formulas alone)


def _load():
    global torch, dev, dist, K
    import torch as torch_
    from soxr_amd import device as dev_, dist as dist_
    torch, dev, dist, K = torch_, dev_, dist_, dev_.KERNEL_ADJOINT_FFT


PARITY = [(48000, 44100, "VHQ"), (48000, 44100, "HQ"), (44100, 48000, "VHQ"), (44100, 48000, "HQ"), (1, 2, "HQ")]
KINDS = {"f32": np.float32, "f64": np.float64}
# name -> (case, type, layout, clips, channels, n_x): the layouts and forms
LAYOUTS = {
    "pairs8": ((44100, 16000, "HQ"), "f32", "inter", 1, 8, 5003),   # 8 interleaved channels: channel pairs
    "strided3": ((48000, 44100, "HQ"), "f32", "inter", 1, 3, 4001),  # 3 interleaved channels: strided columns
    "planar5": ((48000, 44100, "VHQ"), "f64", "planar", 5, 1, 3001),  # a planar batch of 5 columns
    "block": ((48000, 40000, "HQ"), "f32", "planar", 2, 1, 6007),     # a ratio outside the table: k_fft_block
}
RAGGED_CASE = (48000, 44100, "VHQ")


def transposed_taps(L, M, T):
    """csrc/adjoint_fft_rules.h adj_fft_taps"""
    return (2 * -(-(L * (T // 2) + 1) // M) + 7) // 8 * 8


def hop_out(L, M, T, k):
    """fft.hip fft_kept_run for a block of k periods of a plan (L, M, T): the outputs it keeps"""
    disc = ((T // 2 + 2) * L + M - 1) // M
    lead = (disc + L - 1) // L
    return (k * L - disc - lead * L) // L * L


def lengths(taps, hop):
    item = 2 * hop
    return [1, 7, taps // 2, item - 1, item, item + 1, 3 * item + 5]


def fields(line):
    return dict(tok.split("=", 1) for tok in line.split())


class Log:
    def __init__(self):
        self.path, self.pos = os.environ["HIPSOXR_DEBUG_LAUNCH_LOG"], 0

    def take(self):
        if not os.path.exists(self.path):
            return []
        with open(self.path) as f:
            f.seek(self.pos)
            txt = f.read()
        self.pos += len(txt)
        return [ln for ln in txt.splitlines() if ln.strip()]


def cotangent(name, shape, dtype):
    rng = np.random.default_rng([ord(c) for c in name])
    return rng.standard_normal(shape).astype(dtype)


def run(plan, gy, n_x, layout, log):
    """gy [clips, n_y, channels] (numpy) -> (buffer with guards [clips, GUARD + n_x + GUARD, channels], same bytes twice,
    log lines of the first run).  planar: every (clip, channel) column lies by itself, unit stride."""
    clips, n_y, ch = gy.shape
    g = torch.from_numpy(gy).cuda()
    if layout == "planar":
        g = g.transpose(1, 2).contiguous().transpose(1, 2)
        buf = torch.full((clips, ch, n_x + 2 * GUARD), POISON, dtype=g.dtype, device="cuda").transpose(1, 2)
    else:
        buf = torch.full((clips, n_x + 2 * GUARD, ch), POISON, dtype=g.dtype, device="cuda")
    got = []
    for rep in range(2):
        buf[:, GUARD:GUARD + n_x] = float("nan")
        log.take()
        dev.resample_tensor_adjoint(plan, g, n_x, out=buf[:, GUARD:GUARD + n_x], kernel=K)
        torch.cuda.synchronize()
        if rep == 0:
            lines = log.take()
        got.append(buf.cpu().numpy().copy())
    return got[0], got[0].tobytes() == got[1].tobytes(), lines


def parity(out, log):
    for case in PARITY:
        plan = dev.Plan(*case)
        for kind, dtype in KINDS.items():
            tag = "par_%g_%g_%s_%s" % (case + (kind,))
            n_probe = 3000
            _, _, lines = run(plan, cotangent(tag, (1, plan.out_len(n_probe), 1), dtype), n_probe, "planar", log)
            f = fields(lines[0])
            ns = lengths(transposed_taps(plan.L, plan.M, plan.taps), int(f["hop_out"]))
            out["row_" + tag] = np.array(json.dumps(dict(k=int(f["k"]), hop_out=int(f["hop_out"]), form=f["form"], lengths=ns)))
            for n_x in ns:
                name = "%s_%d" % (tag, n_x)
                gy = cotangent(name, (1, plan.out_len(n_x), 1), dtype)
                buf, same, lines = run(plan, gy, n_x, "planar", log)
                out["gy_" + name], out["gx_" + name], out["same_" + name], out["log_" + name] = gy, buf, np.array(same), np.array("\n".join(lines))


def layouts(out, log):
    for name, (case, kind, layout, clips, ch, n_x) in LAYOUTS.items():
        plan = dev.Plan(*case)
        gy = cotangent(name, (clips, plan.out_len(n_x), ch), KINDS[kind])
        buf, same, lines = run(plan, gy, n_x, layout, log)
        out["gy_" + name], out["gx_" + name], out["same_" + name], out["log_" + name] = gy, buf, np.array(same), np.array("\n".join(lines))


def ragged(out, log):
    """Six mono clips packed at odd offsets with sentinels between them, through the raw entry; then an interleaved stereo
    table through dist.resample_ragged_adjoint.  Each clip also alone (equal-length entry), for the test's comparison."""
    plan = dev.Plan(*RAGGED_CASE)
    _, _, lines = run(plan, cotangent("rag_probe", (1, plan.out_len(3000), 1), np.float32), 3000, "planar", log)
    item = 2 * int(fields(lines[0])["hop_out"])
    n_x = [0, 1, transposed_taps(plan.L, plan.M, plan.taps) // 2, item - 1, item + 1, 3 * item + 5]
    n_y = [plan.out_len(n) for n in n_x]
    gap = 7  # sentinels between clips; odd offsets
    gy_off, gx_off, py, px = [], [], 3, 5
    for a, b in zip(n_y, n_x):
        gy_off.append(py); gx_off.append(px)
        py, px = (py + a + gap) | 1, (px + b + gap) | 1
    gy_all = np.full(py + gap, POISON, np.float32)
    gys = [cotangent("rag_%d" % c, (n,), np.float32) for c, n in enumerate(n_y)]
    for o, g in zip(gy_off, gys):
        gy_all[o:o + len(g)] = g
    gyt = torch.from_numpy(gy_all).cuda()
    gxt = torch.full((px + gap,), POISON, dtype=torch.float32, device="cuda")
    table = np.stack([gy_off, n_y, gx_off, n_x], axis=1).astype(np.int64)
    log.take()
    plan.run_adjoint_ragged(gyt.data_ptr(), gxt.data_ptr(), dev._torch_elem(torch.float32), 1, table, (1, 1), (1, 1),
                            stream=torch.cuda.current_stream().cuda_stream, kernel=K)
    torch.cuda.synchronize()
    out["rag_log"] = np.array("\n".join(log.take()))
    out["rag_table"], out["rag_gy"], out["rag_gx"] = table, gy_all, gxt.cpu().numpy()
    for c, (g, n) in enumerate(zip(gys, n_x)):
        out["rag_alone_%d" % c] = dev.resample_tensor_adjoint(plan, torch.from_numpy(g).cuda(), n, kernel=K).cpu().numpy()
    # interleaved stereo, float64
    n2 = [item + 3, 5, 2 * item + 1]
    g2 = [cotangent("rag2_%d" % c, (plan.out_len(n), 2), np.float64) for c, n in enumerate(n2)]
    log.take()
    gx2 = dist.resample_ragged_adjoint(plan, [torch.from_numpy(g).cuda() for g in g2], n2, kernel=K)
    torch.cuda.synchronize()
    out["rag2_log"] = np.array("\n".join(log.take()))
    out["rag2_n"] = np.array(n2)
    for c, (g, n) in enumerate(zip(g2, n2)):
        out["rag2_gy_%d" % c], out["rag2_gx_%d" % c] = g, gx2[c].cpu().numpy()
        out["rag2_alone_%d" % c] = dev.resample_tensor_adjoint(plan, torch.from_numpy(g).cuda(), n, kernel=K).cpu().numpy()


def main():
    _load()
    out, log = {}, Log()
    parity(out, log)
    layouts(out, log)
    ragged(out, log)
    np.savez(sys.argv[1], **out)
    print("ADJOINT_FFT_PROBE done: %d arrays" % len(out))


if __name__ == "__main__":
    main()
